"""Dev tool (GPU box): what the .zip front-end costs over the by-hand form on the same library, and how it compares with
zipfile on the host (lzma_amd/csrc/xlz_zip.hip), in one process.
    python tools/zip_bench.py [--calls 7] [--small] > profiles/zip_extract.txt

Archives, written at run time by tests/zip_files.py's record writer from corpus.py's text (64 distinct plaintexts each,
repeated; liblzma preset 0, end markers): 4096 x 64 KiB LZMA entries; 1024 x 1 MiB LZMA entries; a mix of 2048 LZMA and
2048 stored entries of 64 KiB.  Rows: every entry, 1 % of the entries, one entry -- each the median of --calls calls,
the forms alternating inside every round:
  zip      ZipFile.extract_device into device memory (verify on)
  by hand  (a) what a caller did before: the same streams as a device-resident Batch -- create, run, results, checks of the
           same CRC32 ranges, pack into the same windows -- and one hipMemcpy per stored entry.  Existing code: the floor;
           the difference is what the front-end costs (or, for stored entries, saves).
  host     (b) zipfile.read of the same entries over 16 processes (measured before this process opens the device).
No threshold is set; the file quotes what was measured."""
import ctypes
import os
import random
import statistics
import sys
import tempfile
import time
import zipfile
import zlib
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _hip():
    H = ctypes.CDLL("libamdhip64.so")
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    H.hipMalloc.argtypes = [ctypes.POINTER(vp), sz]
    H.hipFree.argtypes = [vp]
    H.hipMemcpy.argtypes = [vp, vp, sz, ctypes.c_int]
    return H


def _payload(args):
    seed, n = args
    import zip_files as Z
    p = Z.text(seed, n)
    return Z.lzma_payload(p, preset=0), len(p), zlib.crc32(p)


def build(n_lzma, n_stored, size, pool):
    """-> the archive: entry i is LZMA where i % 2 == 0 or there are no stored ones"""
    import zip_files as Z
    distinct = list(pool.map(_payload, [(9000 + size % 977 + k, size) for k in range(64)]))
    noise = [Z.noise(9100 + k, size) for k in range(16)]
    h = Z.Hand()
    total = n_lzma + n_stored
    for i in range(total):
        if n_stored and i % 2:
            h.stored("s/%06d.bin" % i, noise[i % 16])
        else:
            payload, n, crc = distinct[i % 64]
            h.add("l/%06d.txt" % i, payload, n, crc, 14, flags=2)
    return h.finish(zip64=total > 0xFFFF)


def _host_read(args):
    path, names = args
    n = 0
    with zipfile.ZipFile(path) as z:
        for name in names:
            n += len(z.read(name))
    return n


def host_times(path, names, pool, calls):
    ms = []
    for _ in range(min(calls, 3)):
        t0 = time.perf_counter()
        parts = [names[k::16] for k in range(16) if names[k::16]]
        sum(pool.map(_host_read, [(path, p) for p in parts]))
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def _row(label, ms, n_bytes):
    med = statistics.median(ms)
    print("    %-44s median %9.3f ms (min %.3f, max %.3f, %d calls) %8.2f GB/s decoded" %
          (label, med, min(ms), max(ms), len(ms), n_bytes / (med * 1e-3) / 1e9), flush=True)
    return med


def by_hand(ctx, H, arc, z, wants, d_out, cap):
    """the same work without the front-end -> nothing (asserts the CRCs)"""
    import lzma_amd
    streams, ranges, items, crcs = [], [], [], []
    for i, off, _ in wants:
        e = z.entries[i]
        if e["method"] == 14:
            k = len(streams)
            streams.append(lzma_amd.Stream(arc[e["data_off"] + 9:e["data_off"] + e["comp_size"]], lzma_amd.FMT_LZMA_RAW, out_cap=e["size"],
                                           dict_size=e["dict_size"], props=e["props"]))
            ranges.append((k, 0, e["size"], lzma_amd.CHECK_CRC32))
            items.append((k, 0, e["size"], off))
            crcs.append(e["crc"])
        else:
            H.hipMemcpy(ctypes.c_void_p(d_out + off), ctypes.cast(ctypes.c_char_p(arc[e["data_off"]:e["data_off"] + e["size"]]), ctypes.c_void_p), e["size"], 1)
    if streams:
        b = lzma_amd.Batch(ctx, streams)
        b.run()
        assert all(r[1] >= 0 for r in b.results())
        assert b.checks(ranges) == crcs
        b.pack(items, d_out, cap)
        b.close()


def measure(ctx, H, title, arc, host, calls):
    import lzma_amd
    print("%s: %.1f MiB" % (title, len(arc) / 2**20), flush=True)
    with lzma_amd.ZipFile(arc) as z:
        n = len(z.entries)
        rng = random.Random(19)
        for label, which in (("every entry", list(range(n))), ("1 % of the entries", sorted(rng.sample(range(n), max(n // 100, 1)))), ("one entry", [n // 2])):
            wants, total = z.layout(which, align=256)
            d = ctypes.c_void_p()
            assert H.hipMalloc(ctypes.byref(d), max(total, 1)) == 0
            ms = {"zip": [], "hand": []}
            for k in range(calls + 1):
                t0 = time.perf_counter()
                res = z.extract_device(ctx, wants, d.value, total)
                t1 = time.perf_counter()
                by_hand(ctx, H, arc, z, wants, d.value, total)
                t2 = time.perf_counter()
                assert all(st == 0 for st, _ in res)
                if k:
                    ms["zip"].append((t1 - t0) * 1e3), ms["hand"].append((t2 - t1) * 1e3)
                else:
                    print("  %s (%d entries, %.1f MiB decoded): %s" % (label, len(which), total / 2**20, ctx.last_zip_extract_stats()), flush=True)
            assert H.hipFree(d) == 0
            a = _row("zip: ZipFile.extract_device", ms["zip"], total)
            b = _row("by hand: Batch + checks + pack (+ copies)", ms["hand"], total)
            c = _row("host: zipfile.read over 16 processes", host[label], total)
            print("    zip / by hand: %.3f x; zip / host: %.3f x" % (a / b, a / c), flush=True)


def main():
    args = sys.argv[1:]
    calls, small = 7, False
    while args:
        a = args.pop(0)
        if a == "--calls":
            calls = int(args.pop(0))
        elif a == "--small":
            small = True
        else:
            raise SystemExit("unknown argument " + a)
    import lzma_amd
    from lzma_amd import _native as N
    info = N.library_info()
    print("library build %s, decode kernels %s" % (info["build_id"], info["kernel_id"]), flush=True)
    div = 16 if small else 1
    shapes = [("%d x 64 KiB LZMA entries" % (4096 // div), 4096 // div, 0, 64 << 10), ("%d x 1 MiB LZMA entries" % (1024 // div), 1024 // div, 0, 1 << 20),
              ("%d LZMA + %d stored entries of 64 KiB" % (2048 // div, 2048 // div), 2048 // div, 2048 // div, 64 << 10)]
    # (everything the host makes or measures with worker processes is done before this process opens the device)
    built = []
    with ProcessPoolExecutor(16) as pool, tempfile.TemporaryDirectory() as tmp:
        for title, nl, ns, size in shapes:
            arc = build(nl, ns, size, pool)
            path = os.path.join(tmp, "a.zip")
            with open(path, "wb") as f:
                f.write(arc)
            with zipfile.ZipFile(path) as zf:
                names = zf.namelist()
            n = len(names)
            rng = random.Random(19)
            host = {"every entry": host_times(path, names, pool, calls),
                    "1 % of the entries": host_times(path, [names[i] for i in sorted(rng.sample(range(n), max(n // 100, 1)))], pool, calls),
                    "one entry": host_times(path, [names[n // 2]], pool, calls)}
            built.append((title, arc, host))
    H = _hip()
    ctx = lzma_amd.Context(0)
    for title, arc, host in built:
        measure(ctx, H, title, arc, host, calls)


if __name__ == "__main__":
    main()
