"""Dev tool (GPU box): what inflating deflate streams on the device costs (lzma_amd/csrc/xlz_inflate_dev.hip).
    python tools/inflate_bench.py [--small 4096] [--big 1024] [--calls 7] > profiles/device_inflate.txt

1. The kernel alone: lzma_amd.inflate_batch (gather, ONE upload, one launch, the results) of `--small` streams of 64 KiB and
   `--big` streams of 1 MiB of corpus.py text (zlib level 6, 64 distinct plaintexts), and of `--small` x 64 KiB of
   incompressible data (zlib level 0: stored blocks), into device memory; 2 + `--calls` calls each, median and min-max.
   THE ONE-WAVE RATE: one call with ONE stream of 4 MiB of text less one call with one stream of 1 KiB -- a lone wave's
   time for 4 MiB of output -- is what replaces the estimate xlzinf::kWaveBytesPerS behind the launch-length cap.
2. The call a user makes: ZipFile.extract_device (verify on) of an archive of the 64 KiB entries, and of the 1 MiB ones, in
   deflate mode 1 (the kernel) against mode 2 (host threads), against zlib.decompress on 16 threads over the payloads, and
   against zipfile.read over 16 processes (spawned; they never open the device).
3. An archive of mixed LZMA, deflate and stored entries of 64 KiB, mode 1 against mode 2.
Bytes are compared once per form.  Medians, as the project's measuring rules have it; a figure is wall-clock time of the
whole call, so the uploads are in it."""
import argparse
import concurrent.futures as cf
import io
import multiprocessing
import os
import statistics
import struct
import sys
import tempfile
import time
import zipfile
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KIB, MIB = 1 << 10, 1 << 20


def _raw(data, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def _zip(entries):
    """[(name, method, payload, size, crc)] -> the archive (no ZIP64: the callers stay below 4 GiB)"""
    out, central = io.BytesIO(), []
    for name, method, payload, size, crc in entries:
        nm = name.encode()
        flags = 2 if method == 14 else 0
        central.append(struct.pack("<IHHHHHHIIIHHHHHII", 0x02014B50, 63, 63, flags, method, 0, 0x5821, crc, len(payload), size, len(nm), 0, 0, 0, 0,
                                   0, out.tell()) + nm)
        out.write(struct.pack("<IHHHHHIIIHH", 0x04034B50, 63, flags, method, 0, 0x5821, crc, len(payload), size, len(nm), 0) + nm)
        out.write(payload)
    at = out.tell()
    for c in central:
        out.write(c)
    out.write(struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, len(central), len(central), out.tell() - at, at, 0))
    return out.getvalue()


def _timed(fn, calls):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def _fmt(what, t, nbytes):
    med, lo, hi = t
    return "%-58s %9.2f ms  (%.2f - %.2f)  %8.2f GB/s" % (what, med, lo, hi, nbytes / med / 1e6)


def _zipfile_share(job):
    path, lo, hi = job
    n = 0
    with zipfile.ZipFile(path) as z:
        for info in z.infolist()[lo:hi]:
            n += len(z.read(info))
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", type=int, default=4096)
    ap.add_argument("--big", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=7)
    a = ap.parse_args()
    import torch  # (before the library is loaded: torch's HIP runtime must be the one that initialises the device)
    import corpus
    import lzma
    import lzma_amd
    ctx = lzma_amd.Context(0)
    from lzma_amd import _native as N
    print("inflate_bench: library build %s, %s, %d CUs" % (N.lib().xlz_build_id().decode(), torch.cuda.get_device_name(0),
                                                            torch.cuda.get_device_properties(0).multi_processor_count))
    text64 = [corpus.plain_text(100 + k, 64 * KIB) for k in range(64)]
    text1m = [corpus.plain_text(200 + k, MIB) for k in range(16)]
    noise64 = [os.urandom(64 * KIB) for _ in range(64)]
    sets = {"%d x 64 KiB text, level 6" % a.small: ([text64[k % 64] for k in range(a.small)], 6),
            "%d x 1 MiB text, level 6" % a.big: ([text1m[k % 16] for k in range(a.big)], 6),
            "%d x 64 KiB incompressible, stored blocks" % a.small: ([noise64[k % 64] for k in range(a.small)], 0)}
    print("\n1. inflate_batch alone (gather + one upload + one launch + results), into device memory")
    packed = {}
    for what, (plains, level) in sets.items():
        memo = {}
        raws = [memo.setdefault(id(p), _raw(p, level)) for p in plains]
        packed[what] = raws
        items, at = [], 0
        for p, r in zip(plains, raws):
            items.append((r, at, len(p)))
            at += len(p)
        dst = torch.empty(at, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        res = lzma_amd.inflate_batch(ctx, items, dst.data_ptr(), at)
        assert all(st == 0 and n == len(p) for (st, n, _), p in zip(res, plains)), what
        got = dst.cpu().numpy().tobytes()
        assert got[:len(plains[0])] == plains[0] and got[-len(plains[-1]):] == plains[-1], what
        print(_fmt(what + " (%.1f MiB in)" % (sum(map(len, raws)) / MIB), _timed(lambda: lzma_amd.inflate_batch(ctx, items, dst.data_ptr(), at), a.calls), at))
        print("    ", ctx.last_inflate_stats())
        del dst
    one = corpus.plain_text(300, 4 * MIB)
    r_one, r_tiny = _raw(one, 6), _raw(one[:KIB], 6)
    dst = torch.empty(len(one), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t_one = _timed(lambda: lzma_amd.inflate_batch(ctx, [(r_one, 0, len(one))], dst.data_ptr(), len(one)), a.calls)
    t_tiny = _timed(lambda: lzma_amd.inflate_batch(ctx, [(r_tiny, 0, KIB)], dst.data_ptr(), len(one)), a.calls)
    assert dst.cpu().numpy().tobytes() [:KIB] == one[:KIB]
    wave_ms = t_one[0] - t_tiny[0]
    print(_fmt("ONE stream of 4 MiB of text (a lone wave)", t_one, len(one)))
    print(_fmt("one stream of 1 KiB (the call's floor)", t_tiny, KIB))
    print("THE ONE-WAVE RATE: %.1f MB/s of output (4 MiB in %.2f ms); the estimate in xlz_inflate_dev.h was 20 MB/s" % (len(one) / wave_ms / 1e3, wave_ms))

    print("\n2. ZipFile.extract_device, verify on: deflate mode 1 (kernel) / mode 2 (host threads) / zlib on 16 threads / zipfile on 16 processes")
    for what in list(sets)[:2]:
        plains, raws = sets[what][0], packed[what]
        arc = _zip([("e%05d.txt" % k, 8, r, len(p), zlib.crc32(p)) for k, (p, r) in enumerate(zip(plains, raws))])
        total = sum(map(len, plains))
        with lzma_amd.ZipFile(arc) as z:
            wants, need = z.layout(range(len(plains)), align=16)
            dst = torch.empty(need, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            for mode in (1, 2):
                ctx.set_deflate_mode(mode)
                res = z.extract_device(ctx, wants, dst.data_ptr(), need)
                assert all(st == 0 for st, _ in res), (what, mode)
                got = dst.cpu().numpy().tobytes()
                assert got[wants[-1][1]:wants[-1][1] + wants[-1][2]] == plains[-1]
                print(_fmt("%s: extract_device, deflate mode %d" % (what, mode), _timed(lambda: z.extract_device(ctx, wants, dst.data_ptr(), need), a.calls), total))
            ctx.set_deflate_mode(0)
            del dst
        with cf.ThreadPoolExecutor(16) as pool:
            print(_fmt("%s: zlib.decompress on 16 threads" % what,
                       _timed(lambda: sum(pool.map(lambda r: len(zlib.decompressobj(-15).decompress(r)), raws, chunksize=16)), a.calls), total))
        with tempfile.NamedTemporaryFile(suffix=".zip") as f:
            f.write(arc)
            f.flush()
            n = len(plains)
            jobs = [(f.name, n * k // 16, n * (k + 1) // 16) for k in range(16)]
            with cf.ProcessPoolExecutor(16, mp_context=multiprocessing.get_context("spawn")) as pool:
                assert sum(pool.map(_zipfile_share, jobs)) == total
                print(_fmt("%s: zipfile.read over 16 processes" % what, _timed(lambda: sum(pool.map(_zipfile_share, jobs)), a.calls), total))

    print("\n3. a mixed archive: LZMA, deflate and stored entries of 64 KiB, a third each")
    n = a.small // 3 * 3
    lz = {}
    entries = []
    for k in range(n):
        p = text64[k % 64] if k % 3 < 2 else noise64[k % 64]
        if k % 3 == 0:
            if id(p) not in lz:
                props = {"id": lzma.FILTER_LZMA1, "preset": 0, "dict_size": 1 << 16}
                body = lzma.compress(p, format=lzma.FORMAT_RAW, filters=[props])
                lz[id(p)] = struct.pack("<BBH", 9, 20, 5) + bytes([93]) + struct.pack("<I", 1 << 16) + body   # lc 3, lp 0, pb 2
            entries.append(("l%05d" % k, 14, lz[id(p)], len(p), zlib.crc32(p)))
        elif k % 3 == 1:
            entries.append(("d%05d" % k, 8, packed[list(sets)[0]][k % 64], len(p), zlib.crc32(p)))
        else:
            entries.append(("s%05d" % k, 0, p, len(p), zlib.crc32(p)))
    arc = _zip(entries)
    with lzma_amd.ZipFile(arc) as z:
        wants, need = z.layout(range(n), align=16)
        dst = torch.empty(need, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for mode in (1, 2):
            ctx.set_deflate_mode(mode)
            res = z.extract_device(ctx, wants, dst.data_ptr(), need)
            assert all(st == 0 for st, _ in res), ("mixed", mode, [st for st, _ in res if st][:5])
            print(_fmt("%d mixed entries: extract_device, deflate mode %d" % (n, mode), _timed(lambda: z.extract_device(ctx, wants, dst.data_ptr(), need), a.calls),
                       n * 64 * KIB))
        ctx.set_deflate_mode(0)


if __name__ == "__main__":
    main()
