"""Dev tool (GPU box): what the gzip / BGZF / zlib front end and the Adler-32 kernels cost (lzma_amd/csrc/xlz_gz.hip,
xlz_adler_dev.hip).
    python tools/gz_bench.py [--n 4096] [--calls 7] [--no-gib] > profiles/device_gz.txt

(a) The Adler-32 kernels on `--n` ranges of 1 MiB and on ONE range of 1 GiB of a device-resident batch's output, the CRC32
    check kernels beside them IN THE SAME RUN on the same bytes, calls alternating: kernel time by HIP events, medians, and
    the ratio.  The CRC32 kernel is the yardstick; there is no pass mark.
(b) A BGZF file of `--n` blocks of 65 280 input bytes through gz.decode_many_device, verify on: deflate mode 0/1 (the
    kernel) against the same call in deflate mode 2 (host threads), against zlib.decompressobj(-15) per block on 16
    threads, against gzip.decompress on one thread.
(c) `--n` .gz files of 64 KiB, and `--n` zlib streams of 64 KiB, the same way.
(d) ONE ordinary .gz of 1 MiB: a lone wave, expected to lose to the host.  Both times are written down.
Bytes are compared once per form.  Wall-clock figures are of the whole call, uploads included; two warm-up calls, then
medians with min - max."""
import argparse
import concurrent.futures as cf
import gzip
import os
import statistics
import struct
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KIB, MIB, GIB = 1 << 10, 1 << 20, 1 << 30
BGZF_IN = 65280


def raw_deflate(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def gz_member(data, level=6):
    return struct.pack("<BBBBIBB", 0x1F, 0x8B, 8, 0, 0, 0, 255) + raw_deflate(data, level) + struct.pack("<II", zlib.crc32(data), len(data))


def bgzf_block(data, level=6):
    body = raw_deflate(data, level)
    head = struct.pack("<BBBBIBBH", 0x1F, 0x8B, 8, 4, 0, 0, 255, 6) + b"BC" + struct.pack("<HH", 2, 12 + 6 + len(body) + 8 - 1)
    return head + body + struct.pack("<II", zlib.crc32(data), len(data))


def bgzf_file(plains, level=6):
    memo = {}
    return b"".join(memo.setdefault(id(p), bgzf_block(p, level)) for p in plains) + bgzf_block(b"")


def bgzf_bodies(data):
    """the deflate bodies of a BGZF file, by its BSIZE chain (what a host reader hands to its threads)"""
    out, at = [], 0
    while at < len(data):
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        out.append(data[at + 18:at + size - 8])
        at += size
    return out


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
    return "%-66s %9.2f ms  (%.2f - %.2f)  %8.2f GB/s" % (what, med, lo, hi, nbytes / med / 1e6)


def _stored_lzma2(chunks, payload, seed):
    """one LZMA2 stream of `chunks` stored chunks of `payload` random bytes -> (stream, plain bytes)"""
    import numpy as np
    a = np.empty((chunks, payload + 3), dtype=np.uint8)
    a[:, 3:] = np.random.default_rng(seed).integers(0, 256, size=(chunks, payload), dtype=np.uint8)
    a[:, 0], a[0, 0], a[:, 1], a[:, 2] = 2, 1, (payload - 1) >> 8, (payload - 1) & 255
    return a.tobytes() + b"\0", a[:, 3:].tobytes()


def kernels(ctx, n, with_gib, calls=20):
    import ctypes
    import lzma_amd
    from lzma_amd import CHECK_CRC32, _native as N, gz
    L = N.lib()
    L.xlz_internal_adler32_device_timed.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(N.AdlerRange), ctypes.c_size_t,
                                                    ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_double)]

    def adler_ms(base, buf_len, rs):
        arr = (N.AdlerRange * len(rs))(*[N.AdlerRange(o, ln) for o, ln in rs])
        dig, ms = (ctypes.c_uint32 * len(rs))(), ctypes.c_double()
        st = L.xlz_internal_adler32_device_timed(ctx._h, ctypes.c_void_p(base), buf_len, arr, len(rs), dig, ctypes.byref(ms))
        assert st == 0, st
        return list(dig), ms.value

    def pair(label, b, n_streams, size, want_adler, want_crc):
        ptrs = [b.device_output(i)[0] for i in range(n_streams)]
        base = min(ptrs)
        rs = [(p - base, size) for p in ptrs]
        buf_len = max(p - base for p in ptrs) + size
        crc_ranges = [(i, 0, size, CHECK_CRC32) for i in range(n_streams)]
        a_ms, c_ms = [], []
        for k in range(3 + calls):   # alternating: one Adler-32 call, one CRC32 call
            dig, ms = adler_ms(base, buf_len, rs)
            got = b.checks(crc_ranges)
            if k == 0:
                assert all(d == want_adler for d in dig), "wrong Adler-32"
                assert all(g == want_crc for g in got), "wrong CRC32"
            if k >= 3:
                a_ms.append(ms), c_ms.append(ctx.last_check_stats()["kernel_ms"])
        total = n_streams * size
        for name, ms in (("Adler-32", a_ms), ("CRC32 (the yardstick)", c_ms)):
            med = statistics.median(ms)
            print("%-40s %-22s median %8.3f ms (min %.3f, max %.3f; %d calls) %8.1f GB/s" % (label, name, med, min(ms), max(ms), len(ms), total / med / 1e6))
        print("%-40s Adler-32 reads at %.2f x the CRC32 kernel's rate" % (label, statistics.median(c_ms) / statistics.median(a_ms)), flush=True)

    comp, plain = _stored_lzma2(16, 65536, 11)
    b = lzma_amd.Batch(ctx, [lzma_amd.Stream(comp, lzma_amd.FMT_LZMA2_RAW, out_cap=MIB, dict_size=1 << 20) for _ in range(n)])
    b.run()
    assert all(r[0] == MIB and r[1] == 0 for r in b.results())
    pair("%d ranges of 1 MiB" % n, b, n, MIB, zlib.adler32(plain), zlib.crc32(plain))
    b.close()
    if not with_gib:
        return
    comp, plain = _stored_lzma2(16384, 65536, 7)
    b = lzma_amd.Batch(ctx, [lzma_amd.Stream(comp, lzma_amd.FMT_LZMA2_RAW, out_cap=GIB, dict_size=1 << 20)])
    b.run()
    assert b.results()[0][:2] == (GIB, 0)
    pair("ONE range of 1 GiB", b, 1, GIB, zlib.adler32(plain), zlib.crc32(plain))
    b.close()


def front_end(ctx, what, datas, plains, fmt, host_fn, single_fn, calls):
    """datas through gz.decode_many_device in the kernel's mode and in deflate mode 2, against host_fn (16 threads) and
    single_fn (one thread)"""
    import torch
    from lzma_amd import gz
    total = sum(map(len, plains))
    windows, need = gz.layout(datas, caps=[len(p) for p in plains] if fmt == gz.ZLIB else None, align=16, format=fmt)
    dst = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for mode, name in ((1, "the kernel"), (2, "deflate mode 2: host threads")):
        ctx.set_deflate_mode(mode)
        try:
            res = gz.decode_many_device(ctx, datas, dst.data_ptr(), need, windows, format=fmt)
            assert all(r[0] == 0 for r in res), (what, name, [r for r in res if r[0]][:3])
            got = dst.cpu().numpy().tobytes()
            assert b"".join(got[o:o + r[1]] for (o, _), r in zip(windows, res)) == b"".join(plains), (what, name)
            print(_fmt("%s: decode_many_device, verify on, %s" % (what, name),
                       _timed(lambda: gz.decode_many_device(ctx, datas, dst.data_ptr(), need, windows, format=fmt), calls), total))
            print("    ", gz.last_stats(ctx), flush=True)
        finally:
            ctx.set_deflate_mode(0)
    if host_fn:
        with cf.ThreadPoolExecutor(16) as pool:
            assert host_fn(pool) == total
            print(_fmt("%s: zlib on 16 threads" % what, _timed(lambda: host_fn(pool), calls), total))
    if single_fn:
        assert single_fn() == total
        print(_fmt("%s: Python on one thread" % what, _timed(single_fn, calls), total), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--no-gib", action="store_true")
    a = ap.parse_args()
    import torch  # (before the library is loaded: torch's HIP runtime must be the one that initialises the device)
    import corpus
    import lzma_amd
    from lzma_amd import _native as N, gz
    ctx = lzma_amd.Context(0)
    print("gz_bench: library build %s, %s, %d CUs" % (N.lib().xlz_build_id().decode(), torch.cuda.get_device_name(0),
                                                       torch.cuda.get_device_properties(0).multi_processor_count))
    print("\n(a) the Adler-32 kernels beside the CRC32 check kernels, same bytes, same run, kernel time by HIP events")
    kernels(ctx, a.n, not a.no_gib)

    text = [corpus.plain_text(100 + k, 64 * KIB) for k in range(64)]
    print("\n(b) ONE BGZF file of %d blocks of %d input bytes" % (a.n, BGZF_IN))
    blocks = [text[k % 64][:BGZF_IN] for k in range(a.n)]
    f = bgzf_file(blocks)
    bodies = bgzf_bodies(f)
    front_end(ctx, "BGZF, %d blocks" % a.n, [f], [b"".join(blocks)], gz.GZIP,
              lambda pool: sum(pool.map(lambda r: len(zlib.decompressobj(-15).decompress(r)), bodies, chunksize=16)),
              lambda: len(gzip.decompress(f)), a.calls)

    print("\n(c) %d .gz files of 64 KiB; %d zlib streams of 64 KiB" % (a.n, a.n))
    plains = [text[k % 64] for k in range(a.n)]
    memo = {}
    gzs = [memo.setdefault(id(p), gz_member(p)) for p in plains]
    front_end(ctx, "%d .gz files" % a.n, gzs, plains, gz.GZIP,
              lambda pool: sum(pool.map(lambda d: len(zlib.decompressobj(31).decompress(d)), gzs, chunksize=16)),
              lambda: sum(len(gzip.decompress(d)) for d in gzs), a.calls)
    memo = {}
    zs = [memo.setdefault(id(p), zlib.compress(p, 6)) for p in plains]
    front_end(ctx, "%d zlib streams" % a.n, zs, plains, gz.ZLIB,
              lambda pool: sum(pool.map(lambda d: len(zlib.decompress(d)), zs, chunksize=16)),
              lambda: sum(len(zlib.decompress(d)) for d in zs), a.calls)

    print("\n(d) ONE ordinary .gz of 1 MiB: a lone wave against one host thread (the host is expected to win)")
    one = corpus.plain_text(300, MIB)
    g = gz_member(one)
    front_end(ctx, "one .gz of 1 MiB", [g], [one], gz.GZIP, None, lambda: len(gzip.decompress(g)), a.calls)


if __name__ == "__main__":
    main()
