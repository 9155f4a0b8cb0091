"""Dev tool (GPU box): what the device checks (lzma_amd/csrc/xlz_check_dev.hip) cost, in one process.
    python tools/check_bench.py [--parent-so build_ab/parent.so] [--blocks 1024,4096] [--calls 7] [--no-gib] > profiles/device_checks.txt

1. The kernels alone: 4096 x 1 MiB text decoded once into a device-resident batch, then 20 timed Batch.checks calls per
   CRC (the check kernels by HIP events: Context.last_check_stats) after warm-up; the same for ONE stream of 1 GiB
   (stored-chunk LZMA2).  GB/s = bytes read once / time, and its share of the HBM peak.
2. The call a user makes: .xz files of 1 MiB CRC64 blocks as bench.py builds them, through xz_decode_into, check modes 0
   and 1 alternating, medians and min-max; with --parent-so the same file once more through that library (a build of
   the parent commit) in a child process: mode 0 is meant to BE the parent's code path.
Every GPU step is a child process or a call with a time limit of its own around it (the parent run), or this process
under the caller's."""
import ctypes
import os
import statistics
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12       # bytes/s, the part's specification
HBM_MEASURED = 6.29e12  # a float4 copy kernel on the same part


def _rate(label, n_bytes, ms_list):
    med = statistics.median(ms_list)
    gbs = n_bytes / (med * 1e-3) / 1e9
    print("%-44s median %8.3f ms (min %.3f, max %.3f; %d calls)  %8.1f GB/s  %5.1f %% of the 8.0 TB/s peak, %5.1f %% of a copy kernel's 6.29"
          % (label, med, min(ms_list), max(ms_list), len(ms_list), gbs, 100 * gbs * 1e9 / HBM_PEAK, 100 * gbs * 1e9 / HBM_MEASURED), flush=True)


def kernels_alone(ctx, cs, with_gib):
    import check_ref
    import corpus
    import lzma_amd
    from lzma_amd import CHECK_CRC32, CHECK_CRC64
    nd, rep, size = len(cs), 4096 // len(cs), 1 << 20
    streams = [lzma_amd.Stream(c, out_cap=size) for c in cs]
    b = lzma_amd.Batch(ctx, [streams[i % nd] for i in range(nd * rep)])
    b.run()
    res = b.results()
    assert all(r[0] == size and r[1] == 0 for r in res)
    plains = [corpus.plain("T", 501 + i, size) for i in range(nd)]
    for kind, name in ((CHECK_CRC32, "CRC32"), (CHECK_CRC64, "CRC64")):
        ranges = [(i, 0, size, kind) for i in range(nd * rep)]
        want = [check_ref.digest(kind, p) for p in plains]
        ms = []
        for k in range(23):
            got = b.checks(ranges)
            if k == 0:
                assert all(got[i] == want[i % nd] for i in range(nd * rep)), "wrong digest"
            if k >= 3:
                ms.append(ctx.last_check_stats()["kernel_ms"])
        _rate("%d x 1 MiB ranges, %s" % (nd * rep, name), nd * rep * size, ms)
    b.close()
    if not with_gib:
        return
    import numpy as np
    chunks, payload = 16384, 65536   # one stream of 1 GiB in stored LZMA2 chunks
    a = np.empty((chunks, payload + 3), dtype=np.uint8)
    a[:, 3:] = np.random.default_rng(7).integers(0, 256, size=(chunks, payload), dtype=np.uint8)
    a[:, 0], a[0, 0], a[:, 1], a[:, 2] = 2, 1, 0xFF, 0xFF
    want32 = 0
    for i in range(0, chunks, 1024):
        want32 = zlib.crc32(a[i:i + 1024, 3:].tobytes(), want32)
    comp = a.tobytes() + b"\0"
    del a
    b = lzma_amd.Batch(ctx, [lzma_amd.Stream(comp, lzma_amd.FMT_LZMA2_RAW, out_cap=chunks * payload, dict_size=1 << 20)])
    b.run()
    assert b.results()[0][:2] == (chunks * payload, 0), b.results()
    for kind, name in ((CHECK_CRC32, "CRC32"), (CHECK_CRC64, "CRC64")):
        ms = []
        first = None
        for k in range(23):
            got = b.checks([(0, 0, chunks * payload, kind)])
            first = got[0] if first is None else first
            assert got[0] == first
            if k >= 3:
                ms.append(ctx.last_check_stats()["kernel_ms"])
        if kind == CHECK_CRC32:
            assert first == want32, "wrong digest"
        _rate("ONE range of 1 GiB, %s" % name, chunks * payload, ms)
    # (CRC64 of a GiB: liblzma would take minutes; the two halves folded by xlz_crc64_combine must give the whole)
    half = chunks * payload // 2
    h = b.checks([(0, 0, half, CHECK_CRC64), (0, half, half, CHECK_CRC64), (0, 0, 2 * half, CHECK_CRC64)])
    assert lzma_amd.crc64_combine(h[0], h[1], half) == h[2]
    b.close()


def _xz_calls(ctx, data, total, modes, calls):
    """`calls` timed xz_decode_into calls per mode, the modes alternating, after one warm-up call each -> {mode: [ms]}"""
    import lzma_amd
    out = bytearray(total)
    ms = {m: [] for m in modes}
    for k in range(calls + 1):
        for m in modes:
            ctx.set_check_mode(m)
            t0 = time.perf_counter()
            n = lzma_amd.xz_decode_into(ctx, data, out, verify=True)
            dt = (time.perf_counter() - t0) * 1e3
            assert n == total
            if k:
                ms[m].append(dt)
            if m == 1 and k == 1:
                print("    mode 1 check stats: %s" % ctx.last_check_stats(), flush=True)
    ctx.set_check_mode(0)
    return ms


def _parent_child(path, so, calls):
    """child process on the library `so` (no check entry points needed): xlz_xz_decode of the file at `path`"""
    from lzma_amd import _native as N  # noqa: F401  (structures only)
    L = ctypes.CDLL(os.path.abspath(so))
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.xlz_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    L.xlz_xz_index.argtypes = [vp, sz, vp, sz, ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_uint64)]
    L.xlz_xz_decode.argtypes = [vp, vp, sz, vp, sz, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, ctypes.POINTER(sz)]
    L.xlz_build_id.restype = ctypes.c_char_p
    data = open(path, "rb").read()
    ctx = vp()
    assert L.xlz_ctx_create(0, ctypes.byref(ctx)) == 0
    nb, total = sz(), ctypes.c_uint64()
    src = ctypes.c_char_p(data)
    assert L.xlz_xz_index(ctypes.cast(src, vp), len(data), None, 0, ctypes.byref(nb), ctypes.byref(total)) == 0
    out = (ctypes.c_char * total.value)()
    ms = []
    for k in range(calls + 1):
        n, unv = ctypes.c_uint64(), sz()
        t0 = time.perf_counter()
        st = L.xlz_xz_decode(ctx, ctypes.cast(src, vp), len(data), ctypes.cast(out, vp), total.value, ctypes.byref(n), 1, ctypes.byref(unv))
        dt = (time.perf_counter() - t0) * 1e3
        assert st == 0 and n.value == total.value
        if k:
            ms.append(dt)
    print("PARENT %s %s" % (L.xlz_build_id().decode(), " ".join("%.2f" % x for x in ms)))


def _spread(label, ms):
    print("    %-34s median %8.2f ms  min %8.2f  max %8.2f  (%d calls)" % (label, statistics.median(ms), min(ms), max(ms), len(ms)), flush=True)


def user_calls(ctx, files, calls, parent_so):
    if True:
        for blocks, data in files:
            total = blocks << 20
            print("xz file of %d CRC64 blocks of 1 MiB (%.1f MiB compressed), xz_decode_into host to host, verify on:" % (
                blocks, len(data) / 2**20), flush=True)
            ms = _xz_calls(ctx, data, total, (0, 1), calls)
            _spread("mode 0 (host threads, default)", ms[0])
            _spread("mode 1 (device)", ms[1])
            m0, m1 = statistics.median(ms[0]), statistics.median(ms[1])
            spread0 = max(ms[0]) - min(ms[0])
            verdict = "mode 1 is faster" if m0 - m1 > spread0 else "mode 1 is slower" if m1 - m0 > spread0 else "no difference beyond mode 0's own spread"
            print("    medians differ by %.2f ms, mode 0's min-max spread is %.2f ms: %s" % (m0 - m1, spread0, verdict), flush=True)
            if parent_so:
                path = "/dev/shm/xlz_check_bench_%d.xz" % os.getpid()
                with open(path, "wb") as f:
                    f.write(data)
                try:
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--parent-child", path, parent_so, str(calls)],
                                       capture_output=True, text=True, timeout=300, cwd=ROOT)
                finally:
                    os.unlink(path)
                line = [l for l in r.stdout.splitlines() if l.startswith("PARENT ")]
                if r.returncode or not line:
                    print("    parent library: child failed (rc %d): %s" % (r.returncode, r.stderr[-500:]), flush=True)
                else:
                    w = line[0].split()
                    _spread("parent commit's library (%s)" % w[1], [float(x) for x in w[2:]])


def main():
    args = sys.argv[1:]
    if args and args[0] == "--parent-child":
        return _parent_child(args[1], args[2], int(args[3]))
    parent_so, blocks, calls, gib = None, [1024, 4096], 7, True
    while args:
        a = args.pop(0)
        if a == "--parent-so":
            parent_so = args.pop(0)
        elif a == "--blocks":
            blocks = [int(x) for x in args.pop(0).split(",")]
        elif a == "--calls":
            calls = int(args.pop(0))
        elif a == "--no-gib":
            gib = False
        else:
            raise SystemExit("unknown argument " + a)
    import lzma_amd
    from lzma_amd import _native as N
    info = N.library_info()
    print("library build %s, decode kernels %s; check kernels: one wave per 128 KiB segment, LDS 16 KiB (CRC32) / 32 KiB (CRC64) per workgroup of four waves"
          % (info["build_id"], info["kernel_id"]), flush=True)
    # (every worker process has come and gone before this process opens the device)
    import concurrent.futures as cf
    import bench
    import corpus
    cs, _ = corpus.make_alone_batch("T", 64, 1 << 20, base_seed=501, workers=16, preset=0)
    with cf.ProcessPoolExecutor(16) as pool:
        files = [(n, bench.xz_file(pool, n, 1 << 20)[0]) for n in blocks]
    ctx = lzma_amd.Context(0)
    kernels_alone(ctx, cs, gib)
    user_calls(ctx, files, calls, parent_so)


if __name__ == "__main__":
    main()
