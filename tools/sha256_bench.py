"""Dev tool (GPU box): what SHA-256 on the device (lzma_amd/csrc/xlz_sha256_dev.hip) costs, in one process.
    python tools/sha256_bench.py [--parent-so build_ab/parent.so] [--blocks 1024,4096] [--calls 7] [--only kernel|calls] > profiles/device_sha256.txt

1. The kernel alone: a device-resident batch of 256 streams of 16 MiB (stored-chunk LZMA2: decoded once), then ranges of it
   in three shapes -- 65 536 x 64 KiB, 4096 x 1 MiB, 256 x 16 MiB -- through the kernel itself (the library's launch
   entry, not the plan: the plan would refuse the long ranges), 20 timed launches per shape by HIP events after warm-up:
   median (min-max), GB/s, MB/s per lane.  And xlzcheck::sha256 on 16 host threads over the same bytes.  These are the
   two rates xlz_sha256_plan has built in.
2. The call a user makes: .xz files of one-block streams with SHA-256 checks, 1 MiB blocks, through xz_decode_into host to
   host with verify on, check modes 1 and 2 alternating, medians and min-max; with --parent-so the same file through that
   library (a build of the parent commit) in a child process: mode 1 is meant to BE the parent's code path.  And a file
   of 16 blocks of 8 MiB, which the plan must leave to the host.
Every GPU step is a child process with a time limit of its own (the parent run), or this process under the caller's."""
import ctypes
import lzma
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from check_bench import _spread  # noqa: E402


def _sha_block(args):
    import corpus
    seed, size = args
    p = corpus.plain("T", seed, size)
    return lzma.compress(p, format=lzma.FORMAT_XZ, check=lzma.CHECK_SHA256, preset=0), p


def sha_file(pool, blocks, size, distinct=64):
    """-> (.xz file of `blocks` one-block streams with SHA-256 checks, the plaintext); `distinct` different blocks"""
    res = list(pool.map(_sha_block, [(7000 + i, size) for i in range(min(distinct, blocks))]))
    return b"".join(res[k % len(res)][0] for k in range(blocks)), b"".join(res[k % len(res)][1] for k in range(blocks))


def kernel_alone(ctx):
    import hashlib
    import numpy as np
    import lzma_amd
    from lzma_amd import CHECK_SHA256 as SHA
    n_streams, size, payload = 256, 16 << 20, 65536
    chunks = size // payload
    a = np.empty((chunks, payload + 3), dtype=np.uint8)
    a[:, 3:] = np.random.default_rng(11).integers(0, 256, size=(chunks, payload), dtype=np.uint8)
    a[:, 0], a[0, 0], a[:, 1], a[:, 2] = 2, 1, 0xFF, 0xFF
    plain = a[:, 3:].tobytes()
    comp = a.tobytes() + b"\0"
    del a
    s = lzma_amd.Stream(comp, lzma_amd.FMT_LZMA2_RAW, out_cap=size, dict_size=1 << 20)
    b = lzma_amd.Batch(ctx, [s] * n_streams)
    b.run()
    assert all(r[:2] == (size, 0) for r in b.results())
    rates = []
    for n_ranges, length in ((65536, 64 << 10), (4096, 1 << 20), (256, 16 << 20)):
        per = size // length
        ranges = [(i // per, (i % per) * length, length, SHA) for i in range(n_ranges)]
        want = [hashlib.sha256(plain[k * length:(k + 1) * length]).digest() for k in range(per)]
        ms = []
        n_timed = 20 if length <= 1 << 20 else 5   # (a launch of 16 MiB ranges takes most of a second: five are enough)
        for k in range(n_timed + 2):
            got, kernel_ms = b._sha256_kernel(ranges)
            if k == 0:
                assert all(got[i] == want[i % per] for i in range(n_ranges)), "wrong digest"
            if k >= 2:
                ms.append(kernel_ms)
        med = statistics.median(ms)
        total = n_ranges * length
        lane = length / (med * 1e-3)
        print("%6d ranges of %8d bytes: median %9.3f ms (min %.3f, max %.3f; %d launches)  %7.1f GB/s  %6.2f MB/s per lane, %d waves"
              % (n_ranges, length, med, min(ms), max(ms), len(ms), total / (med * 1e-3) / 1e9, lane / 1e6, (n_ranges + 63) // 64), flush=True)
        rates.append(lane)
    b.close()
    # the host's code, sixteen threads, the 4096 x 1 MiB shape
    L = lzma_amd._native.lib()
    L.xlz_internal_sha256_host_bench.restype = ctypes.c_double
    L.xlz_internal_sha256_host_bench.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32]
    buf = ctypes.create_string_buffer(plain[: 1 << 20], 1 << 20)
    hs = [L.xlz_internal_sha256_host_bench(ctypes.cast(buf, ctypes.c_void_p), 1 << 20, 4096, 16) for _ in range(5)]
    med = statistics.median(hs)
    print("host: xlzcheck::sha256, 4096 x 1 MiB on 16 threads: median %.1f ms (min %.1f, max %.1f; 5 runs)  %.2f GB/s  %.1f MB/s per thread"
          % (med * 1e3, min(hs) * 1e3, max(hs) * 1e3, 4096 * 2**20 / med / 1e9, 4096 * 2**20 / med / 16 / 1e6), flush=True)
    print("rates for the plan: lane %.1f MB/s (the slowest of the shapes with at most two waves per SIMD), host thread %.1f MB/s"
          % (min(rates[1:]) / 1e6, 4096 * 2**20 / med / 16 / 1e6), flush=True)


def _parent_child(path, so, calls):
    """child process on the library `so` (a build of the parent commit: no SHA-256 entry points needed): xlz_xz_decode of
    the file at `path` in check mode 1"""
    L = ctypes.CDLL(os.path.abspath(so))
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.xlz_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    L.xlz_ctx_set_check_mode.argtypes = [vp, ctypes.c_int]
    L.xlz_xz_index.argtypes = [vp, sz, vp, sz, ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_uint64)]
    L.xlz_xz_decode.argtypes = [vp, vp, sz, vp, sz, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, ctypes.POINTER(sz)]
    L.xlz_build_id.restype = ctypes.c_char_p
    data = open(path, "rb").read()
    ctx = vp()
    assert L.xlz_ctx_create(0, ctypes.byref(ctx)) == 0
    assert L.xlz_ctx_set_check_mode(ctx, 1) == 0
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


def _xz_calls(ctx, data, total, modes, calls):
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
            if m == 2 and k == 1:
                print("    mode 2 sha256 stats: %s" % ctx.last_sha256_stats(), flush=True)
    ctx.set_check_mode(0)
    return ms


def user_calls(ctx, files, calls, parent_so):
    for label, data, total in files:
        print("xz file of %s (%.1f MiB compressed), xz_decode_into host to host, verify on:" % (label, len(data) / 2**20), flush=True)
        ms = _xz_calls(ctx, data, total, (1, 2), calls)
        _spread("mode 1 (SHA-256 on host threads)", ms[1])
        _spread("mode 2 (SHA-256 by the plan)", ms[2])
        m1, m2 = statistics.median(ms[1]), statistics.median(ms[2])
        spread1 = max(ms[1]) - min(ms[1])
        verdict = "mode 2 is faster" if m1 - m2 > spread1 else "mode 2 is slower" if m2 - m1 > spread1 else "no difference beyond mode 1's own spread"
        print("    medians differ by %.2f ms, mode 1's min-max spread is %.2f ms: %s" % (m1 - m2, spread1, verdict), flush=True)
        if parent_so:
            path = "/dev/shm/xlz_sha256_bench_%d.xz" % os.getpid()
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
                _spread("parent commit's library (%s), mode 1" % w[1], [float(x) for x in w[2:]])


def main():
    args = sys.argv[1:]
    if args and args[0] == "--parent-child":
        return _parent_child(args[1], args[2], int(args[3]))
    parent_so, blocks, calls, only = None, [1024, 4096], 7, None
    while args:
        a = args.pop(0)
        if a == "--parent-so":
            parent_so = args.pop(0)
        elif a == "--blocks":
            blocks = [int(x) for x in args.pop(0).split(",")]
        elif a == "--calls":
            calls = int(args.pop(0))
        elif a == "--only":
            only = args.pop(0)
        else:
            raise SystemExit("unknown argument " + a)
    import lzma_amd
    from lzma_amd import _native as N
    info = N.library_info()
    print("library build %s, decode kernels %s; SHA-256 kernel: one lane per range, one wave per workgroup" % (info["build_id"], info["kernel_id"]),
          flush=True)
    files = []
    if only != "kernel":   # (every worker process has come and gone before this process opens the device)
        import concurrent.futures as cf
        with cf.ProcessPoolExecutor(16) as pool:
            for n in blocks:
                f, p = sha_file(pool, n, 1 << 20)
                files.append(("%d SHA-256 blocks of 1 MiB" % n, f, len(p)))
            f, p = sha_file(pool, 16, 8 << 20, distinct=4)
            files.append(("16 SHA-256 blocks of 8 MiB", f, len(p)))
    ctx = lzma_amd.Context(0)
    if only != "calls":
        kernel_alone(ctx)
    if only != "kernel":
        user_calls(ctx, files, calls, parent_so)


if __name__ == "__main__":
    main()
