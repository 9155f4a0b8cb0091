"""Dev tool (GPU box): what a read of byte ranges of an .xz file (XzFile: xlz_xz_open / xlz_xz_read_device) costs, in one
process.
    python tools/xz_range_bench.py [--parent-so build_ab/parent.so] [--blocks 1024,4096] [--calls 7] > profiles/xz_ranges.txt

On .xz files of 1 MiB CRC64 blocks as bench.py builds them (every 1024 blocks the same 1024), verify on:
(a) xlz_xz_open against the index parse that xlz_xz_decode repeats on every call (two passes of xlz_xz_index: the counts,
    then the table), on the host, medians of 7.
(b) read_device of one block, of 1 % of the blocks as one range that starts inside a block, of 64 scattered 4 KiB ranges
    and of [0, size), against xlz_xz_decode_device of the whole file through the same library -- without the read the
    only way to those bytes --, the five calls alternating, medians of 7 after a warm-up round that also compares the bytes.
    With --parent-so the whole-file call once more through that library (a build of the parent commit) in a child process.
Every GPU step runs in this process under the caller's time limit, or in a child with one of its own."""
import ctypes
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D2H = 2  # hipMemcpyDeviceToHost


def _hip():
    """the HIP runtime libxlz.so has loaded (and no second one)"""
    path = "libamdhip64.so"
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                path = line.split()[-1]
                break
    H = ctypes.CDLL(path)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    H.hipMalloc.argtypes = [ctypes.POINTER(vp), sz]
    H.hipFree.argtypes = [vp]
    H.hipMemcpy.argtypes = [vp, vp, sz, ctypes.c_int]
    return H


def _ok(st):
    assert st == 0, "HIP call failed: %d" % st


def _spread(label, ms):
    print("    %-58s median %9.3f ms  min %9.3f  max %9.3f  (%d calls)" % (label, statistics.median(ms), min(ms), max(ms), len(ms)), flush=True)
    return statistics.median(ms)


def _whole(ctx, data, dptr, total):
    import lzma_amd
    t0 = time.perf_counter()
    n = lzma_amd.xz_decode_device(ctx, data, dptr, total)
    dt = (time.perf_counter() - t0) * 1e3
    assert n == total
    return dt


def _parent_child(path, calls):
    """(XLZ_SO names the library) the whole-file call alone -> one line: PARENT <kernel id> <ms> ..."""
    import lzma_amd
    from lzma_amd import _native as N
    data = open(path, "rb").read()
    total = lzma_amd.xz_index(data)[1]
    ctx = lzma_amd.Context(0)
    H = _hip()
    dst = ctypes.c_void_p()
    _ok(H.hipMalloc(ctypes.byref(dst), total))
    ms = [_whole(ctx, data, dst.value, total) for _ in range(calls + 1)][1:]
    _ok(H.hipFree(dst))
    print("PARENT %s %s" % (N.lib().xlz_build_id().decode(), " ".join("%.3f" % m for m in ms)), flush=True)


def open_cost(data, calls):
    from lzma_amd import _native as N
    L = N.lib()
    src = ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p)
    t_open, t_index = [], []
    for _ in range(calls + 1):
        h = ctypes.c_void_p()
        t0 = time.perf_counter()
        st = L.xlz_xz_open(src, len(data), ctypes.byref(h))
        t1 = time.perf_counter()
        assert st == 0
        L.xlz_xz_close(h)
        n, total = ctypes.c_size_t(), ctypes.c_uint64()
        t2 = time.perf_counter()
        st = L.xlz_xz_index(src, len(data), None, 0, ctypes.byref(n), ctypes.byref(total))
        blocks = (N.XzBlock * max(n.value, 1))()
        st |= L.xlz_xz_index(src, len(data), blocks, n.value, ctypes.byref(n), ctypes.byref(total))
        t3 = time.perf_counter()
        assert st == 0
        t_open.append((t1 - t0) * 1e3), t_index.append((t3 - t2) * 1e3)
    a = _spread("xlz_xz_open (once per file)", t_open[1:])
    b = _spread("the index parse of every xlz_xz_decode call", t_index[1:])
    print("    open / per-call parse: %.2f x" % (a / b), flush=True)


def reads(ctx, H, data, n_blocks, calls, parent_so):
    import lzma_amd
    size = 1 << 20
    total = n_blocks * size
    f = lzma_amd.XzFile(data)
    assert f.size == total and len(f.blocks) == n_blocks
    rnd = random.Random(n_blocks)
    k = n_blocks // 2
    pct = max(n_blocks // 100, 1)
    cases = [
        ("one block", [(k * size, size)]),
        ("1 %% of the blocks as one range (%d MiB)" % pct, [(k * size + 12345, pct * size)]),
        ("64 scattered 4 KiB ranges", [(rnd.randrange(total - 4096), 4096) for _ in range(64)]),
        ("[0, size)", [(0, total)]),
    ]
    whole, dst = ctypes.c_void_p(), ctypes.c_void_p()
    _ok(H.hipMalloc(ctypes.byref(whole), total))
    _ok(H.hipMalloc(ctypes.byref(dst), total))
    ms = {name: [] for name, _ in cases}
    ms["whole"] = []
    stats = {}
    for rnd_k in range(calls + 1):
        dt = _whole(ctx, data, whole.value, total)
        if rnd_k:
            ms["whole"].append(dt)
        for name, ranges in cases:
            laid, at = [], 0
            for off, n in ranges:
                laid.append((off, n, at))
                at += n
            t0 = time.perf_counter()
            copied = f.read_device(ctx, laid, dst.value, total)
            dt = (time.perf_counter() - t0) * 1e3
            assert copied == [n for _, n in ranges]
            if rnd_k:
                ms[name].append(dt)
                continue
            stats[name] = ctx.last_xz_read_stats()
            for off, n, d in laid[:4]:  # the bytes are the whole-file call's (the first ranges, at most 4 MiB of each)
                m = min(n, 4 << 20)
                a, b = (ctypes.c_char * m)(), (ctypes.c_char * m)()
                _ok(H.hipMemcpy(ctypes.cast(a, ctypes.c_void_p), ctypes.c_void_p(whole.value + off), m, D2H))
                _ok(H.hipMemcpy(ctypes.cast(b, ctypes.c_void_p), ctypes.c_void_p(dst.value + d), m, D2H))
                assert a.raw == b.raw, "wrong bytes: " + name
    w = _spread("xz_decode_device of the whole file", ms["whole"])
    for name, _ in cases:
        m = _spread("read_device of " + name, ms[name])
        s = stats[name]
        print("        %d blocks decoded (%.1f MiB of payload), %d bytes copied; whole file / read: %.1f x"
              % (s["blocks"], s["comp_bytes"] / 2**20, s["copied_bytes"], w / m), flush=True)
    _ok(H.hipFree(whole))
    _ok(H.hipFree(dst))
    f.close()
    if parent_so:
        path = "/dev/shm/xlz_range_bench_%d.xz" % os.getpid()
        with open(path, "wb") as fh:
            fh.write(data)
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--parent-child", path, str(calls)], capture_output=True, text=True,
                               timeout=300, cwd=ROOT, env=dict(os.environ, XLZ_SO=os.path.abspath(parent_so)))
        finally:
            os.unlink(path)
        line = [l for l in r.stdout.splitlines() if l.startswith("PARENT ")]
        if r.returncode or not line:  # (it may have faulted the device: nothing more is started on it)
            raise SystemExit("parent library: child failed (rc %d): %s" % (r.returncode, r.stderr[-500:]))
        else:
            v = line[0].split()
            p = _spread("parent commit's library (%s), whole file" % v[1], [float(x) for x in v[2:]])
            print("    whole file, this library / parent's: %.2f x" % (w / p), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--parent-child":
        return _parent_child(args[1], int(args[2]))
    parent_so, blocks, calls = None, [1024, 4096], 7
    while args:
        a = args.pop(0)
        if a == "--parent-so":
            parent_so = args.pop(0)
        elif a == "--blocks":
            blocks = [int(x) for x in args.pop(0).split(",")]
        elif a == "--calls":
            calls = int(args.pop(0))
        else:
            raise SystemExit("unknown argument " + a)
    import lzma_amd
    from lzma_amd import _native as N
    info = N.library_info()
    print("library build %s, decode kernels %s" % (info["build_id"], info["kernel_id"]), flush=True)
    # (every worker process has come and gone before this process opens the device)
    import concurrent.futures as cf
    import bench
    with cf.ProcessPoolExecutor(16) as pool:
        unit = bench.xz_file(pool, min(1024, min(blocks)), 1 << 20)[0]
    unit_blocks = min(1024, min(blocks))
    ctx = lzma_amd.Context(0)
    H = _hip()
    for n in blocks:
        data = unit * (n // unit_blocks)
        print("xz file of %d CRC64 blocks of 1 MiB (%.1f MiB compressed), verify on:" % (n, len(data) / 2**20), flush=True)
        open_cost(data, calls)
        reads(ctx, H, data, n // unit_blocks * unit_blocks, calls, parent_so)


if __name__ == "__main__":
    main()
