"""Dev tool (GPU box): what the pack into device memory (lzma_amd/csrc/xlz_pack_dev.hip) and the device-destination
front-ends cost, in one process.
    python tools/pack_bench.py [--parent-so build_ab/parent.so] [--blocks 1024,4096] [--calls 7] [--no-kernel] > profiles/device_pack.txt

(a) The kernel alone: 4096 x 1 MiB and 65 536 x 64 KiB streams decoded once into a device-resident batch, then packed whole
    and back to back into one buffer, at destination offsets congruent with the arena modulo 16 and moved off by 5 bytes;
    the kernel by HIP events (Context.last_pack_stats) and the call by the wall clock, medians of 7 after a warm-up.
    Beside it what a caller can do without the pack -- one hipMemcpyAsync device to device per stream from
    Batch.device_output into the same buffer, by HIP events around the loop and by the wall clock -- and the roof: ONE
    hipMemcpy device to device of the same total.
(b) xz_decode_device against xz_decode_into (host to host) on .xz files of 1 MiB CRC64 blocks as bench.py builds them, the
    context in check mode 0 and in check mode 1, the calls alternating, medians of 7; with --parent-so the host-to-host
    call once more through that library (a build of the parent commit) in a child process (tools/check_bench.py's).
(c) The same for one .7z archive of 1024 LZMA2 folders of 1 MiB with folder CRCs.
Every GPU step runs in this process under the caller's time limit, or in a child with one of its own."""
import ctypes
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

D2D = 3  # hipMemcpyDeviceToDevice


def _hip():
    H = ctypes.CDLL("libamdhip64.so")
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    H.hipMalloc.argtypes = [ctypes.POINTER(vp), sz]
    H.hipFree.argtypes = [vp]
    H.hipMemset.argtypes = [vp, ctypes.c_int, sz]
    H.hipMemcpy.argtypes = [vp, vp, sz, ctypes.c_int]
    H.hipMemcpyAsync.argtypes = [vp, vp, sz, ctypes.c_int, vp]
    H.hipEventCreate.argtypes = [ctypes.POINTER(vp)]
    H.hipEventRecord.argtypes = [vp, vp]
    H.hipEventSynchronize.argtypes = [vp]
    H.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), vp, vp]
    return H


def _ok(st):
    assert st == 0, "HIP call failed: %d" % st


def _line(label, n_bytes, ms, wall=None):
    med = statistics.median(ms)
    txt = "    %-46s median %8.3f ms (min %.3f, max %.3f)  %8.1f GB/s" % (label, med, min(ms), max(ms), n_bytes / (med * 1e-3) / 1e9)
    if wall:
        txt += "   call by the wall clock: median %8.3f ms" % statistics.median(wall)
    print(txt, flush=True)
    return med


def kernel_alone(ctx, H, n_streams, size, calls):
    import corpus
    import lzma_amd
    nd = 64 if size >= 1 << 20 else 256
    cs, _ = corpus.make_alone_batch("T", nd, size, base_seed=801, workers=16, preset=0)
    streams = [lzma_amd.Stream(c, out_cap=size) for c in cs]
    b = lzma_amd.Batch(ctx, [streams[i % nd] for i in range(n_streams)])
    b.run()
    assert all(r[0] == size and r[1] == 0 for r in b.results())
    total = n_streams * size
    print("%d streams of %d KiB (%.1f GiB), packed whole and back to back:" % (n_streams, size >> 10, total / 2**30), flush=True)
    dst, dst2 = ctypes.c_void_p(), ctypes.c_void_p()
    _ok(H.hipMalloc(ctypes.byref(dst), total + 256))
    _ok(H.hipMalloc(ctypes.byref(dst2), total + 256))
    ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p()
    _ok(H.hipEventCreate(ctypes.byref(ev0)))
    _ok(H.hipEventCreate(ctypes.byref(ev1)))
    med = {}
    for name, shift in (("congruent modulo 16", 0), ("destination moved off by 5 bytes", 5)):
        items = [(i, 0, size, i * size + shift) for i in range(n_streams)]
        ms, wall = [], []
        for k in range(calls + 1):
            t0 = time.perf_counter()
            copied = b.pack(items, dst.value, total + 256)
            dt = (time.perf_counter() - t0) * 1e3
            ps = ctx.last_pack_stats()
            assert sum(copied) == total and ps["congruent_items"] == (n_streams if shift == 0 else 0)
            if k:
                ms.append(ps["kernel_ms"]), wall.append(dt)
        med[shift] = _line("pack kernel, " + name, total, ms, wall)
    # the bytes are what the arena holds (a sample of the streams, through the host)
    got = (ctypes.c_char * size)()
    for i in (0, 1, n_streams // 2, n_streams - 1):
        _ok(H.hipMemcpy(ctypes.cast(got, ctypes.c_void_p), ctypes.c_void_p(dst.value + i * size + 5), size, 2))
        assert got.raw == b.download(i, size), "wrong bytes"
    srcs = [b.device_output(i)[0] for i in range(n_streams)]
    ms, wall = [], []
    for k in range(calls + 1):
        t0 = time.perf_counter()
        _ok(H.hipEventRecord(ev0, None))
        for i in range(n_streams):
            H.hipMemcpyAsync(dst.value + i * size, srcs[i], size, D2D, None)
        _ok(H.hipEventRecord(ev1, None))
        _ok(H.hipEventSynchronize(ev1))
        dt = (time.perf_counter() - t0) * 1e3
        e = ctypes.c_float()
        _ok(H.hipEventElapsedTime(ctypes.byref(e), ev0, ev1))
        if k:
            ms.append(e.value), wall.append(dt)
    per_stream = _line("one hipMemcpyAsync per stream (ctypes loop)", total, ms, wall)
    ms = []
    for k in range(calls + 1):
        _ok(H.hipEventRecord(ev0, None))
        _ok(H.hipMemcpy(dst2, dst, total, D2D))
        _ok(H.hipEventRecord(ev1, None))
        _ok(H.hipEventSynchronize(ev1))
        e = ctypes.c_float()
        _ok(H.hipEventElapsedTime(ctypes.byref(e), ev0, ev1))
        if k:
            ms.append(e.value)
    roof = _line("ONE hipMemcpy device to device (the roof)", total, ms)
    print("    pack / per-stream copies: %.2f x (congruent), %.2f x (moved off); pack / roof: %.2f x, %.2f x; moved off / congruent: %.2f x"
          % (med[0] / per_stream, med[5] / per_stream, med[0] / roof, med[5] / roof, med[5] / med[0]), flush=True)
    H.hipFree(dst), H.hipFree(dst2)
    b.close()


def _spread(label, ms):
    print("    %-44s median %8.2f ms  min %8.2f  max %8.2f  (%d calls)" % (label, statistics.median(ms), min(ms), max(ms), len(ms)), flush=True)
    return statistics.median(ms)


def _sevenzip_into(ctx, data, out, verify=True):
    """xlz_7z_decode with the caller's buffers and nothing else (what xz_decode_into is for .xz)"""
    from lzma_amd import _native as N
    dst = (ctypes.c_char * len(out)).from_buffer(out)
    n, unverified = ctypes.c_uint64(), ctypes.c_size_t()
    st = N.lib().xlz_7z_decode(ctx._h, ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p), len(data), ctypes.cast(dst, ctypes.c_void_p),
                               len(out), ctypes.byref(n), 1 if verify else 0, ctypes.byref(unverified))
    assert st == 0, st
    return n.value


def front_end(ctx, H, what, data, total, calls, parent_so):
    """host to host against into device memory, check modes 0 and 1, the four calls alternating"""
    import lzma_amd
    host = lzma_amd.xz_decode_into if what == "xz" else _sevenzip_into
    dev_fn = lzma_amd.xz_decode_device if what == "xz" else lzma_amd.sevenzip_decode_device
    out = bytearray(total)
    dst = ctypes.c_void_p()
    _ok(H.hipMalloc(ctypes.byref(dst), total))
    ms = {(m, f): [] for m in (0, 1) for f in ("host", "device")}
    for k in range(calls + 1):
        for m in (0, 1):
            ctx.set_check_mode(m)
            t0 = time.perf_counter()
            n = host(ctx, data, out, verify=True)
            t1 = time.perf_counter()
            n2 = dev_fn(ctx, data, dst.value, total)
            t2 = time.perf_counter()
            assert n == n2 == total
            if k:
                ms[(m, "host")].append((t1 - t0) * 1e3), ms[(m, "device")].append((t2 - t1) * 1e3)
            elif m == 0:
                back = (ctypes.c_char * total)()
                _ok(H.hipMemcpy(ctypes.cast(back, ctypes.c_void_p), dst, total, 2))
                assert back.raw == bytes(out), "wrong bytes"
                print("    pack of the call: %s" % ctx.last_pack_stats(), flush=True)
    ctx.set_check_mode(0)
    h0 = _spread("host to host, check mode 0 (default)", ms[(0, "host")])
    h1 = _spread("host to host, check mode 1", ms[(1, "host")])
    d0 = _spread("into device memory (context in mode 0)", ms[(0, "device")])
    d1 = _spread("into device memory (context in mode 1)", ms[(1, "device")])
    print("    %.2f GiB/s into device memory against %.2f host to host (best of the modes each)"
          % (total / 2**30 / (min(d0, d1) * 1e-3), total / 2**30 / (min(h0, h1) * 1e-3)), flush=True)
    _ok(H.hipFree(dst))
    if parent_so and what == "xz":
        path = "/dev/shm/xlz_pack_bench_%d.xz" % os.getpid()
        with open(path, "wb") as f:
            f.write(data)
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_bench.py"), "--parent-child", path, parent_so, str(calls)],
                               capture_output=True, text=True, timeout=300, cwd=ROOT)
        finally:
            os.unlink(path)
        line = [l for l in r.stdout.splitlines() if l.startswith("PARENT ")]
        if r.returncode or not line:
            print("    parent library: child failed (rc %d): %s" % (r.returncode, r.stderr[-500:]), flush=True)
        else:
            w = line[0].split()
            p = _spread("parent commit's library (%s), host to host" % w[1], [float(x) for x in w[2:]])
            print("    into device memory is %s than the parent's host-to-host call (%.2f against %.2f ms)"
                  % ("faster" if min(d0, d1) < p else "NOT faster", min(d0, d1), p), flush=True)


def sevenzip_archive(folders):
    import corpus
    import sevenzip_craft as C
    distinct = []
    for i in range(64):
        p = corpus.plain("T", 9100 + i, 1 << 20)
        rec, packed = C.lzma2_folder(p, dict_byte=18)
        distinct.append((rec, packed, [p]))
    return C.archive([distinct[i % 64] for i in range(folders)], folder_crc=True), folders << 20


def main():
    args = sys.argv[1:]
    parent_so, blocks, calls, kernel = None, [1024, 4096], 7, True
    while args:
        a = args.pop(0)
        if a == "--parent-so":
            parent_so = args.pop(0)
        elif a == "--blocks":
            blocks = [int(x) for x in args.pop(0).split(",")]
        elif a == "--calls":
            calls = int(args.pop(0))
        elif a == "--no-kernel":
            kernel = False
        else:
            raise SystemExit("unknown argument " + a)
    import lzma_amd
    from lzma_amd import _native as N
    info = N.library_info()
    print("library build %s, decode kernels %s; pack kernel: a workgroup of 256 per 16 KiB tile of the destination, at most 8 workgroups per CU"
          % (info["build_id"], info["kernel_id"]), flush=True)
    # (every worker process has come and gone before this process opens the device)
    import concurrent.futures as cf
    import bench
    with cf.ProcessPoolExecutor(16) as pool:
        files = [(n, bench.xz_file(pool, n, 1 << 20)[0]) for n in blocks]
    archive, archive_total = sevenzip_archive(1024)
    H = _hip()
    ctx = lzma_amd.Context(0)
    if kernel:
        kernel_alone(ctx, H, 4096, 1 << 20, calls)
        kernel_alone(ctx, H, 65536, 1 << 16, calls)
    for n, data in files:
        print("xz file of %d CRC64 blocks of 1 MiB (%.1f MiB compressed), verify on:" % (n, len(data) / 2**20), flush=True)
        front_end(ctx, H, "xz", data, n << 20, calls, parent_so)
    print(".7z archive of 1024 LZMA2 folders of 1 MiB with folder CRCs (%.1f MiB compressed), verify on:" % (len(archive) / 2**20), flush=True)
    front_end(ctx, H, "7z", archive, archive_total, calls, None)


if __name__ == "__main__":
    main()
