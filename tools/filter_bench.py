"""Dev tool (GPU box): what the device filters (lzma_amd/csrc/xlz_filter_dev.hip) cost, in one process.
    python tools/filter_bench.py [--parent-so build_ab/parent.so] [--blocks 1024,4096] [--calls 7] [--no-gib] [--copy-so build_ab/libfilter_copy.so] > profiles/device_filters.txt

1. The kernels alone: 4096 x 1 MiB of machine code (the bytes of the Python binary) decoded once into a device-resident
   batch, then 20 timed Batch.filter calls per filter after three warm-up calls (the filter kernels by HIP events:
   Context.last_filter_stats); the same for ONE stream of 1 GiB (stored-chunk LZMA2, random bytes).  GB/s = bytes
   filtered / time, beside a float4 copy kernel's rate over as many bytes measured in this process
   (tools/filter_copy.hip): a copy of n bytes and an in-place pass over n bytes both move 2 n bytes.  A filter applied
   again and again to its own output stays the same work (the x86 bytes stay code-like; Delta's become noise).
2. The call a user makes: .xz files of 1 MiB CRC64 blocks of machine code written with [x86, LZMA2], through
   xz_decode_into host to host with verify on, filter mode 1; beside the same plaintext written without the filter
   (the difference = the filter + the slicing a filtered call gives up; the phase times of one call of each come from a
   child process with XLZ_DEBUG=1) and beside lzma.decompress on ONE host thread (one call, the 1024-block file only).
3. No regression: the UNFILTERED file through this library and, with --parent-so, through that library (a build of the
   parent commit) in a child process.
Every GPU step is this process under the caller's time limit, or a child process with a time limit of its own."""
import ctypes
import lzma
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = {3: "Delta", 4: "x86", 5: "PowerPC", 6: "IA-64", 7: "ARM", 8: "ARM-Thumb", 9: "SPARC"}


COPY_SO = None   # --copy-so: a build of tools/filter_copy.hip made beforehand; without it one is built in a temporary directory
_COPY_LIB = []


def _copy_lib():
    if _COPY_LIB:
        return _COPY_LIB[0]
    if COPY_SO:
        L = ctypes.CDLL(os.path.abspath(COPY_SO))
    else:
        with tempfile.TemporaryDirectory() as d:
            so = os.path.join(d, "libfilter_copy.so")
            subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-shared", "-fPIC",
                                   os.path.join(ROOT, "tools", "filter_copy.hip"), "-o", so])
            L = ctypes.CDLL(so)   # (stays mapped after the directory has gone)
    _COPY_LIB.append(L)
    L.filter_copy_ms.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
    return L


def copy_rate(n_bytes):
    """median GB/s (read + write counted once each way: 2 n bytes moved, n bytes "copied") of the float4 copy kernel"""
    ms = (ctypes.c_float * 20)()
    assert _copy_lib().filter_copy_ms(n_bytes, 20, ms) == 0
    med = statistics.median(list(ms))
    print("float4 copy kernel, %d MiB                       median %8.3f ms (min %.3f, max %.3f; 20 launches)  %8.1f GB/s copied (%.1f GB/s read + written)"
          % (n_bytes >> 20, med, min(ms), max(ms), n_bytes / med / 1e6, 2 * n_bytes / med / 1e6), flush=True)
    return n_bytes / med / 1e6


def _rate(label, n_bytes, ms_list, copy_gbs):
    med = statistics.median(ms_list)
    gbs = n_bytes / med / 1e6
    print("%-48s median %8.3f ms (min %.3f, max %.3f; %d calls)  %8.1f GB/s  %5.1f %% of the copy kernel"
          % (label, med, min(ms_list), max(ms_list), len(ms_list), gbs, 100 * gbs / copy_gbs), flush=True)


def _time_filters(ctx, b, n_streams, size, label, copy_gbs, check_first):
    import lzma_amd
    for fid, prm in ((4, 0), (3, 1), (3, 4), (3, 256), (7, 0), (8, 0), (5, 0), (9, 0), (6, 0)):
        steps = [(i, fid, prm) for i in range(n_streams)]
        ms = []
        for k in range(23):
            before = b.download(0, min(size, 1 << 20)) if (k == 0 and check_first) else None
            b.filter(steps)
            if before is not None and size <= 1 << 20:
                assert b.download(0, size) == lzma_amd.filter_host(fid, prm, before), "wrong bytes"
            if k >= 3:
                ms.append(ctx.last_filter_stats()["kernel_ms"])
        name = NAMES[fid] + (" d=%d" % prm if fid == 3 else "")
        _rate("%s, %s" % (label, name), n_streams * size, ms, copy_gbs)


def prepare():
    """64 plaintexts of 1 MiB of machine code; each as an .lzma stream, as an .xz stream with [x86, LZMA2] and as one with
    [LZMA2].  The worker processes have come and gone before this process opens the device."""
    import filter_ref
    import concurrent.futures as cf
    nd, size = 64, 1 << 20
    code = filter_ref.machine_code(nd * 65536 + size, 0)
    plains = [code[i * 65536: i * 65536 + size] for i in range(nd)]
    with cf.ProcessPoolExecutor(16) as pool:
        cs = list(pool.map(_alone, plains))
        filt = list(pool.map(_xz_block, [(p, True) for p in plains]))
        plain = list(pool.map(_xz_block, [(p, False) for p in plains]))
    return plains, cs, filt, plain


def _alone(p):
    import corpus
    return corpus.compress_alone(p, preset=0)


def run_kernels(ctx, cs, with_gib):
    import lzma_amd
    nd, size = len(cs), 1 << 20
    copy_gbs = copy_rate(4096 * size)
    streams = [lzma_amd.Stream(c, out_cap=size) for c in cs]
    b = lzma_amd.Batch(ctx, [streams[i % nd] for i in range(4096)])
    b.run()
    assert all(r[0] == size and r[1] >= 0 for r in b.results())
    _time_filters(ctx, b, 4096, size, "4096 x 1 MiB", copy_gbs, True)
    b.close()
    if not with_gib:
        return
    import numpy as np
    chunks, payload = 16384, 65536   # one stream of 1 GiB in stored LZMA2 chunks
    a = np.empty((chunks, payload + 3), dtype=np.uint8)
    a[:, 3:] = np.random.default_rng(7).integers(0, 256, size=(chunks, payload), dtype=np.uint8)
    a[:, 0], a[0, 0], a[:, 1], a[:, 2] = 2, 1, 0xFF, 0xFF
    comp = a.tobytes() + b"\0"
    del a
    copy_gbs = copy_rate(chunks * payload)
    b = lzma_amd.Batch(ctx, [lzma_amd.Stream(comp, lzma_amd.FMT_LZMA2_RAW, out_cap=chunks * payload, dict_size=1 << 20)])
    b.run()
    assert b.results()[0][:2] == (chunks * payload, 0), b.results()
    _time_filters(ctx, b, 1, chunks * payload, "ONE stream of 1 GiB", copy_gbs, False)
    b.close()


def _xz_block(job):
    p, x86 = job
    l2 = {"id": lzma.FILTER_LZMA2, "preset": 0, "dict_size": 1 << 20}
    return lzma.compress(p, format=lzma.FORMAT_XZ, check=lzma.CHECK_CRC64, filters=([{"id": lzma.FILTER_X86}] if x86 else []) + [l2])


def _calls(ctx, data, total, calls):
    import lzma_amd
    out = bytearray(total)
    ms = []
    for k in range(calls + 1):
        t0 = time.perf_counter()
        n = lzma_amd.xz_decode_into(ctx, data, out, verify=True)
        dt = (time.perf_counter() - t0) * 1e3
        assert n == total
        if k:
            ms.append(dt)
    return ms, out


def _spread(label, ms):
    print("    %-44s median %8.2f ms  min %8.2f  max %8.2f  (%d calls)" % (label, statistics.median(ms), min(ms), max(ms), len(ms)), flush=True)


def _child(path, so, calls, mode):
    """child process: xlz_xz_decode of the file at `path` on the library `so` (mode >= 0: with that filter mode, phase times
    on stderr when XLZ_DEBUG is set; mode < 0: a library without filter entry points)"""
    L = ctypes.CDLL(os.path.abspath(so))
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.xlz_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    L.xlz_xz_decode.argtypes = [vp, vp, sz, vp, sz, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, ctypes.POINTER(sz)]
    L.xlz_build_id.restype = ctypes.c_char_p
    data = open(path, "rb").read()
    total = int(os.environ["XLZ_BENCH_TOTAL"])
    ctx = vp()
    assert L.xlz_ctx_create(0, ctypes.byref(ctx)) == 0
    if mode >= 0:
        L.xlz_ctx_set_filter_mode.argtypes = [vp, ctypes.c_int]
        assert L.xlz_ctx_set_filter_mode(ctx, mode) == 0
    src = ctypes.c_char_p(data)
    out = (ctypes.c_char * total)()
    ms = []
    for k in range(calls + 1):
        n, unv = ctypes.c_uint64(), sz()
        t0 = time.perf_counter()
        st = L.xlz_xz_decode(ctx, ctypes.cast(src, vp), len(data), ctypes.cast(out, vp), total, ctypes.byref(n), 1, ctypes.byref(unv))
        dt = (time.perf_counter() - t0) * 1e3
        assert st == 0 and n.value == total, (st, n.value)
        if k:
            ms.append(dt)
    print("CHILD %s %s" % (L.xlz_build_id().decode(), " ".join("%.2f" % x for x in ms)))


def _run_child(data, total, so, calls, mode, debug=False):
    env = dict(os.environ, XLZ_BENCH_TOTAL=str(total))
    if debug:
        env["XLZ_DEBUG"] = "1"
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "file.xz")
        with open(path, "wb") as f:
            f.write(data)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, so, str(calls), str(mode)], capture_output=True,
                           text=True, timeout=300, cwd=ROOT, env=env)
    line = [x for x in r.stdout.splitlines() if x.startswith("CHILD ")]
    if r.returncode or not line:
        print("    child failed (rc %d): %s" % (r.returncode, r.stderr[-500:]), flush=True)
        return None, None, ""
    w = line[0].split()
    return w[1], [float(x) for x in w[2:]], r.stderr


def user_calls(ctx, plains, filt, plain, blocks_list, calls, parent_so):
    import lzma_amd
    from lzma_amd import build
    nd = len(plains)
    for blocks in blocks_list:
        total = blocks << 20
        f_x86 = b"".join(filt[i % nd] for i in range(blocks))
        f_plain = b"".join(plain[i % nd] for i in range(blocks))
        print("xz file of %d CRC64 blocks of 1 MiB of machine code, xz_decode_into host to host, verify on (check mode 0):" % blocks, flush=True)
        ctx.set_filter_mode(1)
        ms_f, out = _calls(ctx, f_x86, total, calls)
        for i in (0, blocks // 2, blocks - 1):
            assert bytes(out[i << 20: (i + 1) << 20]) == plains[i % nd], "wrong bytes"
        print("    filter stats of one call: %s" % ctx.last_filter_stats(), flush=True)
        print("    call stats of one call:   %s" % ctx.last_call_stats(), flush=True)
        _spread("[x86, LZMA2] (%.1f MiB), filter mode 1" % (len(f_x86) / 2**20), ms_f)
        ms_p1, _ = _calls(ctx, f_plain, total, calls)
        _spread("[LZMA2] (%.1f MiB), filter mode 1" % (len(f_plain) / 2**20), ms_p1)
        ctx.set_filter_mode(0)
        ms_p0, _ = _calls(ctx, f_plain, total, calls)
        _spread("[LZMA2], filter mode 0 (default)", ms_p0)
        print("    call stats of one call:   %s" % ctx.last_call_stats(), flush=True)
        print("    filtered - unfiltered medians: %.2f ms" % (statistics.median(ms_f) - statistics.median(ms_p0)), flush=True)
        for label, data, mode in (("[x86, LZMA2]", f_x86, 1), ("[LZMA2]", f_plain, 0)):
            _, _, err = _run_child(data, total, build.SO, 1, mode, debug=True)
            lines = [x for x in err.splitlines() if x.startswith("xlz_decode_batch:")]
            print("    XLZ_DEBUG=1 phase times of one %s call (second call of a child process):" % label)
            for x in lines[len(lines) // 2:]:
                print("        " + x, flush=True)
        if parent_so:
            bid, ms, _ = _run_child(f_plain, total, parent_so, calls, -1)
            if ms:
                _spread("[LZMA2], parent commit's library (%s)" % bid, ms)
                spread = max(ms) - min(ms)
                diff = statistics.median(ms_p0) - statistics.median(ms)
                print("    this library - parent, medians: %+.2f ms; the parent's own min-max spread: %.2f ms -> %s"
                      % (diff, spread, "within it" if abs(diff) <= spread else "OUTSIDE it"), flush=True)
        if blocks <= 1024:
            t0 = time.perf_counter()
            got = lzma.decompress(f_x86)
            dt = (time.perf_counter() - t0) * 1e3
            assert len(got) == total
            print("    lzma.decompress of the [x86, LZMA2] file, ONE host thread, one call: %.0f ms" % dt, flush=True)
        else:
            print("    lzma.decompress of the [x86, LZMA2] file: not measured (one host thread: about %d times the 1024-block call)" % (blocks // 1024), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return _child(args[1], args[2], int(args[3]), int(args[4]))
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
        elif a == "--copy-so":
            global COPY_SO
            COPY_SO = args.pop(0)
        else:
            raise SystemExit("unknown argument " + a)
    import lzma_amd
    from lzma_amd import _native as N
    info = N.library_info()
    print("library build %s, decode kernels %s; filter kernels: BCJ 16 KiB per workgroup, x86 one lane per 256-byte window (two launches), "
          "Delta 16 KiB chunks in LDS (four launches)" % (info["build_id"], info["kernel_id"]), flush=True)
    plains, cs, filt, plain = prepare()
    ctx = lzma_amd.Context(0)
    run_kernels(ctx, cs, gib)
    user_calls(ctx, plains, filt, plain, blocks, calls, parent_so)


if __name__ == "__main__":
    main()
