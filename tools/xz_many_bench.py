"""Dev tool (GPU box): what a directory of one-block .xz files costs as ONE batch (xlz_xz_decode_many /
xlz_xz_decode_many_device) against the only way there was before -- a loop of xlz_xz_decode over the files --, in one process.
    python tools/xz_many_bench.py [--sets small,large,mix] [--calls 7] [--loop-files 256] > profiles/xz_many.txt

The files are written by Python's lzma, ONE block each (what xz writes by default), over bench.py's text (its
_gen_xz_block: CRC64, the fast encoder settings of the bench corpus):
    small  4096 files of 64 KiB
    large  1024 files of 1 MiB
    mix    1024 files of 100 B to 4 MiB, log-uniform, seeded
Per set, verify on, on one context:
(a) the many-call in its host form (into one host buffer laid out by xlz_xz_many_layout, align 1) and in its device form
    (into one device allocation, align 256): the C call through ctypes, the file table built once; median of `calls` with
    min - max, behind a warm-up call whose bytes are compared with the plaintext;
(b) a loop of xz_decode_into over the first --loop-files files, each into its own part of the same host buffer: ONE pass
    behind a warm-up of 8 files -- 256 files are enough to know the cost per file, which is one lone wave per call
    whatever else the loop holds --, scaled to the whole set;
(c) lzma.decompress over a pool of 16 threads (liblzma releases the interpreter lock): median of 3;
(d) the bytes uploaded (the payloads of the batch) and decoded.
Every GPU step runs in this process under the caller's time limit."""
import concurrent.futures as cf
import ctypes
import lzma
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _spread(label, ms):
    print("    %-62s median %10.3f ms  min %10.3f  max %10.3f  (%d calls)" % (label, statistics.median(ms), min(ms), max(ms), len(ms)), flush=True)
    return statistics.median(ms)


def _sizes(name):
    if name == "small":
        return [64 << 10] * 4096
    if name == "large":
        return [1 << 20] * 1024
    rnd = random.Random(20241019)
    lo, hi = 100, 4 << 20
    return [int(lo * (hi / lo) ** rnd.random()) for _ in range(1024)]


def make_set(pool, name):
    """-> (sizes, files, plaintexts); on the worker processes, which never open the device"""
    import bench
    sizes = _sizes(name)
    made = list(pool.map(bench._gen_xz_block, [(77000 + i, s) for i, s in enumerate(sizes)], chunksize=max(1, len(sizes) // 256)))
    return sizes, [c for c, _ in made], [p for _, p in made]


def one_set(ctx, name, made, calls, loop_files):
    import numpy
    import torch

    import lzma_amd
    sizes, datas, plains = made
    assert all(len(lzma_amd.xz_index(d)[0]) == 1 for d in datas[:: max(1, len(datas) // 32)])  # ONE block per file
    comp, total = sum(len(d) for d in datas), sum(sizes)
    print("%s: %d files of %s, one block each (%.1f MiB compressed, %.1f MiB decoded), verify on:"
          % (name, len(datas), "%d KiB" % (sizes[0] >> 10) if len(set(sizes)) == 1 else "%d B to %.1f MiB" % (min(sizes), max(sizes) / 2**20),
             comp / 2**20, total / 2**20), flush=True)
    whole = b"".join(plains)
    # ---- (a) the many-call, host form and device form
    host = numpy.empty(max(total, 1), dtype=numpy.uint8)
    hbuf = (ctypes.c_char * host.nbytes).from_buffer(host)
    meds = {}
    for form in ("host", "device"):
        with lzma_amd._ManyFiles(datas) as m:
            laid = m.layout(False, 1 if form == "host" else 256)
            if form == "host":
                assert laid == total
                dst, cap, fn = ctypes.cast(hbuf, ctypes.c_void_p), total, "xlz_xz_decode_many"
            else:
                dev = torch.empty(laid, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                dst, cap, fn = ctypes.c_void_p(dev.data_ptr()), laid, "xlz_xz_decode_many_device"
            ms = []
            for k in range(calls + 1):
                t0 = time.perf_counter()
                res = m.decode(fn, ctx, dst, cap, True)
                ms.append((time.perf_counter() - t0) * 1e3)
                if k:
                    continue
                assert res == [(0, s, 0) for s in sizes], "a file failed"
                got = host.tobytes() if form == "host" else dev.cpu().numpy().tobytes()
                for i in range(len(datas)):
                    off = m.arr[i].dst_off
                    assert got[off:off + sizes[i]] == plains[i], "wrong bytes: file %d" % i
                st = ctx.last_xz_many_stats()
            meds[form] = _spread("xz_decode_many, %s form (align %d)" % (form, 1 if form == "host" else 256), ms[1:])
            if form == "device":
                pk = ctx.last_pack_stats()
                print("        one batch of %d blocks, %d pack launch(es) of %d items" % (st["blocks"], pk["launches"], pk["items"]), flush=True)
                del dev
    print("        uploaded %d bytes (%.1f MiB of payload), decoded %d bytes (%.1f MiB)"
          % (st["comp_bytes"], st["comp_bytes"] / 2**20, st["decoded_bytes"], st["decoded_bytes"] / 2**20), flush=True)
    # ---- (b) the loop of single-file calls: the parent commit's code, unchanged
    k = min(loop_files, len(datas))
    offs = [0]
    for s in sizes:
        offs.append(offs[-1] + s)
    views = [memoryview(host)[offs[i]:offs[i + 1]] if sizes[i] else bytearray(1) for i in range(k)]
    for i in range(min(8, k)):
        lzma_amd.xz_decode_into(ctx, datas[i], views[i])
    t0 = time.perf_counter()
    for i in range(k):
        n = lzma_amd.xz_decode_into(ctx, datas[i], views[i])
        assert n == sizes[i]
    loop_ms = (time.perf_counter() - t0) * 1e3
    assert host[:offs[k]].tobytes() == whole[:offs[k]]
    # (scaled by files: every call is one lone wave, and the first k files are a seeded sample of the sizes)
    scaled = loop_ms * len(datas) / k
    print("    %-62s %10.3f ms for %d files (one pass), %.3f ms per file; scaled to %d files: %.0f ms"
          % ("loop of xz_decode_into, same context", loop_ms, k, loop_ms / k, len(datas), scaled), flush=True)
    # ---- (c) liblzma on 16 threads
    ms = []
    with cf.ThreadPoolExecutor(16) as tp:
        for _ in range(3):
            t0 = time.perf_counter()
            out = list(tp.map(lzma.decompress, datas, chunksize=max(1, len(datas) // 256)))
            ms.append((time.perf_counter() - t0) * 1e3)
        assert [len(o) for o in out] == sizes
    cpu = _spread("lzma.decompress over a pool of 16 threads", ms)
    print("    loop / many-call: host form %.1f x, device form %.1f x;  16 CPU threads / many-call: host form %.2f x, device form %.2f x"
          % (scaled / meds["host"], scaled / meds["device"], cpu / meds["host"], cpu / meds["device"]), flush=True)


def main():
    args = sys.argv[1:]
    sets, calls, loop_files = ["small", "large", "mix"], 7, 256
    while args:
        a = args.pop(0)
        if a == "--sets":
            sets = args.pop(0).split(",")
        elif a == "--calls":
            calls = int(args.pop(0))
        elif a == "--loop-files":
            loop_files = int(args.pop(0))
        else:
            raise SystemExit("unknown argument " + a)
    import lzma_amd
    from lzma_amd import _native as N
    info = N.library_info()
    print("library build %s, decode kernels %s" % (info["build_id"], info["kernel_id"]), flush=True)
    # (every worker process has come and gone before this process opens the device)
    with cf.ProcessPoolExecutor(16) as pool:
        made = {name: make_set(pool, name) for name in sets}
    ctx = lzma_amd.Context(0)
    for name in sets:
        one_set(ctx, name, made.pop(name), calls, loop_files)


if __name__ == "__main__":
    main()
