"""Dev tool (GPU box): what the BCJ2 merge (lzma_amd/csrc/xlz_bcj2_dev.hip) costs.
    python tools/bcj2_bench.py [--items 4096] [--big 64] [--folders 1024] [--calls 7] [--copy-so build_ab/libfilter_copy.so] > profiles/device_bcj2.txt

The question: WHAT SHARE OF A FOLDER'S DECODE TIME IS ITS MERGE.
1. The kernel alone, in one child process: `--items` BCJ2 items of 1 MiB of machine code (the bytes of the Python binary,
   64 distinct plaintexts) whose main / call / jump streams are streams of ONE device-resident batch.  The batch is decoded
   once (xlz_batch_last_kernel_ms: the decode launch that produced the items' streams), then Batch.bcj2 runs 3 + 20 times
   (the merge kernel by HIP events: Context.last_bcj2_stats); median, min-max.  The same for `--big` items of 16 MiB.
   Beside them the float4 copy kernel of tools/filter_copy.hip over as many bytes, in the same process.  The wave rate
   (bytes of one item / kernel time of a launch in which every item has a wave slot of its own) is what replaces the
   estimate xlzbcj2::kWaveBytesPerS behind the launch-length cap.
2. The call a user makes, in a second child process: sevenzip_decode of an archive of `--folders` folders of 1 MiB as BCJ2
   (four coders, LZMA) in bcj2 mode 1 and mode 2, and of the same plaintext as [x86, LZMA] chain folders in filter mode 1;
   `--calls` calls each, alternating, median and min-max, bytes compared once.
Every GPU step is a child process with a time limit of its own; the parent never opens the device."""
import concurrent.futures as cf
import ctypes
import os
import pickle
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

MIB = 1 << 20


def _encode(plain):
    """one plaintext -> its four BCJ2 streams, main / call / jump also as .lzma streams (worker process, no device)"""
    import bcj2_ref
    import corpus
    main, call, jump, rc = bcj2_ref.encode(plain)
    return {"n": len(plain), "lens": (len(main), len(call), len(jump)), "rc": rc,
            "comp": [corpus.compress_alone(x, preset=0) for x in (main, call, jump)]}


def _folder(job):
    import lzma
    import sevenzip_bcj2
    import sevenzip_chains
    plain, bcj2 = job
    if bcj2:
        f = sevenzip_bcj2.bcj2_folder([plain], 4, False, "libarchive")
        f.pop("streams")
        return f
    rec, packed, nc = sevenzip_chains.chain_folder(plain, [{"id": lzma.FILTER_X86}], lzma_first=True)
    return sevenzip_bcj2.plain_folder(rec, packed, [plain], nc)


def prepare(n_big):
    import filter_ref
    code = filter_ref.machine_code(64 * 65536 + 16 * MIB + MIB, 0)
    small = [code[i * 65536: i * 65536 + MIB] for i in range(64)]
    big = [code[i * 65536: i * 65536 + 16 * MIB] for i in range(min(4, n_big))]
    with cf.ProcessPoolExecutor(16) as pool:
        enc_small = list(pool.map(_encode, small))
        enc_big = list(pool.map(_encode, big))
        f_bcj2 = list(pool.map(_folder, [(p, True) for p in small]))
        f_x86 = list(pool.map(_folder, [(p, False) for p in small]))
    return small, big, enc_small, enc_big, f_bcj2, f_x86


def _line(label, n_bytes, ms):
    med = statistics.median(ms)
    print("%-44s median %9.3f ms (min %.3f, max %.3f; %d launches)  %9.1f GB/s" % (label, med, min(ms), max(ms), len(ms), n_bytes / med / 1e6),
          flush=True)
    return med


def child_kernel(path):
    import torch
    import filter_bench
    import lzma_amd
    job = pickle.load(open(path, "rb"))
    filter_bench.COPY_SO = job["copy_so"]
    ctx = lzma_amd.Context(0)
    for label, encs, plains, count in (("1 MiB", job["enc_small"], job["small"], job["items"]), ("16 MiB", job["enc_big"], job["big"], job["big_items"])):
        if not count or not encs:
            continue
        size = encs[0]["n"]
        streams, items = [], []
        for q in range(count):
            e = encs[q % len(encs)]
            idx = []
            for j in range(3):
                idx.append(len(streams))
                streams.append(lzma_amd.Stream(e["comp"][j], out_cap=e["lens"][j]))
            items.append((idx[0], idx[1], idx[2], e["rc"], size, q * size))
        b = lzma_amd.Batch(ctx, streams)
        b.run()
        assert all(r[1] >= 0 for r in b.results())
        decode_ms = b.kernel_ms()
        dst = torch.empty(count * size, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ms = []
        for k in range(23):
            res = b.bcj2(items, dst.data_ptr(), count * size)
            assert all(st == 0 for st, _ in res)
            s = ctx.last_bcj2_stats()
            assert s["device_items"] == count and s["launches"] == 1
            if k >= 3:
                ms.append(s["kernel_ms"])
        for q in (0, count // 2, count - 1):
            assert dst[q * size:(q + 1) * size].cpu().numpy().tobytes() == plains[q % len(plains)], "wrong bytes"
        print("%d BCJ2 items of %s of machine code (main %d, call %d, jump %d, rc %d bytes each):" % ((count, label) + encs[0]["lens"] + (len(encs[0]["rc"]),)))
        med = _line("    merge kernel", count * size, ms)
        print("    decode launch that produced their streams: %9.3f ms -> the merge is %.2f %% of decode + merge" % (decode_ms, 100 * med / (decode_ms + med)))
        slots = 256 * 16  # one-wave workgroups the launch keeps resident at most (xlz_bcj2_dev.hip: kBcj2WgPerCu x CUs)
        rounds = (count + slots - 1) // slots
        print("    one wave: %.1f MB/s of output (%d round(s) of at most %d resident waves)" % (size * rounds / med / 1e3, rounds, slots), flush=True)
        filter_bench.copy_rate(count * size)
        b.close()
        del dst


def child_calls(path):
    import lzma_amd
    import sevenzip_bcj2
    job = pickle.load(open(path, "rb"))
    nf, calls = job["folders"], job["calls"]
    fb, fx, small = job["f_bcj2"], job["f_x86"], job["small"]
    a_bcj2 = sevenzip_bcj2.archive([fb[i % len(fb)] for i in range(nf)])
    a_x86 = sevenzip_bcj2.archive([fx[i % len(fx)] for i in range(nf)])
    ctx = lzma_amd.Context(0)
    legs = [("BCJ2, bcj2 mode 1 (merge kernel)", a_bcj2, 0, 1), ("BCJ2, bcj2 mode 2 (host threads)", a_bcj2, 0, 2),
            ("[x86, LZMA] chain, filter mode 1", a_x86, 1, 0)]
    times = {name: [] for name, _, _, _ in legs}
    for k in range(calls + 1):
        for name, arch, fmode, bmode in legs:
            ctx.set_filter_mode(fmode)
            ctx.set_bcj2_mode(bmode)
            t0 = time.perf_counter()
            out = lzma_amd.sevenzip_decode(ctx, arch, verify=True)
            dt = (time.perf_counter() - t0) * 1e3
            if k == 0:
                assert len(out) == nf * MIB and out[:MIB] == small[0] and out[-MIB:] == small[(nf - 1) % len(small)], "wrong bytes"
                if bmode:
                    print("    %s: %s" % (name, ctx.last_bcj2_stats()), flush=True)
            else:
                times[name].append(dt)
    print("sevenzip_decode of %d folders of 1 MiB of machine code, host to host, verify on; %d alternating calls:" % (nf, calls))
    for name, arch, _, _ in legs:
        ms = times[name]
        print("    %-40s (%.1f MiB) median %8.2f ms  min %8.2f  max %8.2f" % (name, len(arch) / 2**20, statistics.median(ms), min(ms), max(ms)), flush=True)


def _run(which, job, limit):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "job.pickle")
        with open(path, "wb") as f:
            pickle.dump(job, f)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), which, path], capture_output=True, text=True, timeout=limit, cwd=ROOT)
    sys.stdout.write(r.stdout)
    if r.returncode:
        print("%s failed (rc %d): %s" % (which, r.returncode, r.stderr[-800:]), flush=True)
    return r.returncode == 0


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child-kernel":
        return child_kernel(args[1])
    if args and args[0] == "--child-calls":
        return child_calls(args[1])
    opt = {"--items": 4096, "--big": 64, "--folders": 1024, "--calls": 7, "--copy-so": None}
    while args:
        a = args.pop(0)
        if a not in opt:
            raise SystemExit("unknown argument " + a)
        v = args.pop(0)
        opt[a] = v if a == "--copy-so" else int(v)
    from lzma_amd import _native as N
    info = N.library_info()
    print("library build %s, decode kernels %s; merge kernel: one 64-lane workgroup per item, windows of 1024 main bytes" % (info["build_id"], info["kernel_id"]),
          flush=True)
    small, big, enc_small, enc_big, f_bcj2, f_x86 = prepare(opt["--big"])
    ok = _run("--child-kernel", {"copy_so": opt["--copy-so"], "enc_small": enc_small, "small": small, "items": opt["--items"], "enc_big": enc_big,
                                 "big": big, "big_items": opt["--big"]}, 420)
    # (after a child that failed nothing more is started on the device)
    if ok:
        _run("--child-calls", {"f_bcj2": f_bcj2, "f_x86": f_x86, "small": small, "folders": opt["--folders"], "calls": opt["--calls"]}, 420)


if __name__ == "__main__":
    main()
