"""Measures the .bz2 batch decoder (lzma_amd.bzip2) -> profiles/device_bz2.txt.

Whole calls of bzip2.decode_many_device into device memory, verify on, the median of --repeats calls behind one warm-up:
  A  one file of --blocks level-9 blocks of text (as many one-block streams back to back: the decoder sees a block candidate
     each and settles one chain, as for one long stream)
  B  --blocks files of one level-1 block
  C  one file of one level-9 block: the lone wave
each against bz2 mode 2 (every block on host threads, uploaded) and against bz2.decompress over 16 processes, which leaves
the bytes on the host; and D, the break-even: one file of 8 .. --blocks blocks, level 9 and level 1, the same three ways --
the smallest count at which the device beats BOTH host forms, which run 16 ways.  From C's kernel times per phase come the
rates of lzma_amd/csrc/xlz_bz2_dev.h: ns per symbol of phase A, and ns per dependent load of phase C (the walk kernel's time over nblock / 64 x 2: every lane walks its
share twice over -- once to find where the segments end, once implied by the scatter -- so this is an upper bound).

    python tools/bz2_bench.py [--blocks 4096] [--repeats 5] [--out profiles/device_bz2.txt]
"""
import argparse
import bz2
import multiprocessing
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))


def _decompress_all(streams):
    return sum(len(bz2.decompress(s)) for s in streams)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "device_bz2.txt"))
    a = ap.parse_args()
    import torch
    import bz2_files as F
    import lzma_amd
    from lzma_amd import bzip2

    ctx = lzma_amd.Context(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def device_call(files, caps, mode):
        windows, total = bzip2.layout(files, caps, 16)
        dst = torch.empty((max(total, 1),), dtype=torch.uint8, device="cuda")
        bzip2.set_mode(ctx, mode)
        times = []
        for k in range(a.repeats + 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = bzip2.decode_many_device(ctx, files, dst.data_ptr(), total, windows)
            times.append(time.perf_counter() - t)
            assert all(r[0] == 0 for r in res), [r for r in res if r[0] != 0][:3]
        bzip2.set_mode(ctx, bzip2.DEVICE)
        return statistics.median(times[1:]), sum(r[1] for r in res), bzip2.last_stats(ctx)

    pool = multiprocessing.get_context("spawn").Pool(16)
    pool.map(_decompress_all, [[bz2.compress(b"x")]] * 64, chunksize=1)   # (the processes exist)

    def python_16(streams):
        groups = [streams[k::16] for k in range(16) if streams[k::16]]
        times = []
        for _ in range(a.repeats):
            t = time.perf_counter()
            pool.map(_decompress_all, groups, chunksize=1)
            times.append(time.perf_counter() - t)
        return statistics.median(times)

    def row(name, files, caps, streams):
        t1, out_bytes, s1 = device_call(files, caps, bzip2.DEVICE)
        t2, _, s2 = device_call(files, caps, bzip2.HOST_THREADS)
        t3 = python_16(streams)
        mb = out_bytes / 1e6
        say("%s: %d blocks, %.1f MB decoded" % (name, s1["chain_blocks"], mb))
        say("  device        %9.1f ms  %8.1f MB/s   rounds %d, kernels: symbols %.1f walk %.1f expand %.1f crc %.1f ms"
            % (1e3 * t1, mb / t1, s1["rounds"], s1["symbols_ms"], s1["walk_ms"], s1["expand_ms"], s1["crc_ms"]))
        say("  bz2 mode 2    %9.1f ms  %8.1f MB/s   (host threads, uploaded)" % (1e3 * t2, mb / t2))
        say("  python x16    %9.1f ms  %8.1f MB/s   (bz2.decompress over 16 processes, bytes stay on the host)" % (1e3 * t3, mb / t3))
        return t1, t2, t3, s1

    from lzma_amd import _native as N
    say("# tools/bz2_bench.py --blocks %d --repeats %d on %s; library %s" % (a.blocks, a.repeats, torch.cuda.get_device_name(0), N.lib().xlz_build_id().decode()))
    text9 = F.text(899900, 9)
    one9 = bz2.compress(text9, 9)
    n9 = bzip2.probe(one9)["candidates"]
    many9 = [one9] * max(1, a.blocks // n9)
    row("A one file of level-9 blocks", [b"".join(many9)], [len(text9) * len(many9)], many9)
    text1 = F.text(99900, 1)
    one1 = bz2.compress(text1, 1)
    files1 = [one1] * a.blocks
    row("B files of one level-1 block", files1, [len(text1)] * a.blocks, files1)
    full = bz2.compress(F.text(899000, 11), 9)
    assert bzip2.probe(full)["candidates"] == 1
    t1, t2, t3, s = row("C one file of one level-9 block (the lone wave: the host wins)", [full], [899000], [full])
    nblock = 899000   # (text: the run-length stage folds next to nothing)
    say("  rate constants from C: phase A %.0f ns per block byte (symbols are fewer than bytes: an upper bound per symbol);"
        " phase B + C + measuring %.0f ns per dependent load at nblock / 64 x 2 loads per lane"
        % (1e6 * s["symbols_ms"] / nblock, 1e6 * s["walk_ms"] / (nblock / 64 * 2)))
    # the break-even: the smallest block count at which the device's call is faster than BOTH host forms, each of which
    # runs 16 ways.  One file of n one-block streams, n rising.
    say("D break-even, ms per call (device / bz2 mode 2 / python x16) by block count")
    for label, one, size in (("level 9", one9, len(text9)), ("level 1", one1, len(text1))):
        per = bzip2.probe(one)["candidates"]
        even = None
        for n in (8, 16, 32, 64, 128, 256, 512, 1024):
            if n > a.blocks:
                break
            streams = [one] * max(1, n // per)
            td, _, _ = device_call([b"".join(streams)], [size * len(streams)], bzip2.DEVICE)
            th, _, _ = device_call([b"".join(streams)], [size * len(streams)], bzip2.HOST_THREADS)
            tp = python_16(streams)
            say("  %s x %4d: %8.1f / %8.1f / %8.1f" % (label, len(streams) * per, 1e3 * td, 1e3 * th, 1e3 * tp))
            if even is None and td < min(th, tp):
                even = len(streams) * per
        say("  %s: the device wins from %s blocks on" % (label, even if even is not None else "more than %d" % a.blocks))
    pool.close()
    pool.join()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
