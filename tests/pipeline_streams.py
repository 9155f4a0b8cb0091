"""Stream sets of the batch pipeline's GPU tests (tests/test_gpu_shapes.py, tests/test_gpu_pipeline.py), and the child
process of tests/test_gpu_pipeline.py's run of a library built with -DXLZ_DEV_KNOBS.  A plain module, not a conftest.

A job is (Stream, want): want() is the oracle's (output bytes, status, in_consumed) for that stream, computed once."""
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import corpus  # noqa: E402
import lzma_craft  # noqa: E402
import oracle  # noqa: E402
from lzma_amd import FMT_LZMA2_RAW, FMT_LZMA_ALONE, Stream  # noqa: E402


class Want:
    """the oracle's result of one stream, computed on the first call (streams repeated in a corpus share one)"""

    def __init__(self, fn, *args):
        self.fn, self.args, self.v = fn, args, None

    def __call__(self):
        if self.v is None:
            self.v = self.fn(*self.args)
        return self.v


def alone_job(c, cap):
    return Stream(c, FMT_LZMA_ALONE, out_cap=cap), Want(oracle.lzma1_alone, c, cap)


def raw2_job(c, cap, dict_size=65536):
    return Stream(c, FMT_LZMA2_RAW, out_cap=cap, dict_size=dict_size), Want(oracle.lzma2_raw, c, dict_size, cap)


# models beyond LDS (lc + lp = 9 .. 12) among the crafted streams' properties: their own launch behind the slices
BEYOND_LDS = lzma_craft.SMALL_PROPS + [(8, 4, 2), (6, 4, 0), (8, 1, 0)]


# streams of mixed_kind_jobs() that a sliced call fetches again at least: the 7 crafted streams with a chunk whose model
# is beyond LDS (lc + lp > 8) and the 6 whose heads run out in the first launch
MIXED_REFETCHED_AT_LEAST = 13


def mixed_kind_jobs():
    """Streams of every kind, for ONE call: all four plaintext families at several sizes, known sizes without end marker,
    output room that is too small, streams cut short or with a flipped byte, an empty one, tiny ones (shorter than a
    slice's 256-byte grain), LZMA2 streams of several units, of stored chunks and damaged, crafted LZMA2 streams whose
    copies read behind dictionary resets (settled by collect()'s exact re-run), crafted streams whose models do not fit
    LDS, and streams whose head compresses so badly that the first launch of a sliced call -- which starts on a share of
    every input -- falls short of its bound.  -> list of (Stream, want)"""
    rnd = random.Random(5005)
    jobs = []  # (Stream, oracle call)

    def alone(c, cap):
        jobs.append(alone_job(c, cap))

    def raw2(c, cap, dict_size=65536):
        jobs.append(raw2_job(c, cap, dict_size))

    for i in range(160):
        size = rnd.choice([300, 5_000, 70_000, 200_000, 333_333])
        p = corpus.plain("TMZR"[i % 4], 95_000 + i, size)
        c = corpus.compress_alone(p, preset=0, known_size=(i % 5 == 0))
        kind = i % 8
        if kind == 5:
            c = bytearray(c)
            c[13 + (len(c) - 13) * rnd.randrange(1, 9) // 10] ^= 1 << rnd.randrange(8)
            c = bytes(c)
        elif kind == 6:
            c = c[: 13 + (len(c) - 13) * rnd.randrange(1, 9) // 10]
        alone(c, size if kind != 7 else size * rnd.randrange(1, 9) // 10)   # kind 7: not enough room
    for i in range(6):   # an incompressible head, then long repeats: the first launch sees a share of the INPUT (the rest
        # is still being uploaded), runs out of it far in front of its output bound and pauses -- the bytes up to the bound
        # come out of a later launch, when that bound's pieces have gone out: the stream is fetched again
        p = corpus.plain("R", 95_400 + i, 60_000 + 10_000 * i) + corpus.plain("Z", 95_410 + i, 400_000)
        alone(corpus.compress_alone(p, preset=0), len(p))
    for i in range(12):                                                         # the a.lzma flavour
        p = corpus.plain("T", 95_500 + i, 60_000)
        c = corpus.alone_known_size_no_eos(p)
        if c:
            alone(c, len(p))
    alone(b"", 100)
    alone(open(os.path.join(HERE, "golden", "a.lzma"), "rb").read(), 4096)
    for i in range(24):                                                         # LZMA2: units, stored chunks, damage
        segs = [corpus.plain("TRMZ"[(i + j) % 4], 96_000 + 10 * i + j, rnd.choice([40_000, 150_000, 262_144]))
                for j in range(rnd.randrange(1, 6))]
        c = corpus.lzma2_concat(segs, preset=0)
        total = sum(len(s) for s in segs)
        if i % 4 == 1:
            c = bytearray(c)
            c[len(c) * rnd.randrange(1, 9) // 10] ^= 0x10
            c = bytes(c)
        elif i % 4 == 2:
            c = c[: len(c) * rnd.randrange(3, 9) // 10]
        raw2(c, total if i % 6 else total - 1000)
    for i in range(40):                                                         # copies behind dictionary resets
        c, want = lzma_craft.random_lzma2_stream(rnd, dict_size=4096)
        raw2(c, len(want) + 64, dict_size=4096)
    for i in range(16):                                                         # models beyond LDS: their own launch
        c, want = lzma_craft.random_lzma2_stream(rnd, dict_size=4096, props=BEYOND_LDS)   # behind the slices, fetched at the end
        raw2(c, len(want) + 64, dict_size=4096)
    return jobs


def mismatches(jobs, got):
    """indices of the streams whose (bytes, status, in_consumed) in `got` differ from the oracle's"""
    return [i for i, (_, want) in enumerate(jobs) if got[i] != want()]


def flat_call(ctx, streams):
    """xlz_decode_batch with the outputs back to back in one zeroed host array (a corpus of thousands of long streams:
    no buffer per stream, and a stream repeated in the corpus is one input buffer) -> (status, out, offsets, results)"""
    import numpy as np
    from lzma_amd import _native as N
    n = len(streams)
    offs = np.zeros(n + 1, dtype=np.int64)
    offs[1:] = np.cumsum([int(s.out_cap) for s in streams])
    out = np.zeros(int(offs[-1]) + 1, dtype=np.uint8)
    ins = {}
    descs = (N.StreamDesc * n)()
    for i, s in enumerate(streams):
        a = ins.setdefault(id(s.data), np.frombuffer(s.data, dtype=np.uint8))
        descs[i].inp = a.ctypes.data if a.size else None
        descs[i].in_len = a.size
        descs[i].out, descs[i].out_cap = out.ctypes.data + int(offs[i]), int(s.out_cap)
        descs[i].format = s.fmt
        descs[i].dict_size = s.dict_size & 0xFFFFFFFF
        descs[i].unpack_size = s.unpack_size
        descs[i].props = s.props
    res = (N.Result * n)()
    st = N.lib().xlz_decode_batch(ctx._h, descs, n, res)
    return st, out, offs, [(r.out_len, r.status, r.in_consumed) for r in res]


def flat_mismatches(jobs, out, offs, res):
    """indices of the streams of a flat_call whose bytes, status or in_consumed differ from the oracle's"""
    import numpy as np
    bad = []
    for i, (_, want) in enumerate(jobs):
        w, w_st, w_in = want()
        n_out, st, n_in = res[i]
        if (n_out, st, n_in) != (len(w), w_st, w_in) or \
                not np.array_equal(out[offs[i]: offs[i] + n_out], np.frombuffer(w, dtype=np.uint8)):
            bad.append(i)
    return bad


def _child():
    """python tests/pipeline_streams.py: the mixed-kind set in one call, sliced as tests/test_gpu_pipeline.py asks, on the
    library XLZ_SO names; prints one JSON line: the call's stats and the streams that differ from the oracle"""
    import json
    import lzma_amd
    from lzma_amd import _native as N
    ctx = lzma_amd.Context(0)
    jobs = mixed_kind_jobs()
    ctx.set_slicing(1, 1 << 20, 5)
    got = lzma_amd.decode_batch(ctx, [j[0] for j in jobs])
    st = ctx.last_call_stats()
    info = N.library_info()
    print(json.dumps({"stats": st, "bad": mismatches(jobs, got), "n": len(jobs), "kernel_id": info["kernel_id"],
                      "so": info["path"]}))


if __name__ == "__main__":
    _child()
