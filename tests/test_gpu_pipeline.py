"""GPU: xlz_decode_batch's host pipeline in its three forms (xlz_decode_batch_plan: 0 one sliced piece, 1 overlapping
pieces, 2 one-round pieces of long streams), every stream against the oracle on bytes, status and consumed input.

The host side decides which bytes of a sliced call reach the caller: behind launch k it packs the pieces the launch
finished, clamps each to what its unit had produced by then (the unit results of launch k) and fetches again the streams
that fell short of a bound.  Results read after launch k + 1 has run make a short unit look finished: its bytes are never
fetched again.  A library built with -DXLZ_DEV_KNOBS reads them that late every time (XLZ_DEV_LATE_RESULTS=1)."""
import json
import os
import random
import subprocess
import sys

import pytest

import corpus
import lzma_amd
import pipeline_streams as ps
from lzma_amd import FMT_LZMA_ALONE
from lzma_amd import _native as N

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KERNEL_ID = "6dd215c46ed5"
HOST_RING_CHUNK = 32 << 20  # HostPipe::kRingBytes (lzma_amd/csrc/xlz_host.hip)


@pytest.fixture(scope="module")
def knob_so(tmp_path_factory):
    """the library with the test knobs compiled in (-DXLZ_DEV_KNOBS), built apart from the shipped one"""
    from lzma_amd import build
    return build.build(extra_flags=["-DXLZ_DEV_KNOBS"], out=str(tmp_path_factory.mktemp("knobs") / "libxlz_knobs.so"))


def _child(so, late):
    """the mixed-kind set in one call sliced five ways, in a fresh process on library `so` -> its JSON line"""
    env = dict(os.environ, XLZ_SO=so)
    env.pop("XLZ_DEV_LATE_RESULTS", None)
    if late:
        env["XLZ_DEV_LATE_RESULTS"] = "1"
    r = subprocess.run([sys.executable, "-s", os.path.join(HERE, "pipeline_streams.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "child (late=%s) exited %d:\n%s" % (late, r.returncode, r.stderr[-4000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_sliced_download_uses_each_launchs_own_results(knob_so):
    """Every launch of a sliced call writes the same device array of unit results.  The download of launch k's pieces must
    use launch k's results: the scatter clamps a piece to them, and a unit that fell short of launch k's bound (its head
    ran out of input) is fetched again only if they say so.  With the results read as late as possible -- after launch
    k + 1 -- the call still gives the oracle's result on every stream and fetches the same streams again."""
    plain = _child(knob_so, late=False)
    late = _child(knob_so, late=True)
    for run in (plain, late):
        assert run["kernel_id"] == KERNEL_ID
        assert run["stats"]["slices"] == 6 and run["stats"]["sub_batches"] == 1, run["stats"]
        assert run["bad"] == [], "streams that differ from the oracle: %s" % run["bad"][:20]
    assert plain["stats"]["refetched"] >= ps.MIXED_REFETCHED_AT_LEAST, plain["stats"]
    assert late["stats"]["refetched"] == plain["stats"]["refetched"], (plain["stats"], late["stats"])


def _specials(rnd, cap, seed):
    """streams of the kinds that take the pipeline's side paths, each for an output slot of `cap` bytes -> [(Stream, want)]:
    LZMA2 of several units, of stored chunks, crafted LZMA2 that reads behind a dictionary reset (collect()'s exact
    re-run), a model beyond LDS (its own HBM launch), a flipped byte, a cut stream, an empty one, one without room"""
    import lzma_craft
    third = cap // 3
    multi = corpus.lzma2_concat([corpus.plain("TMZ"[j], seed + j, third) for j in range(2)]
                                + [corpus.plain("T", seed + 2, cap - 2 * third)], preset=0)
    stored = corpus.lzma2_concat([corpus.plain("R", seed + 3, cap // 2), corpus.plain("Z", seed + 4, cap - cap // 2)], preset=0)
    reset, _ = lzma_craft.random_lzma2_stream(rnd, dict_size=4096)
    big, _ = lzma_craft.random_lzma2_stream(rnd, dict_size=4096, props=ps.BEYOND_LDS[-3:])
    good = corpus.compress_alone(corpus.plain("M", seed + 5, cap), preset=0)
    flip = bytearray(good)
    flip[13 + (len(good) - 13) * rnd.randrange(1, 9) // 10] ^= 1 << rnd.randrange(8)
    cut = good[: 13 + (len(good) - 13) * rnd.randrange(1, 9) // 10]
    more = corpus.compress_alone(corpus.plain("T", seed + 6, cap + cap // 3), preset=0)
    return [ps.raw2_job(multi, cap), ps.raw2_job(stored, cap), ps.raw2_job(reset, cap, 4096), ps.raw2_job(big, cap, 4096),
            ps.alone_job(bytes(flip), cap), ps.alone_job(cut, cap), ps.alone_job(b"", cap), ps.alone_job(more, cap)]


def test_overlapping_pieces_with_every_stream_kind(ctx):
    """Mode 1: 16 384 streams of 32-128 KiB (48 distinct plaintexts) in pieces whose upload, decode and download overlap,
    with a special stream -- every kind of _specials -- at the first and the last index of every piece and others inside
    the pieces.  Twice: the second call finds the pools warm."""
    nd, n = 48, 16384
    sizes = [32 << 10, 64 << 10, 96 << 10, 128 << 10]
    cs = [corpus.compress_alone(corpus.plain("TMZR"[d % 4], 93_500 + d, sizes[(d // 4) % 4]), preset=0) for d in range(nd)]
    common = [ps.alone_job(cs[d], sizes[(d // 4) % 4]) for d in range(nd)]
    jobs = [common[(i * 7) % nd] for i in range(n)]
    cuts, mode = lzma_amd.decode_batch_plan([j[0].out_cap for j in jobs])
    assert mode == 1 and len(cuts) >= 4, (cuts, mode)
    at = set()
    for a, b in zip(cuts, cuts[1:]):
        at |= {a, b - 1, a + 1, b - 2} | {a + (b - a) * q // 7 for q in range(1, 7)}
    at |= set(range(333, n, 2011))
    rnd = random.Random(6006)
    for k, i in enumerate(sorted(at)):
        jobs[i] = _specials(rnd, jobs[i][0].out_cap, 94_000 + 10 * k)[k % 8]
    assert lzma_amd.decode_batch_plan([j[0].out_cap for j in jobs]) == (cuts, mode)
    for run in range(2):
        st, out, offs, res = ps.flat_call(ctx, [j[0] for j in jobs])
        assert st == 0
        s = ctx.last_call_stats()
        assert s["sub_batches"] == len(cuts) - 1 and s["streams"] == n, s
        bad = ps.flat_mismatches(jobs, out, offs, res)
        assert bad == [], "run %d: %d streams differ from the oracle, first %s (specials at %s)" % (
            run, len(bad), bad[:10], sorted(at)[:10])
        del out


def test_one_round_pieces_of_multi_unit_lzma2_streams(ctx):
    """Mode 2: 8193 streams of 256 KiB and 300 KiB are three pieces, 4096 + 4096 + 1, each a wave round of its own that
    runs alone: LZMA1 mixed with LZMA2 streams of 2-4 units -- a piece has more units than one sliced launch holds and
    runs as it can (slices in the message: not asserted) -- and damaged streams at the pieces' edges (4095, 4096, 8191,
    8192)."""
    nd, n = 48, 8193
    caps = [256 << 10, 300 << 10]
    common = []
    for d in range(nd):
        cap = caps[d % 2]
        if d % 3:                                     # two thirds: LZMA2 of 2, 3 or 4 units
            k = 2 + d % 3
            segs = [corpus.plain("TMZR"[(d + j) % 4], 95_700 + 10 * d + j, cap // k) for j in range(k - 1)]
            segs.append(corpus.plain("T", 95_700 + 10 * d + 9, cap - (k - 1) * (cap // k)))
            common.append(ps.raw2_job(corpus.lzma2_concat(segs, preset=0), cap))
        else:
            common.append(ps.alone_job(corpus.compress_alone(corpus.plain("TMZR"[d % 4], 95_600 + d, cap), preset=0), cap))
    jobs = [common[(i * 5) % nd] for i in range(n)]
    for i in (4095, 4096, 8191, 8192):
        s, _ = jobs[i]
        c = bytearray(s.data)
        if i % 2:
            c[len(c) // 2] ^= 0x55
        else:
            del c[len(c) * 2 // 3:]
        jobs[i] = (ps.raw2_job if s.fmt != FMT_LZMA_ALONE else ps.alone_job)(bytes(c), s.out_cap)
    assert lzma_amd.decode_batch_plan([j[0].out_cap for j in jobs]) == ([0, 4096, 8192, 8193], 2)
    st, out, offs, res = ps.flat_call(ctx, [j[0] for j in jobs])
    assert st == 0
    s = ctx.last_call_stats()
    assert s["sub_batches"] == 3 and s["streams"] == n, s
    bad = ps.flat_mismatches(jobs, out, offs, res)
    assert bad == [], "%d streams differ from the oracle, first %s (slices: %d)" % (len(bad), bad[:10], s["slices"])
    assert N.library_info()["kernel_id"] == KERNEL_ID


def test_slices_that_span_several_ring_chunks(ctx):
    """Mode 0 with slices of about 100 MiB: every launch's packed pieces go through three or four 32 MiB chunks of the
    pinned download ring, so pieces straddle chunk boundaries.  The mixed-kind set spread among 1200 streams of 256 KiB,
    in three slices (the heads-first upload included), every stream against the oracle; twice."""
    mixed = ps.mixed_kind_jobs()
    fill = [ps.alone_job(corpus.compress_alone(corpus.plain("TMZR"[d % 4], 95_800 + d, 256 << 10), preset=0), 256 << 10)
            for d in range(24)]
    jobs = [fill[i % 24] for i in range(1200 + len(mixed))]
    for k, j in enumerate(mixed):
        jobs[k * len(jobs) // len(mixed)] = j
    assert lzma_amd.decode_batch_plan([j[0].out_cap for j in jobs])[1] == 0
    total = sum(j[0].out_cap for j in jobs)
    assert total // 3 > 2 * HOST_RING_CHUNK
    ctx.set_slicing(1, 1 << 20, 3)
    try:
        for run in range(2):
            st, out, offs, res = ps.flat_call(ctx, [j[0] for j in jobs])
            assert st == 0
            s = ctx.last_call_stats()
            assert s["slices"] == 3 and s["sub_batches"] == 1 and s["refetched"] >= ps.MIXED_REFETCHED_AT_LEAST, s
            bad = ps.flat_mismatches(jobs, out, offs, res)
            assert bad == [], "run %d: %d streams differ from the oracle, first %s" % (run, len(bad), bad[:10])
            del out
    finally:
        ctx.set_slicing(0, 0, 0)
