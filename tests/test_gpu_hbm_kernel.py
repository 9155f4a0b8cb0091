"""GPU: the HBM-model decode kernel on damaged, cut and crafted streams, with the kernel ASSERTED.

A unit whose stream announces lc + lp > 8 is decoded by xlz_decode_kernel_hbm_model (xlz_kernel.hip:
decode_units<true, false>): the model lives in a workgroup's slot of HBM scratch, only the checked C++ packet path runs,
and the launch has ONE workgroup per CU that takes unit after unit off the queue -- so a slot is used again, by a unit of
another stream with another model.  tests/test_gpu_kernels.py leaves this kernel out by construction; here every batch
but the mixed one holds nothing else (tests/hbm_streams.py).  (a) the edge corpus in one launch, (b) more units than
workgroups, in three orders, (c) the exact and the widest re-run with more streams than they have workgroups, (d) the
edge corpus among units of the LDS-model launch, in every form of the interface.  Everything is bit-exact against the
oracle on bytes, status and consumed input."""
import pytest

import hbm_streams as hs
import kernel_streams as ks
import lzma_amd
import test_gpu_kernels as tk
from lzma_amd import FMT_LZMA_ALONE, Stream

pytestmark = pytest.mark.gpu

HBM = ks.KERNEL_NAMES["hbm"]


def _assert_hbm_only(ctx, streams, what):
    """the batch's main launch is the HBM-model launch: no unit has its model in LDS"""
    name, (workgroups, _) = ks.kernel_of(ctx, streams)
    assert (name, workgroups) == (HBM, 0), (what, name, workgroups)


def _against_crafter(entries, got, what):
    bad = [name for (name, _, crafted), g in zip(entries, got) if crafted is not None and g != (crafted, 0, g[2])]
    assert bad == [], "%s: %d valid streams differ from the crafter's expected bytes, first %s" % (what, len(bad), bad[:10])


# ------------------------------------------------------------------ (a) the edge corpus in one launch ----
_EDGE = {}   # "digests": those of hbm_edge_jobs() on the HBM-model kernel


def _edge_digests(ctx, monkeypatch):
    """hbm_edge_jobs() in one HBM-model launch, device-resident and through xlz_decode_batch: the kernel asserted, the two
    result lists equal, every stream against the oracle -> digests"""
    if "digests" not in _EDGE:
        ks.unforced(monkeypatch)
        entries = hs.hbm_edge_entries()
        jobs = hs.hbm_edge_jobs()
        streams = [j[0] for j in jobs]
        _assert_hbm_only(ctx, streams, "edge corpus")
        got, _ = tk._decode(ctx, streams, "batch")
        called, stats = tk._decode(ctx, streams, "call")
        assert stats["slices"] <= 1 and stats["wave_slots"] == 0, stats
        assert tk._digest(got) == tk._digest(called), "device-resident and xlz_decode_batch differ"
        tk._against_oracle(jobs, got, "HBM-model kernel, batch")
        tk._against_oracle(jobs, called, "HBM-model kernel, call")
        _against_crafter(entries, got, "HBM-model kernel")
        _EDGE["digests"] = tk._digest(got)
    return _EDGE["digests"]


def test_the_hbm_kernel_decodes_the_edge_streams(ctx, monkeypatch):
    """hbm_streams.hbm_edge_jobs() -- about 1400 streams: valid crafted streams of lc + lp = 9 .. 12 and pb 0 .. 4, three
    small streams cut at every length and without room, flipped bits, LZMA2 streams of several units whole and damaged,
    stale reads, walks into larger properties, relabelled and zero payloads -- in ONE launch.  First the kernel: the
    HBM-model one and no LDS-model workgroup; then device-resident Batch = xlz_decode_batch = the oracle."""
    _edge_digests(ctx, monkeypatch)


@pytest.mark.parametrize("kernel", tk.KERNELS)
def test_the_forcing_variables_do_not_reach_the_hbm_launch(ctx, monkeypatch, kernel):
    """XLZ_NO_COMPACT and XLZ_BRANCHY choose among the three LDS-model kernels: with each of them set the edge corpus still
    names the HBM-model kernel and gives the same results"""
    want = _edge_digests(ctx, monkeypatch)
    ks.forced(monkeypatch, kernel)
    streams = [j[0] for j in hs.hbm_edge_jobs()]
    _assert_hbm_only(ctx, streams, "forced " + kernel)
    got, _ = tk._decode(ctx, streams, "batch")
    assert tk._digest(got) == want, "forced %s changes the HBM-model launch's results" % kernel


# ------------------------------------------------------------------ (b) more units than workgroups ----
def test_more_units_than_workgroups_reuse_the_model_slots(ctx, monkeypatch):
    """2 CUs + 37 tiny units on CUs workgroups: every workgroup's model slot is used again, by a unit of another stream --
    a model of lc + lp = 9 where one of 12 was, an LZMA2 unit that is not its stream's first (no reset of the model at the
    unit's start: its first chunk must bring one).  Every stream against the oracle; then the same streams in reversed
    order and rotated by CUs / 2 + 1 -- other units meet in a slot -- and a second run() of each batch: every stream's
    result stays what it was."""
    ks.unforced(monkeypatch)
    cus = ks.cus(ctx)
    n_units = 2 * cus + 37
    entries = hs.hbm_many_entries(n_units)
    jobs = [e[1] for e in entries]
    n = len(jobs)
    assert jobs == hs.hbm_many_jobs(n_units)
    rot = cus // 2 + 1
    orders = {"as built": list(range(n)), "reversed": list(range(n))[::-1], "rotated": [(i + rot) % n for i in range(n)]}
    first = None
    for what, order in orders.items():
        streams = [jobs[i][0] for i in order]
        b = lzma_amd.Batch(ctx, streams)
        try:
            assert (b.kernel_name(), b.launch_info()[0]) == (HBM, 0), what
            runs = []
            for _ in range(2):
                b.run()
                runs.append(tk._batch_results(b))
                assert b.stats()[2] == n_units, (what, b.stats(), n_units)
        finally:
            b.close()
        assert runs[0] == runs[1], "%s: the second run() differs from the first" % what
        got = [None] * n
        for k, i in enumerate(order):
            got[i] = runs[0][k]
        if first is None:
            first = got
            tk._against_oracle(jobs, got, "%d tiny units on %d workgroups" % (n_units, cus))
            _against_crafter(entries, got, "tiny units")
        else:
            bad = [i for i in range(n) if got[i] != first[i]]
            assert bad == [], "%s: %d streams' results depend on the order, first %s" % (what, len(bad), [entries[i][0] for i in bad[:10]])


# ------------------------------------------------------------------ (c) the re-runs past their grids ----
def test_exact_and_widest_reruns_take_more_streams_than_workgroups(ctx, monkeypatch):
    """40 stale-read streams, 24 damaged multi-unit streams (the exact re-run with big = true, whose slots are the main
    launch's) and the 40 streams that walk into larger properties, in one batch: HBM-model kernel, both forms against the
    oracle, the valid streams against the crafter's own bytes too.  The stale-read streams bring lc + lp = 12 into that
    batch, so its units decode the hidden chunks where they stand; the 40 walking streams ALONE are a launch of
    lc + lp = 9 whose units all stop in front of the hidden chunk (AUX_GROW): the widest re-run, entered from an
    HBM-model launch, with more streams than its 32 workgroups.  And the exact re-run has min(streams, CUs) workgroups:
    CUs + 37 tiny streams of two units whose first unit falls short of its headers use its slots again."""
    ks.unforced(monkeypatch)
    cus = ks.cus(ctx)
    for what, entries in (("re-runs", hs.rerun_entries()), ("walks alone", hs.walk_entries()),
                          ("short first units", hs.hbm_redo_entries(cus + 37))):
        jobs = [e[1] for e in entries]
        streams = [j[0] for j in jobs]
        _assert_hbm_only(ctx, streams, what)
        for form in tk.FORMS[:2]:
            got, _ = tk._decode(ctx, streams, form)
            tk._against_oracle(jobs, got, "%s, %s" % (what, form))
            _against_crafter(entries, got, "%s, %s" % (what, form))
    assert len(hs.walk_entries()) == 40 > 32 and all(e[2] is not None for e in hs.walk_entries())
    assert max(max(lc + lp for lc, lp, _ in ks.visible_props(e[1][0])) for e in hs.walk_entries()) == 9


# ------------------------------------------------------------------ (d) among units of the LDS-model launch ----
@pytest.mark.parametrize("form", tk.FORMS)
def test_the_edge_streams_among_lds_units(ctx, monkeypatch, form):
    """hbm_edge_jobs(), and the six cuts of its LZMA2 stream that are too short to show a properties byte, scattered
    evenly among 300 valid 8 KiB streams of pb <= 2: the main launch is the compact kernel over the LDS units alone, the
    large-model units run in their launch behind it (in the sliced form: behind the slices, fetched again at the end).
    Edge streams against the oracle, fillers by SHA-256, status, length and consumed input; the large-model streams'
    results are those of the HBM-only launch."""
    want = _edge_digests(ctx, monkeypatch)
    ks.unforced(monkeypatch)
    edges, shorts = hs.hbm_edge_jobs(), hs.short_cut_jobs()
    scattered = edges + shorts
    comp, _ = tk._fillers()
    n_fill = 300
    n = len(scattered) + n_fill
    at = {k * n // len(scattered): j for k, j in enumerate(scattered)}
    assert len(at) == len(scattered)
    fill, streams, shared = {}, [], {}
    for i in range(n):
        if i in at:
            streams.append(at[i][0])
        else:
            fill[i] = len(fill) % len(comp)
            if fill[i] not in shared:
                shared[fill[i]] = Stream(comp[fill[i]], FMT_LZMA_ALONE, out_cap=8192)
            streams.append(shared[fill[i]])
    lds_units = n_fill + sum(ks.lds_units(j[0]) for j in shorts)
    assert len(fill) == n_fill and all(ks.lds_units(j[0]) == 0 for j in edges)
    name, (workgroups, _) = ks.kernel_of(ctx, streams)
    assert (name, workgroups) == (ks.KERNEL_NAMES["compact"], lds_units), (name, workgroups)
    got, stats = tk._decode(ctx, streams, form)
    if form == "sliced":
        reached = sum(1 for name, _, _ in hs.hbm_edge_entries() if name not in hs.HOST_SETTLED)
        assert stats["slices"] == 6 and stats["refetched"] >= reached, (stats, reached)
    if stats is not None:
        assert stats["wave_slots"] == lds_units, (stats, lds_units)
    tk._check_scattered(at, fill, lambda i: got[i], "mixed, " + form)
    where = sorted(at)[:len(edges)]     # (positions grow with the corpus's order, the short cuts come last)
    assert all(at[p] is j for p, j in zip(where, edges))
    assert tk._digest([got[p] for p in where]) == want, "the large-model streams' results differ from those of the HBM-only launch"
