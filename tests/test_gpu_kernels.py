"""GPU: each of the three LDS-model decode kernels on damaged, cut and crafted streams, with the kernel ASSERTED.

The launch, not the caller, picks the kernel (xlz_kernel.hip: launch_decode, decode_per_cu, decode_branchy):
xlz_decode_kernel (full model layout) when some LDS-model unit announces pb > 2, xlz_decode_kernel_pb2 (compact layout)
otherwise, and xlz_decode_kernel_pb2_br (compact, branchy decisions) when the compact launch holds 24 workgroups per CU
-- one round of 20 CUs + 1 .. 24 CUs units, or at least 3.2 rounds of 24 CUs.  The batches of the other GPU tests that
carry a stream which is not a valid liblzma stream have a few hundred units: the compact select kernel.  Here the same
streams meet every kernel: forced through XLZ_NO_COMPACT / XLZ_BRANCHY (a), and inside batches that are large enough
for the library to pick the branchy kernel by itself (b); the stops that hand a stream to another launch (c) and the
layout choice (d) are checked with the launch's kernel named.  Every stream is compared with the oracle on bytes,
status and consumed input; valid fillers by SHA-256, status, length and consumed input."""
import hashlib

import numpy as np
import pytest

import corpus
import kernel_streams as ks
import lzma_amd
import lzma_craft
import lzma_pydec
import pipeline_streams as ps
from kernel_streams import cus as _cus
from lzma_amd import FMT_LZMA_ALONE, Stream

pytestmark = pytest.mark.gpu

KERNELS = ("full", "compact", "branchy")
FORMS = ("batch", "call", "sliced")


def _batch_results(b):
    """a device-resident batch that has run -> [(bytes, status, in_consumed)] (xlz_batch_results + xlz_batch_download)"""
    return [(b.download(i, n_out), st, n_in) for i, (n_out, st, n_in) in enumerate(b.results())]


def _decode(ctx, streams, form):
    """`streams` through one form of the public interface -> ([(bytes, status, in_consumed)], call stats or None)"""
    if form == "batch":
        b = lzma_amd.Batch(ctx, streams)
        try:
            b.run()
            return _batch_results(b), None
        finally:
            b.close()
    if form == "call":
        ctx.set_slicing(0, 0, 1)
    else:
        ctx.set_slicing(1, 1 << 20, 5)
    try:
        got = lzma_amd.decode_batch(ctx, streams)
        return got, ctx.last_call_stats()
    finally:
        ctx.set_slicing(0, 0, 0)


def _against_oracle(jobs, got, what):
    assert len(got) == len(jobs)
    bad = ps.mismatches(jobs, got)
    assert bad == [], "%s: %d of %d streams differ from the oracle, first %s: got %r, oracle %r" % (
        what, len(bad), len(jobs), bad[:10], tuple(x if not isinstance(x, bytes) else len(x) for x in got[bad[0]]),
        tuple(x if not isinstance(x, bytes) else len(x) for x in jobs[bad[0]][1]()))


def _digest(got):
    return [(hashlib.sha256(o).digest(), len(o), st, n_in) for o, st, n_in in got]


# ------------------------------------------------------------------ (a) the forced matrix ----
_CELLS = {}   # (kernel, form) -> digests of the results on pb2_edge_jobs(), in that order


def _cell(ctx, monkeypatch, kernel, form):
    """pb2_edge_jobs() -- for the full layout edge_jobs() too, which adds streams of pb 3 and 4 -- by `kernel` through
    `form`: the kernel asserted, then every stream against the oracle -> digests of the results on pb2_edge_jobs()"""
    if (kernel, form) in _CELLS:
        return _CELLS[(kernel, form)]
    ks.forced(monkeypatch, kernel)
    narrow, every = ks.pb2_edge_jobs(), ks.edge_jobs()
    assert every[:len(narrow)] == narrow and len(every) > len(narrow)
    runs = [("pb <= 2", narrow)] + ([("every pb", every)] if kernel == "full" else [])
    digests = []
    for what, jobs in runs:
        streams = [j[0] for j in jobs]
        name, (workgroups, lds_bytes) = ks.kernel_of(ctx, streams)
        assert name == ks.KERNEL_NAMES[kernel], (kernel, form, what, name)
        assert 0 < workgroups == sum(ks.lds_units(s) for s in streams), (workgroups, what)   # (one round: a workgroup per unit)
        got, stats = _decode(ctx, streams, form)
        if form == "sliced":     # (five shares, the last one cut in two; the streams fetched again after their slices)
            assert stats["slices"] == 6 and stats["sub_batches"] == 1 and 0 < stats["slot_occupancy"] <= 1.0, stats
            assert stats["refetched"] >= ps.MIXED_REFETCHED_AT_LEAST, stats
        elif form == "call":
            assert stats["slices"] <= 1 and stats["sub_batches"] == 1, stats
        if stats is not None:
            assert stats["wave_slots"] == workgroups, (stats, workgroups)
        _against_oracle(jobs, got, "%s kernel, %s, %s" % (kernel, form, what))
        digests.append(_digest(got[:len(narrow)]))
    assert all(d == digests[0] for d in digests)
    _CELLS[(kernel, form)] = digests[0]
    return digests[0]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_every_kernel_decodes_the_edge_streams_in_every_form(ctx, monkeypatch, kernel, form):
    """Forced matrix: full / compact / branchy kernel x device-resident Batch / xlz_decode_batch unsliced / in 5 slices,
    on kernel_streams.edge_jobs() in one launch (about 1500 streams: every damaged, cut and crafted stream of the GPU
    suite, two small streams cut at every length, output room of 0, 1 and size - 1).  The compact kernels see the
    streams that announce pb <= 2; the full kernel sees those (streams it never meets in production, where they run on
    the compact layout) and, in a second launch, all of them with streams of pb 3 and 4 among them.  First the kernel
    (xlz_batch_kernel_name in the same environment), then every stream's (bytes, status, in_consumed) against the
    oracle, then equality with every cell that ran before."""
    mine = _cell(ctx, monkeypatch, kernel, form)
    for other, theirs in _CELLS.items():
        assert theirs == mine, "results of %s differ from those of %s" % ((kernel, form), other)


def test_the_nine_cells_of_the_matrix_agree(ctx, monkeypatch):
    """The results must not depend on the kernel (xlz_kernel.hip: decode_branchy): the nine result lists are equal to each
    other (cells that have not run yet in this session run here)"""
    cells = {(k, f): _cell(ctx, monkeypatch, k, f) for k in KERNELS for f in FORMS}
    first = cells[("full", "batch")]
    assert len(cells) == 9 and len(first) == len(ks.pb2_edge_jobs())
    for key, d in cells.items():
        assert d == first, key


# ------------------------------------------------------------------ (b) the kernel the product picks by itself ----
_FILLERS = {}


def _fillers():
    """1024 valid default-parameter streams of 8 KiB -> (compressed, SHA-256 of the plaintexts)"""
    if not _FILLERS:
        _FILLERS["v"] = corpus.make_alone_batch("M", 1024, 8192, base_seed=91_000,
                                                preset={"mode": 1, "mf": 3, "nice_len": 32, "depth": 2})
    return _FILLERS["v"]


def _edges_among_fillers(n_units):
    """default_props_edge_jobs() scattered evenly among as many fillers as make `n_units` units
    -> (streams, {index: job} of the edge streams, {index: filler number} of the others)"""
    edges = ks.default_props_edge_jobs()
    comp, _ = _fillers()
    edge_units = sum(ks.lds_units(j[0]) for j in edges)
    n = len(edges) + n_units - edge_units
    assert n_units - edge_units >= len(edges), "more fillers than edge streams"
    at = {k * n // len(edges): j for k, j in enumerate(edges)}
    assert len(at) == len(edges)
    fill, streams, shared = {}, [], {}
    for i in range(n):
        if i in at:
            streams.append(at[i][0])
        else:
            fill[i] = len(fill) % len(comp)
            if fill[i] not in shared:
                shared[fill[i]] = Stream(comp[fill[i]], FMT_LZMA_ALONE, out_cap=8192)
            streams.append(shared[fill[i]])
    return streams, at, fill


def _check_scattered(at, fill, result_of, what):
    """result_of(i) -> (bytes, status, in_consumed) of stream i: edge streams against the oracle, fillers by SHA-256,
    status, length and consumed input"""
    comp, sha = _fillers()
    bad = [i for i, (_, want) in at.items() if result_of(i) != want()]
    assert bad == [], "%s: %d edge streams differ from the oracle, first %s" % (what, len(bad), sorted(bad)[:10])
    for i, f in fill.items():
        out, st, n_in = result_of(i)
        assert (st, len(out), n_in) == (0, 8192, len(comp[f])) and hashlib.sha256(out).digest() == sha[f], (what, i, st, len(out), n_in)


def _flat_result_of(out, offs, res):
    return lambda i: (out[offs[i]: offs[i] + res[i][0]].tobytes(), res[i][1], res[i][2])


def _picked_by_itself(ctx, monkeypatch, n_units, workgroups, sliced):
    ks.unforced(monkeypatch)
    streams, at, fill = _edges_among_fillers(n_units)
    b = lzma_amd.Batch(ctx, streams)
    try:
        # the kernel and its grid BEFORE anything is compared: a batch that lands on another kernel fails here
        assert b.kernel_name() == ks.KERNEL_NAMES["branchy"], (b.kernel_name(), b.launch_info(), n_units)
        assert b.launch_info()[0] == workgroups, (b.launch_info(), workgroups, n_units)
        b.run()
        res = b.results()
        assert b.stats()[2] == n_units
        _check_scattered(at, fill, lambda i: (b.download(i, res[i][0]), res[i][1], res[i][2]), "device-resident")
    finally:
        b.close()
    for form in ("call", "sliced") if sliced else ("call",):
        if form == "call":
            ctx.set_slicing(0, 0, 1)
        else:
            ctx.set_slicing(1, 1 << 20, 4)
        try:
            st, out, offs, res = ps.flat_call(ctx, streams)
            stats = ctx.last_call_stats()
        finally:
            ctx.set_slicing(0, 0, 0)
        assert st == 0
        assert stats["sub_batches"] == 1 and stats["units"] == n_units and stats["wave_slots"] == workgroups, stats
        assert stats["slices"] >= 2 if form == "sliced" else stats["slices"] <= 1, stats
        _check_scattered(at, fill, _flat_result_of(out, offs, res), "xlz_decode_batch, " + form)
        del out


def test_one_round_at_24_per_cu_picks_the_branchy_kernel_and_decodes_the_edge_streams(ctx, monkeypatch):
    """No variable set.  kernel_streams.default_props_edge_jobs() -- about 1500 damaged, cut and crafted streams, 1750
    units -- scattered among valid 8 KiB streams to a batch of 24 CUs - CUs / 2 - 16 units (6000 on 256 CUs): one round
    at 24 workgroups per CU, which the launch runs on the branchy kernel.  Asserted: the kernel and a workgroup per unit;
    then device-resident, through xlz_decode_batch, and through xlz_decode_batch in slices (the branchy kernel's save /
    resume of every unit): edge streams against the oracle, fillers by SHA-256, status, length and consumed input."""
    cus = _cus(ctx)
    n_units = ks.BRANCHY_PER_CU * cus - cus // 2 - 16
    assert 20 * cus < n_units <= ks.BRANCHY_PER_CU * cus
    _picked_by_itself(ctx, monkeypatch, n_units, n_units, sliced=True)


def test_many_rounds_at_24_per_cu_pick_the_branchy_kernel_and_decode_the_edge_streams(ctx, monkeypatch):
    """No variable set.  The same edge streams among valid 8 KiB streams to 96 CUs units (24 576 on 256 CUs): four rounds
    of 24 per CU, more than the 3.2 from which on a launch takes 24 -- the shape of the headline benchmark.  Asserted: the
    branchy kernel on 24 CUs workgroups; then device-resident and through xlz_decode_batch."""
    cus = _cus(ctx)
    n_units = 4 * ks.BRANCHY_PER_CU * cus
    assert n_units * 5 >= 16 * ks.BRANCHY_PER_CU * cus
    _picked_by_itself(ctx, monkeypatch, n_units, ks.BRANCHY_PER_CU * cus, sliced=False)


# ------------------------------------------------------------------ (c) the stops that send a stream to another launch ----
def _neighbours():
    return [ps.alone_job(corpus.compress_alone(corpus.plain("TMZR"[i % 4], 4400 + i, 20_000 + 999 * i), preset=0), 20_000 + 999 * i)
            for i in range(8)]


@pytest.mark.parametrize("kernel", ["compact", "branchy"])
@pytest.mark.parametrize("which", ["walks_into_larger_pb", "walks_into_larger_props"])
def test_a_stream_that_walks_into_larger_properties_stops_a_compact_launch(ctx, monkeypatch, which, kernel):
    """A chunk hidden from the host's scan renews the model with pb 4 (a larger LAYOUT than the compact launch has) or with
    lc 8 / lp 4 (a larger MODEL): the unit stops in front of it (AUX_GROW) and the stream is decoded again by the widest
    launch.  The launch that has to stop IS a compact-layout launch -- the select kernel as the library picks it for nine
    streams, and the branchy one forced --, the result is the oracle's and the Python restatement's, and the ordinary
    streams around it are not disturbed."""
    import test_crafted_streams as tc
    blob, ds, cap = getattr(tc, which)()
    if kernel == "compact":
        ks.unforced(monkeypatch)
    else:
        ks.forced(monkeypatch, kernel)
    jobs = _neighbours()
    jobs.insert(3, ps.raw2_job(blob, cap, ds))
    streams = [j[0] for j in jobs]
    name, (workgroups, _) = ks.kernel_of(ctx, streams)
    assert name == ks.KERNEL_NAMES[kernel] and workgroups == 9, (name, workgroups)
    want = jobs[3][1]()
    assert want[1] == 0 and lzma_pydec.lzma2_raw(blob, ds) == want
    for form in FORMS[:2]:
        got, _ = _decode(ctx, streams, form)
        _against_oracle(jobs, got, "%s, %s kernel, %s" % (which, kernel, form))


@pytest.mark.parametrize("kernel", KERNELS)
def test_stale_reads_are_settled_by_an_exact_launch_of_the_same_kernel(ctx, monkeypatch, kernel):
    """40 crafted LZMA2 streams whose copies read behind dictionary resets: the ordinary launch flags them (AUX_STALE),
    collect() decodes each again as one unit of an exact launch, which runs the same kernel (forced here: with
    XLZ_BRANCHY=1 the re-run of a handful of units is branchy too).  Against the oracle and the Python restatement."""
    ks.forced(monkeypatch, kernel)
    jobs = ks.stale_read_jobs()
    streams = [j[0] for j in jobs]
    assert len(jobs) == 40 and ks.kernel_of(ctx, streams)[0] == ks.KERNEL_NAMES[kernel]
    # (the streams do read stale bytes: a decoder that finds zeros behind a reset gives other bytes for most of them)
    for s, want in jobs:
        assert lzma_pydec.lzma2_raw(s.data, s.dict_size) == want()
    for form in FORMS:
        got, _ = _decode(ctx, streams, form)
        _against_oracle(jobs, got, "stale reads, %s kernel, %s" % (kernel, form))


# ------------------------------------------------------------------ (d) the layout choice ----
def test_one_stream_of_pb_3_moves_the_launch_to_the_full_layout(ctx, monkeypatch):
    """No variable set.  32 streams of pb <= 2 alone run on the compact layout; with one stream of pb 3 among them the
    launch uses the full layout; a stream of lc + lp = 9 alone has no LDS-model launch at all.  The 32 streams' results
    are the same in both launches, and everything equals the oracle."""
    ks.unforced(monkeypatch)
    rnd = np.random.default_rng(4545)
    jobs = []
    for i, (lc, lp, pb) in enumerate([(3, 0, 2), (0, 0, 0), (1, 1, 1), (0, 2, 0), (4, 0, 0), (2, 2, 2), (0, 4, 1), (3, 1, 2)] * 4):
        p = corpus.plain("TMZR"[i % 4], 4500 + i, 12_000 + 701 * i)
        c = corpus.compress_alone(p, dict_size=1 << 16, lc=lc, lp=lp, pb=pb, preset=0, known_size=(i % 3 == 0))
        if i % 8 == 5:
            c = c[: len(c) * 2 // 3]
        elif i % 8 == 6:
            c = bytearray(c)
            c[13 + int(rnd.integers(20, len(c) - 13))] ^= 0x08
            c = bytes(c)
        jobs.append(ps.alone_job(c, len(p) if i % 8 != 7 else len(p) // 2))
    p3 = corpus.plain("T", 4599, 25_000)
    wide = ps.alone_job(corpus.compress_alone(p3, lc=3, lp=0, pb=3, preset=0), len(p3))
    c9, want9 = lzma_craft.long_lzma1_stream(8, 1, 0, total=60_000, seed=9)
    big = ps.alone_job(c9, len(want9))
    assert len(jobs) == 32
    results = {}
    for what, js, name, workgroups in (("32 of pb <= 2", jobs, "compact", 32), ("with one of pb 3", jobs[:16] + [wide] + jobs[16:], "full", 33),
                                       ("lc + lp = 9 alone", [big], "hbm", 0)):
        streams = [j[0] for j in js]
        got_name, (wg, _) = ks.kernel_of(ctx, streams)
        assert (got_name, wg) == (ks.KERNEL_NAMES[name], workgroups), what
        for form in FORMS[:2]:
            got, _ = _decode(ctx, streams, form)
            _against_oracle(js, got, what + ", " + form)
            results[(what, form)] = got
    assert big[1]() == (want9, 0, len(c9))
    for form in FORMS[:2]:
        mixed = results[("with one of pb 3", form)]
        assert mixed[:16] + mixed[17:] == results[("32 of pb <= 2", form)], form
