"""GPU: the inflate kernel (lzma_amd/csrc/xlz_inflate_dev.hip) on the stream lists of tests/inflate_matrix.py, each list in ONE
launch of lzma_amd.inflate_batch into a buffer of 0xA5 with guard bytes between the ranges: the zlib-made corpus (long codes
by the thousand, many-block streams, 200 000-byte items), the sweep of a probe block and of LEN / NLEN across the seam of the
1024-byte input window, the stored-copy matrix, every order of three blocks, 6000 + 2000 mutations, and kinds of stream
padded so that the launch rule runs a chosen one behind a chosen one in the same LDS.  The judge is Python's zlib (inflate_edges.judge); both CPU twins
equal it on every list (tests/test_inflate_matrix_cpu.py).  Every stream is bounds-checked data: a damaged one is an error
the kernel reports, nothing here reads or writes out of range."""
import pytest
import torch   # (before libxlz.so is loaded: torch brings its own HIP runtime, which must be the one that initialises the device)

import inflate_edges as E
import inflate_matrix as M
import lzma_amd
from inflate_check import check, filled, layout

pytestmark = pytest.mark.gpu

WG_PER_CU = 16                # xlz_inflate_dev.hip: kInflateWgPerCu


def _run(ctx, specs, mode, what):
    """one inflate_batch of the whole list, compared with the judge; -> the judge's classes"""
    memo = {}
    judged = [memo.setdefault((d, c), E.judge(d, c)) for d, c, _ in specs]
    items, total = layout(specs)
    dst = filled(total)
    ctx.set_deflate_mode(mode)
    try:
        results = lzma_amd.inflate_batch(ctx, items, dst.data_ptr(), total)
    finally:
        ctx.set_deflate_mode(0)
    check(items, results, dst.cpu().numpy().tobytes(), judged, "%s, mode %d" % (what, mode))
    s = ctx.last_inflate_stats()
    bad = sum(j[0] != E.OK for j in judged)
    good_bytes = sum(len(j[1]) for j in judged if j[0] == E.OK)
    if mode == 1:
        assert s == {"device_items": len(specs), "device_bytes": good_bytes, "host_items": 0, "host_bytes": 0, "failed_items": bad,
                     "uploads": 1, "launches": 1}, what
    else:
        assert s == {"device_items": 0, "device_bytes": 0, "host_items": len(specs), "host_bytes": good_bytes, "failed_items": bad,
                     "uploads": 0, "launches": 0}, what
    return [j[0] for j in judged]


def test_the_zlib_made_corpus(ctx):
    classes = _run(ctx, M.corpus(), 1, "corpus")
    assert set(classes) == {E.OK, E.RESULT, E.EOF, E.OUT_CAP}


@pytest.mark.parametrize("mode", [1, 2], ids=["kernel", "host-threads"])
def test_the_window_seam_sweep(ctx, mode):
    _run(ctx, M.seam_sweep(), mode, "seam sweep")


@pytest.mark.parametrize("mode", [1, 2], ids=["kernel", "host-threads"])
def test_the_stored_copy_matrix(ctx, mode):
    _run(ctx, M.stored_matrix(), mode, "stored matrix")


def test_every_order_of_three_blocks(ctx):
    _run(ctx, M.block_orders(), 1, "block orders")


def test_6000_mutations_of_the_small_seeds(ctx):
    classes = _run(ctx, M.mutation_lists()[0], 1, "mutations")
    assert all(classes.count(c) >= n for c, n in ((E.OK, 1000), (E.EOF, 1000), (E.RESULT, 1000), (E.OUT_CAP, 500)))


def test_2000_mutations_of_corpus_streams(ctx):
    _run(ctx, M.mutation_lists()[1], 1, "mutations of the big pool")


def test_ordered_pairs_on_one_workgroup(ctx):
    """workgroup g takes sorted positions g, g + grid, ...: position p of the list and position p + grid share an LDS, one
    behind the other.  An empty input cannot stand in FRONT of another kind there (tests/inflate_matrix.py: EMPTY)"""
    grid = WG_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count
    if grid < 144:
        pytest.skip("fewer than 144 workgroups in a launch")
    specs = M.pairs(grid)
    assert len(specs) > grid and len(M.pairs_met(grid)) == 133
    lens = [len(d) for d, _, _ in specs]
    assert lens == sorted(lens, reverse=True)
    classes = _run(ctx, specs, 1, "pairs")
    assert set(classes) == {E.OK, E.RESULT, E.EOF, E.OUT_CAP}
