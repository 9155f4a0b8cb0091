"""GPU: the inflate kernel (lzma_amd/csrc/xlz_inflate_dev.hip) through lzma_amd.inflate_batch.  The judge is Python's zlib
(tests/inflate_edges.py: judge).  All crafted edge cases run in ONE launch into a buffer of 0xA5 with guard bytes between
the ranges, destinations at the residue each case names; then a launch of so many tiny items, damaged ones among them,
that every workgroup takes three and more in turn; an item above the launch-length cap, which the host threads take; the
host-thread mode on the same list; the argument rules.  Every stream is bounds-checked data: a damaged one is an error the
kernel reports, nothing here reads or writes out of range."""
import ctypes

import pytest
import torch   # (before libxlz.so is loaded: torch brings its own HIP runtime, which must be the one that initialises the device)

import inflate_edges as E
import lzma_amd
from inflate_check import FILL, check as _check, filled as _filled, layout as _layout
from lzma_amd import _native as N

pytestmark = pytest.mark.gpu

WG_PER_CU = 16                # xlz_inflate_dev.hip: kInflateWgPerCu
MAX_DEVICE_LEN = 3_600_000    # xlz_inflate_dev.h: kMaxDeviceLen


@pytest.fixture(scope="module")
def edge_judged():
    """per case: the judge's (class, bytes, input used) -- computed once, never changed"""
    return [E.judge(data, cap) for _, data, cap, _, _ in E.cases()]


@pytest.mark.parametrize("mode", [1, 2], ids=["kernel", "host-threads"])
def test_every_edge_case_in_one_launch(ctx, edge_judged, mode):
    cs = E.cases()
    items, total = _layout([(data, cap, res) for _, data, cap, _, res in cs])
    dst = _filled(total)
    ctx.set_deflate_mode(mode)
    try:
        results = lzma_amd.inflate_batch(ctx, items, dst.data_ptr(), total)
    finally:
        ctx.set_deflate_mode(0)
    _check(items, results, dst.cpu().numpy().tobytes(), edge_judged, "edges, mode %d" % mode)
    s = ctx.last_inflate_stats()
    bad = sum(c[3] != E.OK for c in cs)
    good_bytes = sum(len(j[1]) for j in edge_judged if j[0] == E.OK)
    if mode == 1:
        assert s == {"device_items": len(cs), "device_bytes": good_bytes, "host_items": 0, "host_bytes": 0, "failed_items": bad, "uploads": 1,
                     "launches": 1}
    else:
        assert s == {"device_items": 0, "device_bytes": 0, "host_items": len(cs), "host_bytes": good_bytes, "failed_items": bad, "uploads": 0,
                     "launches": 0}


def test_every_workgroup_takes_three_items_and_more(ctx):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 3 * WG_PER_CU * cus + 517
    tiny = E.tiny_items(n, 99)
    assert len(tiny) == n > 3 * WG_PER_CU * 256 and all(len(d) <= 200 for d, _ in tiny)
    memo = {}
    judged = [memo.setdefault((d, c), E.judge(d, c)) for d, c in tiny]
    kinds = [j[0] == E.OK for j in judged]
    assert 0.25 < kinds.count(False) / n < 0.45 and any(not a and b for a, b in zip(kinds, kinds[1:]))   # a good one behind a failed one
    items, total = _layout([(d, c, (5 * k) % 16) for k, (d, c) in enumerate(tiny)])
    dst = _filled(total)
    results = lzma_amd.inflate_batch(ctx, items, dst.data_ptr(), total)
    _check(items, results, dst.cpu().numpy().tobytes(), judged, "tiny items")
    s = ctx.last_inflate_stats()
    assert (s["device_items"], s["host_items"], s["uploads"], s["launches"]) == (n, 0, 1, 1)
    assert s["failed_items"] == kinds.count(False)


def test_an_item_above_the_launch_length_cap_is_the_hosts(ctx):
    """the cap is a constant of the library: an item with more ROOM than it goes to the host threads, whatever it holds"""
    cs = [c for c in E.cases() if c[0].startswith("copy/")]
    specs = [(data, cap, res) for _, data, cap, _, res in cs]
    big = E.cases()[1]
    assert big[0] == "block/stored-65535:ok"
    specs.insert(3, (big[1], MAX_DEVICE_LEN + 1, 5))
    specs.insert(9, (big[1], MAX_DEVICE_LEN, 0))
    items, total = _layout(specs)
    dst = _filled(total)
    results = lzma_amd.inflate_batch(ctx, items, dst.data_ptr(), total)
    judged = [E.judge(d, c) for d, c, _ in specs]
    _check(items, results, dst.cpu().numpy().tobytes(), judged, "above the cap")
    s = ctx.last_inflate_stats()
    assert (s["host_items"], s["host_bytes"], s["device_items"], s["uploads"], s["launches"]) == (1, 65535, len(specs) - 1, 1, 1)


def test_argument_rules(ctx):
    data = E.cases()[1][1]
    dst = _filled(70000)
    before = dst.cpu().numpy().tobytes()
    ptr = dst.data_ptr()

    def bad(items, p, cap):
        with pytest.raises(lzma_amd.LzmaError) as e:
            lzma_amd.inflate_batch(ctx, items, p, cap)
        assert e.value.status == lzma_amd.ERR_BAD_ARG

    ctx_stats = lzma_amd.inflate_batch(ctx, [(data, 0, 65535)], ptr, 70000) and ctx.last_inflate_stats()
    dst.fill_(FILL)
    bad([(data, 0, 65535)], 0, 70000)                          # no destination
    bad([(data, 4466, 65535)], ptr, 70000)                     # a range that leaves the destination
    bad([(data, 70001, 0)], ptr, 70000)
    bad([(data, 0, 100), (data, 99, 100)], ptr, 70000)         # two ranges that share a byte
    bad([(data, 0, 65535)], ptr, 70000 + (1 << 30))            # more than the allocation holds
    host = ctypes.create_string_buffer(70000)
    bad([(data, 0, 65535)], ctypes.addressof(host), 70000)     # not device memory
    L = N.lib()
    res = (N.InflateResult * 1)()
    assert L.xlz_inflate_batch(ctx._h, None, 1, ctypes.c_void_p(ptr), 70000, res) == lzma_amd.ERR_BAD_ARG
    item = (N.InflateItem * 1)()
    item[0].inp, item[0].in_len, item[0].dst_off, item[0].dst_cap = None, 5, 0, 10
    assert L.xlz_inflate_batch(ctx._h, item, 1, ctypes.c_void_p(ptr), 70000, res) == lzma_amd.ERR_BAD_ARG
    assert L.xlz_inflate_batch(ctx._h, item, 1, ctypes.c_void_p(ptr), 70000, None) == lzma_amd.ERR_BAD_ARG
    assert L.xlz_inflate_batch(ctx._h, None, 0, None, 0, None) == lzma_amd.OK   # nothing to do
    assert lzma_amd.inflate_batch(ctx, [], ptr, 70000) == []
    assert dst.cpu().numpy().tobytes() == before and ctx.last_inflate_stats() == ctx_stats
    # ranges that touch, and ranges of no room, are fine
    assert [r[0] for r in lzma_amd.inflate_batch(ctx, [(data, 0, 65535), (b"\x03\x00", 65535, 0), (b"\x03\x00", 100, 0)], ptr, 70000)] == [0, 0, 0]
