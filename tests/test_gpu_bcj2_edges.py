"""GPU: the BCJ2 merge kernel (lzma_amd/csrc/xlz_bcj2_dev.hip) on streams that sit on the seams of its work split -- the
crafted cases of tests/bcj2_edges.py, which tests/test_bcj2_edges_cpu.py shows to bite -- in one launch, and on so many tiny
items of mixed kinds that every workgroup merges three and more of them in turn, a good one behind a failed one.
Everything is bit-exact and the judge is tests/bcj2_ref.py.  Damaged items are data errors the merge must report: every
read is bounds-checked, nothing here reads or writes out of range."""
import lzma
import random
import time

import numpy as np
import pytest
import torch   # (before libxlz.so is loaded: torch brings its own HIP runtime, which must be the one that initialises the device)

import bcj2_edges as E
import bcj2_ref as B
import lzma_amd
from lzma_amd import FMT_LZMA2_RAW

pytestmark = pytest.mark.gpu

DICT = 1 << 16
FILL = 0xA5
GUARD = 19
WG_PER_CU = 16   # kBcj2WgPerCu of xlz_bcj2_dev.hip: the cap of one-wave workgroups per CU


def _filled(n):
    t = torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t


def _lzma2(data):
    return lzma.compress(data, format=lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA2, "dict_size": DICT, "preset": 0}])


def _lay_out(specs, from_batch):
    """specs: [(the four streams, out_len, residue)] -> (streams of the batch, items for Batch.bcj2, [(at, out_len)], size of
    the destination).  Item q with from_batch(q) takes main / call / jump from streams the same batch decodes (those of
    them that have bytes); GUARD bytes and more lie between two destinations"""
    streams, items, ranges, at = [], [], [], 0
    for q, (st4, n, res) in enumerate(specs):
        src = []
        for j in range(3):
            if st4[j] and from_batch(q):
                src.append(len(streams))
                streams.append(lzma_amd.Stream(_lzma2(st4[j]), FMT_LZMA2_RAW, out_cap=len(st4[j]), dict_size=DICT))
            else:
                src.append(st4[j])
        at += GUARD
        at += (res - at) % 16
        items.append((src[0], src[1], src[2], st4[3], n, at))
        ranges.append((at, n))
        at += n
    if not streams:
        streams.append(lzma_amd.Stream(_lzma2(b"x"), FMT_LZMA2_RAW, out_cap=1, dict_size=DICT))
    return streams, items, ranges, at + 64


def _merge_and_compare(ctx, b, items, ranges, cap, judged, names, what):
    """one Batch.bcj2 call: the reference's status per item, its bytes where that is OK, FILL in every byte no item owns"""
    dst = _filled(cap)
    t0 = time.time()
    res = b.bcj2(items, dst.data_ptr(), cap)
    st = ctx.last_bcj2_stats()
    print("%s: %d items, %.1f ms wall, stats %s" % (what, len(items), 1e3 * (time.time() - t0), st))
    got = dst.cpu().numpy()
    outside = np.ones(cap, dtype=bool)
    for q, ((at, n), (ref_st, ref)) in enumerate(zip(ranges, judged)):
        outside[at:at + n] = False
        if ref_st == B.OK:
            assert res[q] == (lzma_amd.OK, n), (what, names[q], res[q])
            if got[at:at + n].tobytes() != ref:
                k = next(i for i in range(n) if got[at + i] != ref[i])
                raise AssertionError("%s: %s (destination %d mod 16, out_len %d) differs from the reference at byte %d: got %02x, want %02x"
                                     % (what, names[q], at % 16, n, k, got[at + k], ref[k]))
        else:
            assert res[q] == (lzma_amd.ERR_RESULT, 0), (what, names[q], res[q])
    bad = np.flatnonzero(outside & (got != FILL))
    assert bad.size == 0, "%s: %d bytes outside the items' ranges were written, the first at %d" % (what, bad.size, bad[0])
    failed = sum(ref_st != B.OK for ref_st, _ in judged)
    assert st["launches"] == 1 and st["host_items"] == 0 and st["failed_items"] == failed and st["kernel_ms"] > 0, (what, st, failed)
    assert st["device_items"] == len(items) and st["device_bytes"] == sum(n for _, n in ranges), (what, st)


def test_edge_cases_in_one_launch(ctx):
    """every family of bcj2_edges.cases() in ONE Batch.bcj2 call, in seeded shuffled order, each destination at the residue
    its case names; every third item takes main / call / jump from streams the same batch decoded.  Then the same call once
    more: the item table, the uploaded streams and the results of the first call are still in the batch's scratch"""
    t_start = time.time()
    cs = E.cases()
    random.Random(9001).shuffle(cs)
    judged = [B.decode(*st4, n) for _, st4, n, _ in cs]
    t_ref = time.time()
    streams, items, ranges, cap = _lay_out([(st4, n, E.residue(name)) for name, st4, n, _ in cs], lambda q: q % 3 == 0)
    assert {at % 16 for at, _ in ranges} == set(range(16)) and all(at % 16 == E.residue(c[0]) for (at, _), c in zip(ranges, cs))
    assert all(b[0] - (a[0] + a[1]) >= GUARD for a, b in zip(ranges, ranges[1:])) and ranges[0][0] >= GUARD
    assert sum(isinstance(it[0], int) for it in items) >= len(cs) // 3 - 10 and sum(isinstance(it[1], int) for it in items) >= len(cs) // 5
    print("%d cases judged in %.1f s, %d streams of the batch prepared in %.1f s" % (len(cs), t_ref - t_start, len(streams), time.time() - t_ref))
    b = lzma_amd.Batch(ctx, streams)
    b.run()
    assert all(st >= 0 for _, st, _ in b.results())
    names = [c[0] for c in cs]
    _merge_and_compare(ctx, b, items, ranges, cap, judged, names, "edge cases")
    _merge_and_compare(ctx, b, items, ranges, cap, judged, names, "edge cases, dirty scratch")
    b.close()
    print("test_edge_cases_in_one_launch: %.1f s wall" % (time.time() - t_start))


def test_three_rounds_of_mixed_items(ctx):
    """3 x 16 x CUs + 5 tiny items whose kind cycles with period 7: every workgroup re-initialises its Wave for a second and a
    third item, behind an item that failed, ended in mid-window or left its lines and probabilities behind"""
    t_start = time.time()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 3 * WG_PER_CU * cus + 5
    assert n >= 3 * WG_PER_CU * cus
    rounds = E.rounds(n)
    judged = [(B.OK, data) if data is not None else (B.ERR_RESULT, b"") for _, _, data in rounds]
    names = ["rounds/%d/%s" % (i, E.ROUND_KINDS[i % 7]) for i in range(n)]
    for i in range(0, 7 * E.ROUND_VARIANTS):       # (each distinct item once; tests/test_bcj2_edges_cpu.py checks them more closely)
        st4, out_len, _ = rounds[i]
        st, out = B.decode(*st4, out_len)
        assert st == judged[i][0] and (st != B.OK or out == judged[i][1]), names[i]
    streams, items, ranges, cap = _lay_out([(st4, out_len, (5 * i + 1) % 16) for i, (st4, out_len, _) in enumerate(rounds)], lambda q: False)
    failed = sum(st != B.OK for st, _ in judged)
    print("rounds: %d items (%d of them fail) on %d CUs, a cap of %d workgroups: %.2f items per workgroup; %d bytes of destination"
          % (n, failed, cus, WG_PER_CU * cus, n / (WG_PER_CU * cus), cap))
    assert failed == sum(i % 7 in (2, 4) for i in range(n)) >= 2 * (n // 7)
    b = lzma_amd.Batch(ctx, streams)
    b.run()
    _merge_and_compare(ctx, b, items, ranges, cap, judged, names, "rounds")
    b.close()
    print("test_three_rounds_of_mixed_items: %.1f s wall" % (time.time() - t_start))
