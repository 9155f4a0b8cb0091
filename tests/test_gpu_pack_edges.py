"""GPU: the pack kernel (lzma_amd/csrc/xlz_pack_dev.hip) on tables that sit on the seams of its work split -- the crafted
plans of tests/pack_edges.py, which tests/test_pack_edges_cpu.py shows to bite -- at a destination pointer that is 0 and 5
modulo 16, and on a destination of three times as many tiles as a launch has workgroups, and one more.  Everything is
bit-exact: the whole destination against the sources' bytes laid out item by item (pack_edges.expect_pack)."""
import lzma
import time

import numpy as np
import pytest
import torch   # (before libxlz.so is loaded: torch brings its own HIP runtime, which must be the one that initialises the device)

import corpus
import lzma_amd
import pack_edges as E
from lzma_amd import FMT_LZMA2_RAW

pytestmark = pytest.mark.gpu

DICT = 1 << 16
WG_PER_CU = 8   # kPackWgPerCu of xlz_pack_dev.hip: the cap of workgroups per CU
SLACK = 64


@pytest.fixture(scope="module")
def world(ctx):
    """the batch of the source streams, run once -> (batch, liblzma's decode of each stream)"""
    plains = E.plains()
    streams = []
    for p in plains:
        segs = [p[o:o + (1 << 20)] for o in range(0, len(p), 1 << 20)]
        comp = corpus.lzma2_concat(segs, dict_size=DICT, preset=0)
        assert lzma.decompress(comp, format=lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA2, "dict_size": DICT}]) == p
        streams.append(lzma_amd.Stream(comp, FMT_LZMA2_RAW, out_cap=len(p), dict_size=DICT))
    b = lzma_amd.Batch(ctx, streams)
    b.run()
    for k, (n, st, _) in enumerate(b.results()):
        assert n == len(plains[k]) and st >= 0, (k, n, st)
    yield b, plains
    b.close()


def _pack_and_compare(ctx, b, plains, items, cap, mis, what):
    """one Batch.pack call into a destination whose address is `mis` modulo 16 (SLACK bytes of FILL behind it, `mis` in
    front): the whole allocation against the expectation, on the device"""
    dst = torch.full((mis + cap + SLACK,), E.FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert dst.data_ptr() % 16 == 0
    want, copied, stats = E.expect_pack(items, plains, cap, mis)
    assert copied == [n for _, _, n, _ in items] and stats["empty_items"] == 0
    whole = torch.from_numpy(np.frombuffer(bytes([E.FILL]) * mis + want + bytes([E.FILL]) * SLACK, dtype=np.uint8).copy()).cuda()
    t0 = time.time()
    assert b.pack(items, dst.data_ptr() + mis, cap) == copied
    ps = ctx.last_pack_stats()
    print("%s, mis %d: %d items, %d bytes into %d, %.1f ms wall, stats %s" % (what, mis, len(items), stats["bytes"], cap, 1e3 * (time.time() - t0), ps))
    if not torch.equal(dst, whole):
        at = int(torch.nonzero(dst != whole)[0]) - mis
        raise AssertionError("%s, mis %d: the destination differs at dst_off %d (kernel offset %d: tile %d + %d)"
                             % (what, mis, at, at + mis, (at + mis) // E.TILE, (at + mis) % E.TILE))
    assert {k: ps[k] for k in stats} == stats and ps["launches"] == 1 and ps["kernel_ms"] > 0, (what, mis, ps, stats)
    return stats


@pytest.mark.parametrize("mis", E.MIS)
@pytest.mark.parametrize("family", E.FAMILIES)
def test_edge_tables(ctx, world, family, mis):
    t_start = time.time()
    b, plains = world
    sizes, items, cap, probe = E.plan(family, mis)
    assert sizes == tuple(len(p) for p in plains)
    counted = probe()
    stats = _pack_and_compare(ctx, b, plains, items, cap, mis, family)
    assert 0 < stats["congruent_items"] < stats["items"] == len(items)
    print("test_edge_tables[%s-%d]: %s, %.1f s wall" % (family, mis, counted, time.time() - t_start))


def test_three_rounds_of_tiles(ctx, world):
    """3 x 8 x CUs + 1 tiles, one item of 100 to 700 bytes in each: every workgroup walks tile0 + t for t >= gridDim.x, twice
    and more"""
    t_start = time.time()
    b, plains = world
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_tiles = 3 * WG_PER_CU * cus + 1
    assert n_tiles >= 3 * WG_PER_CU * cus
    for mis in E.MIS:
        sizes, items, cap, probe = E.rounds(n_tiles, mis)
        counted = probe()
        assert counted["tiles"] == n_tiles == E.tiles_of(items, mis)[1] and cap + mis == n_tiles * E.TILE
        print("rounds, mis %d: %s on %d CUs, a cap of %d workgroups: %.2f tiles per workgroup"
              % (mis, counted, cus, WG_PER_CU * cus, n_tiles / (WG_PER_CU * cus)))
        _pack_and_compare(ctx, b, plains, items, cap, mis, "rounds")
    print("test_three_rounds_of_tiles: %.1f s wall" % (time.time() - t_start))
