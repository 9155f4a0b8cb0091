"""GPU: the CRC32 / CRC64 / SHA-256 kernels (lzma_amd/csrc/xlz_check_dev.hip, xlz_sha256_dev.hip) on ranges that sit on the
seams of their work split -- the crafted cases of tests/digest_edges.py, which tests/test_digest_edges_cpu.py shows to
bite.  Everything is bit-exact; the judges are zlib, liblzma and hashlib over the plain bytes (digest_edges.expected), never
the library's host code.  Two streams are decoded once for the whole module, "long" (64.4 MiB) among them: its ranges of 258
and more segments give the fold's threads a second and a third Horner trip, the one checks call of all CRC cases gives every
wave of the segment kernels three trips and more through a table of mixed ranges, and sha/rounds needs a second launch."""
import random
import time

import pytest
import torch   # (before libxlz.so is loaded: torch brings its own HIP runtime, which must be the one that initialises the device)

import digest_edges as E
import lzma_amd
import pipeline_streams as ps
from digest_edges import CRC32, CRC64, SHA

pytestmark = pytest.mark.gpu

DICT = 1 << 16


@pytest.fixture(scope="module")
def world(ctx):
    """the batch of the two streams, run once, and every case's expected digest (kept by digest_edges)"""
    t0 = time.time()
    raws = [E.raw_lzma2(E.stream(s)) for s in E.STREAMS]
    t1 = time.time()
    print("prepared the raw LZMA2 streams (%d and %d bytes) in %.2f s" % (len(raws[0]), len(raws[1]), t1 - t0))
    jobs = [ps.raw2_job(raw, len(E.stream(s)), DICT) for raw, s in zip(raws, E.STREAMS)]
    b = lzma_amd.Batch(ctx, [j[0] for j in jobs])
    b.run()
    res = b.results()
    for k, s in enumerate(E.STREAMS):
        w, w_st, w_in = jobs[k][1]()
        assert w == E.stream(s) and res[k] == (len(w), w_st, w_in) and w_st >= 0, (s, res[k], w_st, w_in)
        assert b.download(k, len(w)) == w, s
    t2 = time.time()
    E.expected(E.cases() + [E.BALLAST, WHOLE_LONG])
    print("decoded and downloaded in %.1f s, the judges' digests of %d cases in %.1f s" % (t2 - t1, len(E.cases()), time.time() - t2))
    yield b, raws
    b.close()


WHOLE_LONG = E.Case("sha/whole-long", "long", 0, E.LONG_BYTES + 100, SHA)   # longer than a lane may take: the host's


def _show(d):
    return d.hex() if isinstance(d, bytes) else "%016x" % d


def _compare(cs, got, what):
    want = E.expected(cs)
    assert len(got) == len(cs) == len(want)
    bad = [(c, g, w) for c, g, w in zip(cs, got, want) if g != w]
    if bad:
        lines = ["%s %s: got %s, want %s" % (c, E.probes(c), _show(g), _show(w)) for c, g, w in bad[:8]]
        raise AssertionError("%s: %d of %d digests differ from the judge's:\n%s" % (what, len(bad), len(cs), "\n".join(lines)))


def _n_bytes(cs):
    return sum(hi - lo for lo, hi in map(E.clip, cs))


def _checks(ctx, b, cs, what, launches=1):
    """cs through Batch.checks: every digest against its judge, and the device did all of it"""
    t0 = time.time()
    got = b.checks([E.as_range(c) for c in cs])
    st = ctx.last_check_stats()
    print("%s: %d ranges, %.1f ms wall, stats %s" % (what, len(cs), 1e3 * (time.time() - t0), st))
    _compare(cs, got, what)
    n_empty = sum(1 for c in cs if not E.probes(c)["m"])
    assert (st["host_ranges"], st["empty_ranges"], st["device_ranges"]) == (0, n_empty, len(cs) - n_empty), (what, st)
    assert st["launches"] == launches and st["device_bytes"] == _n_bytes(cs) and (st["kernel_ms"] > 0) == (launches > 0), (what, st)
    return st


def test_crc_edges_in_one_launch(ctx, world):
    """every CRC case of both kinds in ONE checks call: the segment kernels walk 27 000 segments per kind grid-stride, three
    trips and more per wave, through a table in which ranges of one and of several segments take turns"""
    t_start = time.time()
    b, _ = world
    order = E.one_launch_order()
    assert sorted(order) == sorted(E.cases("crc"))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for kind, per_cu in ((CRC32, 8), (CRC64, 4)):
        tab = E.table_of(order, kind)
        n_many = sum(m > 1 for m in tab)
        print("kind %d: %d ranges, %d of several segments, %d segments; %d CUs: %.1f trips per wave"
              % (kind, len(tab), n_many, sum(tab), cus, sum(tab) / (4.0 * per_cu * cus)))
        assert sum(tab) >= 3 * 4 * per_cu * cus, (kind, sum(tab), cus)
        assert n_many >= 200 and tab[0] == tab[-1] == 1 and E.changes(tab) == 2 * n_many, kind
    _checks(ctx, b, order, "all CRC cases")
    print("test_crc_edges_in_one_launch: %.1f s wall" % (time.time() - t_start))


def test_crc_edges_on_dirty_scratch(ctx, world):
    """the batch's check buffers shrink, grow again and hold the segment values of the call before: all cases, ten of them,
    all in reverse order, the fold family alone"""
    t_start = time.time()
    b, _ = world
    order = E.one_launch_order()
    _checks(ctx, b, order, "all CRC cases")
    few = random.Random(8400).sample(order, 8) + [c for c in E.cases("crc/fold") if "/m515/off3/full" in c.name]
    assert len(few) == 10 and {c.kind for c in few} == set(E.KINDS)
    _checks(ctx, b, few, "ten ranges")
    _checks(ctx, b, order[::-1], "all CRC cases, last to first")
    _checks(ctx, b, E.cases("crc/fold"), "the fold family")
    print("test_crc_edges_on_dirty_scratch: %.1f s wall" % (time.time() - t_start))


def test_crc_tables_of_one(ctx, world):
    """a table of one range (the search for a segment's range has nothing to halve), of one segment and of 515; and calls
    of one kind only: without CRC32 ranges the CRC64 table and its segment values start where the buffers start"""
    t_start = time.time()
    b, _ = world
    by = {c.name: c for c in E.cases("crc")}
    for kind in E.KINDS:
        tag = E.TAG[kind]
        for name in ("crc/segments/%s/one-byte-at-127", "crc/short/%s/off1136/len300", "crc/fold/%s/m515/off3/full",
                     "crc/fold/%s/m515/off0/one-byte", "crc/fold/%s/m258/off3/full"):
            c = by[name % tag]
            st = _checks(ctx, b, [c], "one range: " + c.name)
            assert st["device_ranges"] == 1, st
        assert E.probes(by["crc/fold/%s/m515/off3/full" % tag])["m"] == 515 and E.probes(by["crc/short/%s/off1136/len300" % tag])["m"] == 1
        only = [c for c in E.cases("crc") if c.kind == kind and E.family(c) in ("crc/rows", "crc/segments", "crc/fold")]
        random.Random(8401).shuffle(only)
        _checks(ctx, b, only, "%s only" % tag)
    print("test_crc_tables_of_one: %.1f s wall" % (time.time() - t_start))


def _digests(ctx, b, cs, what):
    """cs through Batch.digests: every digest against its judge, and who hashed what is what the plan says
    -> (SHA-256 statistics, the plan's verdict per non-empty SHA-256 range in call order)"""
    t0 = time.time()
    got = b.digests([E.as_range(c) for c in cs])
    st, c_st = ctx.last_sha256_stats(), ctx.last_check_stats()
    print("%s: %d ranges, %.1f ms wall, sha256 stats %s, check stats %s" % (what, len(cs), 1e3 * (time.time() - t0), st, c_st))
    _compare(cs, got, what)
    sha = [c for c in cs if c.kind == SHA]
    lens = [hi - lo for lo, hi in map(E.clip, sha) if hi > lo]
    on = lzma_amd.sha256_plan(lens)
    n_dev, dev_bytes = sum(on), sum(n for n, d in zip(lens, on) if d)
    assert (st["device_ranges"], st["device_bytes"]) == (n_dev, dev_bytes), (what, st)
    assert (st["host_ranges"], st["host_bytes"]) == (len(lens) - n_dev, sum(lens) - dev_bytes), (what, st)
    assert st["empty_ranges"] == len(sha) - len(lens) and (st["kernel_ms"] > 0) == (n_dev > 0), (what, st)
    assert st["launches"] == -(-n_dev // E.ROUND), (what, st)
    crc = [c for c in cs if c.kind != SHA]
    n_crc = sum(1 for c in crc if E.probes(c)["m"])
    assert c_st["host_ranges"] == st["host_ranges"] and c_st["device_ranges"] == n_dev + n_crc, (what, c_st)
    assert c_st["empty_ranges"] == st["empty_ranges"] + len(crc) - n_crc, (what, c_st)
    return st, on


def test_sha_edges(ctx, world):
    """sha/grid and sha/blocks among 200 CRC cases in one digests call, in shuffled order: every shift of the start times
    every tail, the padding's corners behind 1 to 1000 full blocks.  The plan leaves the few ranges of 1000 blocks to the
    host's threads; so once more with a range in the call that keeps those threads busy: then they are the device's too"""
    t_start = time.time()
    b, _ = world
    rnd = random.Random(8402)
    cs = E.cases("sha/grid") + E.cases("sha/blocks") + rnd.sample([c for c in E.cases("crc") if E.clip(c)[1] - E.clip(c)[0] < 1 << 20], 200)
    for extra in ([], [WHOLE_LONG]):
        call = cs + extra
        rnd.shuffle(call)
        st, on = _digests(ctx, b, call, "sha/grid, sha/blocks, 200 CRC cases" + (" and the whole of long" if extra else ""))
        assert st["device_ranges"] > 12000 and st["launches"] == 1, st
    sha = [c for c in call if c.kind == SHA and c.len]
    assert [c.name for c, d in zip(sha, on) if not d] == [WHOLE_LONG.name] and st["device_ranges"] == len(sha) - 1, st
    print("test_sha_edges: %.1f s wall" % (time.time() - t_start))


def test_sha_single_waves(ctx, world):
    """a launch of one wave whose 64 lanes all have another number of blocks; of two waves, the second of one lane; of one
    lane; of 63 lanes.  Each set in a call of its own, with the range that keeps the host's threads busy (digest_edges.wave_set)"""
    t_start = time.time()
    b, _ = world
    for n in E.WAVE_SETS:
        call = E.wave_set(n) + [E.BALLAST]
        st, on = _digests(ctx, b, call, "a wave set of %d" % n)
        assert on == [True] * n + [False], n
        assert (st["device_ranges"], st["host_ranges"], st["empty_ranges"], st["launches"]) == (n, 1, 1, 1), (n, st)
    print("test_sha_single_waves: %.1f s wall" % (time.time() - t_start))


def test_sha_second_launch(ctx, world):
    """one round of lanes and 65 ranges more: the second launch reads its table behind the first one's and writes its digests
    behind the first one's; every range has other bytes, so a digest at the wrong index shows.  Twice on the same batch"""
    t_start = time.time()
    b, _ = world
    cs = E.cases("sha/rounds")
    assert len(cs) == E.ROUND + 65
    for run in range(2):
        st, on = _digests(ctx, b, cs, "sha/rounds, run %d" % run)
        assert all(on) and (st["launches"], st["host_ranges"], st["device_ranges"]) == (2, 0, E.ROUND + 65), st
    print("test_sha_second_launch: %.1f s wall" % (time.time() - t_start))


def test_edges_through_the_one_call_pipeline(ctx, world):
    """crc/rows, crc/segments and sha/blocks -- the families that need "grid" only -- through decode_batch_digests: the
    same digests, the decoded bytes, and on the host only the SHA-256 ranges the plan leaves there"""
    t_start = time.time()
    _, raws = world
    grid = E.stream("grid")
    cs = E.cases("crc/rows") + E.cases("crc/segments") + E.cases("sha/blocks")
    assert all(c.stream == "grid" for c in cs)
    random.Random(8403).shuffle(cs)
    s = lzma_amd.Stream(raws[0], lzma_amd.FMT_LZMA2_RAW, out_cap=len(grid), dict_size=DICT)
    got, dig = lzma_amd.decode_batch_digests(ctx, [s], [E.as_range(c) for c in cs])
    assert got[0][0] == grid and got[0][1] >= 0
    _compare(cs, dig, "decode_batch_digests")
    st, c_st = ctx.last_sha256_stats(), ctx.last_check_stats()
    print("decode_batch_digests: %d ranges, sha256 stats %s, check stats %s" % (len(cs), st, c_st))
    sha = [c for c in cs if c.kind == SHA]
    on = lzma_amd.sha256_plan([c.len for c in sha])
    n_host = len(sha) - sum(on)
    assert c_st["host_ranges"] == n_host == st["host_ranges"] and st["device_ranges"] == sum(on) > 0, (st, c_st)
    assert c_st["empty_ranges"] == 0 and c_st["device_ranges"] == len(cs) - n_host, c_st
    print("test_edges_through_the_one_call_pipeline: %.1f s wall" % (time.time() - t_start))
