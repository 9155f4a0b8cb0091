"""GPU: the Delta / BCJ filter kernels (lzma_amd/csrc/xlz_filter_dev.hip) on content that sits on the seams of their work
split -- the crafted cases of tests/filter_edges.py, which tests/test_filter_edges_cpu.py shows to bite.  Everything is
bit-exact and the judge is liblzma: it decodes the same raw LZMA2 streams with the filters in its chain."""
import random
import time
import zlib

import pytest

import filter_edges as E
import lzma_amd
from check_ref import CRC32
from lzma_amd import FMT_LZMA2_RAW

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def prepared():
    """per case name: (the raw LZMA2 stream, liblzma's result) -- built once, never changed"""
    out = {}
    t0 = time.time()
    for c in E.cases() + E.alternating_batch():
        comp = E.compressed(c)
        out[c.name] = (comp, E.liblzma(comp, c.steps))
    print("prepared %d cases in %.1f s" % (len(out), time.time() - t0))
    return out


def _stream(comp, n):
    return lzma_amd.Stream(comp, FMT_LZMA2_RAW, out_cap=n, dict_size=E.DICT)


def _compare(b, k, case, want, what):
    got = b.download(k, len(case.data))
    if got != want:
        at = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError("%s: case %s (%d bytes, steps %s) differs from liblzma at byte %d: got %02x, want %02x (input %02x)"
                             % (what, case.name, len(case.data), case.steps, at, got[at], want[at], case.data[at]))


def _filter_and_compare(ctx, b, items, steps, what):
    """items: [(stream index, case or None for a sentinel, expected bytes)]; steps as Batch.filter takes them"""
    b.run()
    res = b.results()
    for k, c, want in items:
        assert res[k][0] == len(want) and res[k][1] >= 0, (what, k, res[k])
    t0 = time.time()
    b.filter(steps)
    st = ctx.last_filter_stats()
    print("%s: %d steps, %.1f ms wall, stats %s" % (what, len(steps), 1e3 * (time.time() - t0), st))
    n_all = sum(len(c.steps) for _, c, _ in items if c)
    n_empty = sum(len(c.steps) for _, c, _ in items if c and not c.data)
    assert st["host_steps"] == 0 and st["empty_steps"] == n_empty and st["device_steps"] == n_all - n_empty, (what, st)
    assert st["device_bytes"] == sum(len(c.steps) * len(c.data) for _, c, _ in items if c) and st["kernel_ms"] > 0, (what, st)
    for k, c, want in items:
        if c:
            _compare(b, k, c, want, what)
        else:
            assert b.download(k, len(want)) == want, "%s: sentinel stream %d was touched" % (what, k)
    return st


def test_edge_cases_on_a_device_resident_batch(ctx, prepared):
    """Every case as a raw LZMA2 stream of one batch, in seeded shuffled order, every third stream a sentinel without steps
    that is full of opcodes; the steps of different streams interleaved.  Then the same once more on the scratch the
    first pass left behind, the streams' steps dealt in reverse order and the Delta group cases first, and a small second
    batch on the same context."""
    t_start = time.time()
    cs = E.cases()
    random.Random(7007).shuffle(cs)
    items, streams = [], []
    for i, c in enumerate(cs):
        comp, want = prepared[c.name]
        items.append((len(streams), c, want))
        streams.append(_stream(comp, len(c.data)))
        if i % 2 == 1:
            s = E.sentinel(i)
            items.append((len(streams), None, s))
            streams.append(_stream(E.raw_lzma2(s), len(s)))
    assert all(c is None for _, c, _ in items[2::3]) and len(items) == len(cs) + len(cs) // 2
    b = lzma_amd.Batch(ctx, streams)
    steps = [(k, f, p) for k, c, _ in items if c for f, p in c.steps]
    steps.sort(key=lambda s: s[0] * 7919 % 13)   # (streams in mixed order; a stable sort keeps the order of one stream's steps)
    st = _filter_and_compare(ctx, b, items, steps, "edge cases")
    assert 1 <= st["launches"] <= 3 * 7, st
    # dirty scratch: the window table, the rows and the group rows of the first pass are still there, laid out differently
    back = [(k, c) for k, c, _ in reversed(items) if c]
    back.sort(key=lambda kc: "/groups/" not in kc[1].name)
    _filter_and_compare(ctx, b, items, [(k, f, p) for k, c in back for f, p in c.steps], "edge cases, dirty scratch")
    b.close()
    by = {c.name: c for c in cs}
    small = [by["x86/nosync/257-windows/b"], by["delta/d255/groups/len%d" % (E.G * E.C + 1)]]
    b = lzma_amd.Batch(ctx, [_stream(prepared[c.name][0], len(c.data)) for c in small])
    _filter_and_compare(ctx, b, [(k, c, prepared[c.name][1]) for k, c in enumerate(small)],
                        [(k, f, p) for k, c in enumerate(small) for f, p in c.steps], "a second batch")
    b.close()
    print("test_edge_cases_on_a_device_resident_batch: %.1f s wall" % (time.time() - t_start))


def test_single_step_launches(ctx, prepared):
    """a launch whose table has one entry, per class of kernel; and tables in which streams of no bytes, one tile and many
    tiles take turns, so that the search for a tile's step ends at the table's first and last entry"""
    t_start = time.time()
    for batch, launches in zip(E.single_step_batches(), (1, 2, 4)):
        b = lzma_amd.Batch(ctx, [_stream(prepared[c.name][0], len(c.data)) for c in batch])
        st = _filter_and_compare(ctx, b, [(k, c, prepared[c.name][1]) for k, c in enumerate(batch)],
                                 [(k, f, p) for k, c in enumerate(batch) for f, p in c.steps], "one step: " + batch[0].name)
        assert st["device_steps"] == 1 and st["launches"] == launches, st
        b.close()
    batch = E.alternating_batch()
    b = lzma_amd.Batch(ctx, [_stream(prepared[c.name][0], len(c.data)) for c in batch])
    st = _filter_and_compare(ctx, b, [(k, c, prepared[c.name][1]) for k, c in enumerate(batch)],
                             [(k, f, p) for k, c in enumerate(batch) for f, p in c.steps], "alternating sizes")
    assert st["empty_steps"] == 16 and st["launches"] == 7, st
    b.close()
    print("test_single_step_launches: %.1f s wall" % (time.time() - t_start))


def test_edge_cases_through_the_filtered_call(ctx, prepared):
    """the Thumb cases at the tile edge, the x86 runs of 257 windows and the Delta streams of three groups through
    decode_batch_filtered, each with a CRC32 over its whole output: the bytes are liblzma's, the digests zlib's"""
    t_start = time.time()
    edge = ("@%d" % E.TB, "@%d" % (E.TB - 2), "@%d" % (E.TB - 4), "@%d" % (E.TB + 2), ",%d" % E.TB, "/tile+", "/base%d/" % E.TB)
    sub = [c for c in E.cases() if (c.name.startswith("thumb/") and any(e in c.name for e in edge))
           or c.name.startswith("x86/nosync/257-windows") or (c.name.startswith("delta/") and E.probes(c)["delta"]["groups"] == 3)]
    assert len(sub) == 28 + 4 + 6, [c.name for c in sub]
    random.Random(7008).shuffle(sub)
    streams = [_stream(prepared[c.name][0], len(c.data)) for c in sub]
    steps = [(k, f, p) for k, c in enumerate(sub) for f, p in c.steps]
    got, dig = lzma_amd.decode_batch_filtered(ctx, streams, steps, [(k, 0, len(c.data) + 1, CRC32) for k, c in enumerate(sub)])
    st = ctx.last_filter_stats()
    print("decode_batch_filtered: %d streams, stats %s" % (len(sub), st))
    for k, c in enumerate(sub):
        want = prepared[c.name][1]
        assert got[k][1] >= 0 and len(got[k][0]) == len(want), (c.name, got[k][1:])
        if got[k][0] != want:
            at = next(i for i in range(len(want)) if got[k][0][i] != want[i])
            raise AssertionError("case %s (steps %s) differs from liblzma at byte %d" % (c.name, c.steps, at))
        assert dig[k] == zlib.crc32(want), c.name
    assert st["host_steps"] == 0 and st["empty_steps"] == 0 and st["device_steps"] == len(steps), st
    assert st["device_bytes"] == sum(len(c.data) for c in sub), st
    print("test_edge_cases_through_the_filtered_call: %.1f s wall" % (time.time() - t_start))
