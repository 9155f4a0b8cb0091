"""GPU: the Delta / BCJ filters undone on the device between decode and check (lzma_amd/csrc/xlz_filter_dev.hip) --
Batch.filter on a device-resident batch, decode_batch_filtered in the three forms of the host pipeline, and the .xz / .7z
front-ends in filter mode 1.  Everything is bit-exact.  The judge is liblzma (tests/filter_ref.py): for raw LZMA2 streams
it decodes AND filters (filters=[..., LZMA2]); for the pipeline's stream sets, whose unfiltered results the oracle gives,
the expected bytes are those results passed through filter_host, which tests/test_filter_dev.py holds against liblzma.
Content placed ON the seams of the kernels' work split (lane, wave, tile, window, chunk and group edges) is in
tests/test_gpu_filter_edges.py; the buffers here meet those seams by chance."""
import ctypes
import lzma
import random
import struct
import time
import zlib

import numpy as np
import pytest

import check_ref
import corpus
import filter_ref as R
import lzma_amd
import pipeline_streams as ps
import sevenzip_chains as Z
import xz_chains as X
from check_ref import CRC32, CRC64
from lzma_amd import FMT_LZMA2_RAW, LzmaError
from lzma_amd import _native as N

pytestmark = pytest.mark.gpu

DICT = 1 << 16


def _liblzma(comp, steps):
    """a raw LZMA2 stream decoded and passed through `steps` (decoder order) by liblzma alone"""
    chain = [R.filter_dict(f, p) for f, p in reversed(steps)] + [{"id": lzma.FILTER_LZMA2, "dict_size": DICT}]
    return lzma.decompress(comp, format=lzma.FORMAT_RAW, filters=chain)


def _chains(rnd, k):
    """the steps of stream k: every (filter, parameter) pair once as a single step in turn, then seeded chains of one to
    three steps"""
    singles = [(f, p) for f in R.ALL for p in R.params(f)]
    if k < len(singles):
        return [singles[k]]
    return [rnd.choice(singles) for _ in range(rnd.choice((1, 2, 2, 3, 3)))]


def test_filter_on_a_device_resident_batch(ctx):
    """300 raw LZMA2 streams of 0 bytes to 8 MiB (opcodes of all seven filters; real machine code) and one of 300 MiB that
    spans thousands of workgroups; every filter with every parameter, chains of two and three steps.  The downloaded
    bytes are liblzma's, Batch.checks afterwards gives the CRCs of the filtered bytes, and a new run decodes afresh."""
    rnd = random.Random(8008)
    sizes = [0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 18, 31, 33, 255, 256, 257, 261, 4095, 4096, 4101, 16379, 16384, 16389, 32768 + 1,
             65531, 65536, 65541, 100_000, 262_144 + 3, 1 << 20, (1 << 20) + 16385, 3_000_001, 8 << 20]
    code = R.machine_code(9 << 20, 0)
    plains = [R.opcode_soup(n, 100 + i) if n <= 300_000 else code[i * 4096: i * 4096 + n] for i, n in enumerate(sizes)]
    comps = []
    for p in plains:
        segs = [p[o:o + (1 << 20)] for o in range(0, len(p), 1 << 20)] or [b""]
        comps.append(corpus.lzma2_concat(segs, dict_size=DICT, preset=0))
    order = [i % len(sizes) for i in range(300)]
    rnd.shuffle(order)
    streams = [lzma_amd.Stream(comps[i], FMT_LZMA2_RAW, out_cap=len(plains[i]), dict_size=DICT) for i in order]
    steps_of = [_chains(rnd, k) for k in range(len(order))]
    # one stream of 300 MiB: 300 units of 1 MiB (eight different ones), x86 then Delta
    segs = [code[(k + 1) * 333_333: (k + 1) * 333_333 + (1 << 20)] for k in range(8)]
    parts = [corpus.compress_raw_lzma2(s, dict_size=DICT, preset=0)[:-1] for s in segs]
    big_comp = b"".join(parts[k % 8] for k in range(300)) + b"\x00"
    big_at = len(streams) // 2
    streams.insert(big_at, lzma_amd.Stream(big_comp, FMT_LZMA2_RAW, out_cap=300 << 20, dict_size=DICT))
    steps_of.insert(big_at, [(R.X86, 4096), (R.DELTA, 3)])
    order.insert(big_at, -1)

    memo = {}

    def want(k):
        key = (order[k], tuple(steps_of[k]))
        if key not in memo:
            memo[key] = _liblzma(big_comp if order[k] < 0 else comps[order[k]], steps_of[k])
        return memo[key]

    b = lzma_amd.Batch(ctx, streams)
    b.run()
    res = b.results()
    for k, s in enumerate(streams):
        assert res[k][0] == s.out_cap and res[k][1] >= 0, (k, res[k])
    steps = [(k, f, p) for k in range(len(streams)) for f, p in steps_of[k]]
    steps.sort(key=lambda s: s[0] * 7919 % 13)   # (streams in mixed order; a stable sort keeps the order of one stream's steps)
    t0 = time.time()
    b.filter(steps)
    st = ctx.last_filter_stats()
    print("Batch.filter: %d steps, %.1f ms wall, stats %s" % (len(steps), 1e3 * (time.time() - t0), st))
    n_empty = sum(len(steps_of[k]) for k, s in enumerate(streams) if s.out_cap == 0)
    assert st["host_steps"] == 0 and st["empty_steps"] == n_empty and st["device_steps"] == len(steps) - n_empty, st
    assert st["device_bytes"] == sum(len(steps_of[k]) * s.out_cap for k, s in enumerate(streams)) and st["kernel_ms"] > 0, st
    assert 1 <= st["launches"] <= 3 * 7, st   # (BCJ 1, x86 2, Delta 4 kernels per round of steps)
    changed = 0
    for k, s in enumerate(streams):
        got = b.download(k, s.out_cap)
        w = want(k)
        if got != w:
            at = next(i for i in range(len(w)) if got[i] != w[i])
            raise AssertionError("stream %d (%d bytes, steps %s) differs from liblzma at byte %d" % (k, s.out_cap, steps_of[k], at))
        if order[k] >= 0 and 4095 <= s.out_cap <= 300_000:   # (opcode soup: a quarter of its words are work for some filter)
            assert w != plains[order[k]], (k, steps_of[k])
            changed += 1
    assert changed >= 96   # (12 of the 34 sizes, each at least eight times among the 300)
    # the checks read the filtered bytes
    ranges = [(k, 0, s.out_cap + 9, CRC64 if (k % 3 == 0 and s.out_cap <= 1 << 20) else CRC32) for k, s in enumerate(streams)]
    ranges += [(big_at, (100 << 20) + 1, (64 << 20) + 5, CRC32)]
    for (k, off, length, kind), g in zip(ranges, b.checks(ranges)):
        w = want(k)[off: off + length]
        assert g == check_ref.digest(kind, w), (k, off, length, kind)
    # a later run decodes afresh; the same steps give the same bytes again
    b.run()
    b.results()
    for k in (0, 1, big_at + 1, len(streams) - 1):
        assert b.download(k, streams[k].out_cap) == plains[order[k]]
    b.filter([s for s in steps if s[0] == len(streams) - 1])
    assert b.download(len(streams) - 1, streams[-1].out_cap) == want(len(streams) - 1)
    # argument errors
    for bad in ([(len(streams), R.X86, 0)], [(0, 10, 0)], [(0, 2, 0)], [(0, R.DELTA, 0)], [(0, R.DELTA, 257)], [(0, R.ARM, 2)],
                [(0, R.IA64, 8)], [(3, R.X86, 0)] * 4):
        with pytest.raises(LzmaError) as e:
            b.filter(bad)
        assert e.value.status == lzma_amd.ERR_BAD_ARG, bad
    b.filter([])
    b.close()


# ---- decode_batch_filtered in the three forms of the pipeline ------------------------------------------------------------
def _flat_call_filtered(ctx, streams, steps, ranges):
    """pipeline_streams.flat_call through xlz_decode_batch_filtered -> (status, out, offsets, results, digests)"""
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
    arr = (N.CheckRange * max(len(ranges), 1))()
    for q, (stream, off, length, kind) in enumerate(ranges):
        arr[q].stream, arr[q].off, arr[q].len, arr[q].kind = stream, off, length, kind
    dig = np.zeros(max(len(ranges), 1), dtype=np.uint64)
    st = N.lib().xlz_decode_batch_filtered(ctx._h, descs, n, res, lzma_amd._make_steps(steps), len(steps), arr, len(ranges),
                                           dig.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
    return st, out, offs, [(r.out_len, r.status, r.in_consumed) for r in res], dig


def _filtered_pipeline(ctx, jobs, forced=()):
    """One filtered call over `jobs`: steps (one to three, seeded) on a seeded half of the streams and on every stream of
    `forced`, a whole-output CRC32 per stream.  Statuses and consumed input are the oracle's -- the unfiltered call's --,
    the bytes are the oracle's passed through filter_host, the digests zlib's CRC32 of those.  -> (call stats, filter stats)"""
    rnd = random.Random(9009)
    singles = [(f, p) for f in R.ALL for p in R.params(f)]
    pool = [[rnd.choice(singles) for _ in range(1 + q % 3)] for q in range(24)]   # (few different chains: results are shared)
    chain = {i: pool[rnd.randrange(len(pool))] for i in range(len(jobs)) if rnd.random() < 0.5 or i in forced}
    steps = [(i, f, p) for i in sorted(chain) for f, p in chain[i]]
    ranges = [(i, 0, j[0].out_cap + 1, CRC32) for i, j in enumerate(jobs)]
    st, out, offs, res, dig = _flat_call_filtered(ctx, [j[0] for j in jobs], steps, ranges)
    assert st == 0
    s, f = ctx.last_call_stats(), ctx.last_filter_stats()
    print("call stats:", s, "filter stats:", f)
    memo, bad = {}, []
    for i, (_, want) in enumerate(jobs):
        w, w_st, w_in = want()
        key = (id(want), id(chain.get(i)))
        if key not in memo:
            e = w
            for fid, prm in chain.get(i, ()):
                e = lzma_amd.filter_host(fid, prm, e)
            memo[key] = (np.frombuffer(e, dtype=np.uint8), zlib.crc32(e))
        e, crc = memo[key]
        if res[i] != (len(w), w_st, w_in) or not np.array_equal(out[offs[i]: offs[i] + len(w)], e) or int(dig[i]) != crc:
            bad.append(i)
    assert bad == [], "%d streams differ from the unfiltered call + filter_host, first %s (steps %s)" % (
        len(bad), bad[:10], [chain.get(i) for i in bad[:10]])
    n_empty = sum(len(chain[i]) for i in chain if res[i][0] == 0)
    assert f["host_steps"] == 0 and f["empty_steps"] == n_empty and f["device_steps"] == len(steps) - n_empty, f
    assert f["device_bytes"] == sum(len(chain[i]) * res[i][0] for i in chain) and f["kernel_ms"] > 0, f
    return s, f


def test_filtered_call_of_one_piece(ctx):
    """Mode 0: the mixed-kind set among 1200 streams of 256 KiB, with slicing asked for as tests/test_gpu_checks.py does --
    a call with steps must not run sliced.  The set holds malformed LZMA2 streams whose copies read behind dictionary
    resets and streams whose models do not fit LDS: collect() decodes them again behind the launch, and every one of
    them carries steps here -- a filter queued in front of those re-runs would be overwritten by them."""
    mixed = ps.mixed_kind_jobs()
    fill = [ps.alone_job(corpus.compress_alone(corpus.plain("TMZR"[d % 4], 95_800 + d, 256 << 10), preset=0), 256 << 10)
            for d in range(24)]
    jobs = [fill[i % 24] for i in range(1200 + len(mixed))]
    forced = set()
    for k, j in enumerate(mixed):
        jobs[k * len(jobs) // len(mixed)] = j
        if k >= len(mixed) - 56:   # the 40 + 16 crafted LZMA2 streams at the end of the set
            forced.add(k * len(jobs) // len(mixed))
    assert lzma_amd.decode_batch_plan([j[0].out_cap for j in jobs])[1] == 0
    ctx.set_slicing(1, 1 << 20, 3)
    try:
        for run in range(2):
            s, f = _filtered_pipeline(ctx, jobs, forced)
            assert s["slices"] <= 1 and s["sub_batches"] == 1, s
        # the same call without steps is the sliced call it always was
        st, out, offs, res, _ = _flat_call_filtered(ctx, [j[0] for j in jobs], [], [])
        assert st == 0 and ctx.last_call_stats()["slices"] == 3
        assert ps.flat_mismatches(jobs, out, offs, res) == []
    finally:
        ctx.set_slicing(0, 0, 0)


def test_filtered_call_of_overlapping_pieces(ctx):
    """Mode 1: 16 384 streams of 32-128 KiB (tests/test_gpu_checks.py's shape); piece k is filtered and checked while
    piece k + 1 decodes"""
    from test_gpu_pipeline import _specials
    nd, n = 48, 16384
    sizes = [32 << 10, 64 << 10, 96 << 10, 128 << 10]
    cs = [corpus.compress_alone(corpus.plain("TMZR"[d % 4], 93_500 + d, sizes[(d // 4) % 4]), preset=0) for d in range(nd)]
    common = [ps.alone_job(cs[d], sizes[(d // 4) % 4]) for d in range(nd)]
    jobs = [common[(i * 7) % nd] for i in range(n)]
    cuts, mode = lzma_amd.decode_batch_plan([j[0].out_cap for j in jobs])
    assert mode == 1 and len(cuts) >= 4, (cuts, mode)
    at = set()
    for a, b in zip(cuts, cuts[1:]):
        at |= {a, b - 1, a + 1, b - 2}
    rnd = random.Random(6006)
    for k, i in enumerate(sorted(at)):
        jobs[i] = _specials(rnd, jobs[i][0].out_cap, 94_000 + 10 * k)[k % 8]
    assert lzma_amd.decode_batch_plan([j[0].out_cap for j in jobs]) == (cuts, mode)
    s, f = _filtered_pipeline(ctx, jobs, at)
    assert s["sub_batches"] == len(cuts) - 1 and s["streams"] == n, s


def test_filtered_call_of_one_round_pieces(ctx):
    """Mode 2: 8193 streams of 256 KiB and 300 KiB, LZMA1 and LZMA2 of 2-4 units; the pieces that have steps (all three)
    run unsliced, one behind the other"""
    nd, n = 48, 8193
    caps = [256 << 10, 300 << 10]
    common = []
    for d in range(nd):
        cap = caps[d % 2]
        if d % 3:
            k = 2 + d % 3
            segs = [corpus.plain("TMZR"[(d + j) % 4], 95_700 + 10 * d + j, cap // k) for j in range(k - 1)]
            segs.append(corpus.plain("T", 95_700 + 10 * d + 9, cap - (k - 1) * (cap // k)))
            common.append(ps.raw2_job(corpus.lzma2_concat(segs, preset=0), cap))
        else:
            common.append(ps.alone_job(corpus.compress_alone(corpus.plain("TMZR"[d % 4], 95_600 + d, cap), preset=0), cap))
    jobs = [common[(i * 5) % nd] for i in range(n)]
    assert lzma_amd.decode_batch_plan([j[0].out_cap for j in jobs]) == ([0, 4096, 8192, 8193], 2)
    s, f = _filtered_pipeline(ctx, jobs, {8192})
    assert s["sub_batches"] == 3 and s["streams"] == n and s["slices"] <= 1, s


def test_filtered_call_argument_errors(ctx):
    s = lzma_amd.Stream(corpus.compress_alone(b"abc" * 100, preset=0), out_cap=300)
    for bad in ([(2, R.X86, 0)], [(0, 11, 0)], [(0, R.DELTA, 300)], [(0, R.SPARC, 3)], [(1, R.X86, 0)] * 4):
        with pytest.raises(LzmaError) as e:
            lzma_amd.decode_batch_filtered(ctx, [s, s], bad)
        assert e.value.status == lzma_amd.ERR_BAD_ARG, bad
    got, dig = lzma_amd.decode_batch_filtered(ctx, [s, s], [(1, R.DELTA, 1), (1, R.DELTA, 2)], [(1, 0, 300, CRC32), (0, 0, 300, CRC64)])
    want = R.apply_steps([(R.DELTA, 1), (R.DELTA, 2)], b"abc" * 100)
    assert got[0][0] == b"abc" * 100 and got[1][0] == want
    assert dig == [zlib.crc32(want), check_ref.crc64(b"abc" * 100)]
    # a slice of an LZMA2 stream has no start for a filter to count from
    c = corpus.lzma2_concat([b"x" * 1000, b"y" * 1000], preset=0)
    descs, keep, outs = lzma_amd._make_descs([lzma_amd.Stream(c, FMT_LZMA2_RAW, out_cap=2000, dict_size=4096)])
    descs[0].flags = 1
    res = (N.Result * 1)()
    assert N.lib().xlz_decode_batch_filtered(ctx._h, descs, 1, res, lzma_amd._make_steps([(0, R.X86, 0)]), 1, None, 0, None) == lzma_amd.ERR_BAD_ARG
    for mode in (2, -1):
        with pytest.raises(LzmaError) as e:
            ctx.set_filter_mode(mode)
        assert e.value.status == lzma_amd.ERR_BAD_ARG
    assert ctx.filter_mode() == 0


# ---- the container front-ends in filter mode 1 -------------------------------------------------------------------------
@pytest.fixture
def fmode1(ctx):
    ctx.set_filter_mode(1)
    assert ctx.filter_mode() == 1
    yield ctx
    ctx.set_filter_mode(0)
    ctx.set_check_mode(0)


L2 = {"id": lzma.FILTER_LZMA2, "preset": 1}


def _xz_blocks():
    code = R.machine_code(3 << 20, 0)
    blocks = [(code[: 1 << 20], [{"id": lzma.FILTER_X86}, L2]),
              (R.text(200_000), [L2]),
              (R.opcode_soup(150_000, 5), [{"id": lzma.FILTER_DELTA, "dist": 3}, {"id": lzma.FILTER_POWERPC, "start_offset": 8}, L2]),
              (b"", [{"id": lzma.FILTER_ARM}, L2]),
              (code[1 << 20: (1 << 20) + 70_001], [{"id": lzma.FILTER_SPARC}, {"id": lzma.FILTER_ARMTHUMB, "start_offset": 2}, {"id": lzma.FILTER_IA64}, L2])]
    for k, fid in enumerate(R.ALL):
        blocks.append((R.opcode_soup(40_000 + 1001 * k, 50 + k), [R.filter_dict(fid, R.params(fid)[1]), L2]))
    return blocks


def test_xz_front_end_with_filter_chains(ctx, fmode1):
    blocks = _xz_blocks()
    plain = b"".join(d for d, _ in blocks)
    files = [X.stream(blocks, check=lzma.CHECK_CRC64),
             X.stream(blocks[:3], check=lzma.CHECK_CRC32) + bytes(4) + X.stream(blocks[3:], check=lzma.CHECK_NONE),
             lzma.compress(blocks[0][0], format=lzma.FORMAT_XZ, filters=[{"id": lzma.FILTER_X86}, L2])]
    plains = [plain, plain, blocks[0][0]]
    for f, p in zip(files, plains):
        assert lzma.decompress(f.replace(bytes(4) + b"\xfd7zXZ", b"\xfd7zXZ")) == p   # (liblzma reads the same file)
        ctx.set_filter_mode(0)
        for fn in (lzma_amd.xz_decode, lzma_amd.xz_index):
            with pytest.raises(LzmaError) as e:
                fn(*((ctx, f) if fn is lzma_amd.xz_decode else (f,)))
            assert e.value.status == lzma_amd.ERR_UNSUPPORTED
        ctx.set_filter_mode(1)
        got_blocks, steps, _ = lzma_amd.xz_index_chains(f)
        for cmode in (0, 1):
            ctx.set_check_mode(cmode)
            assert lzma_amd.xz_decode(ctx, f, verify=True) == p
            st = ctx.last_filter_stats()
            n_empty = sum(1 for k, _, _ in steps if got_blocks[k]["uncomp_len"] == 0)
            assert st["device_steps"] == len(steps) - n_empty and st["host_steps"] == 0 and st["empty_steps"] == n_empty, st
            assert st["device_bytes"] == sum(got_blocks[k]["uncomp_len"] for k, _, _ in steps), st
            if cmode == 1:
                c = ctx.last_check_stats()
                assert c["device_ranges"] == sum(1 for b in got_blocks if b["check_type"] in (1, 4) and b["uncomp_len"]), c
            # a flipped check of a filtered block, a flipped payload byte of one
            hit = [k for k, _, _ in steps if got_blocks[k]["check_type"] in (1, 4) and got_blocks[k]["uncomp_len"]]
            if hit:
                bad = bytearray(f)
                bad[got_blocks[hit[0]]["check_off"]] ^= 0x40
                with pytest.raises(LzmaError) as e:
                    lzma_amd.xz_decode(ctx, bytes(bad))
                assert e.value.status == lzma_amd.ERR_RESULT
                assert lzma_amd.xz_decode(ctx, bytes(bad), verify=False) == p
                bad = bytearray(f)
                bad[got_blocks[hit[0]]["comp_off"] + 40] ^= 0x10
                with pytest.raises(LzmaError) as e:
                    lzma_amd.xz_decode(ctx, bytes(bad))
                assert e.value.status == lzma_amd.ERR_RESULT
    # a file without chains is decoded as ever in mode 1, and the _multi form keeps refusing chains
    ctx.set_check_mode(0)
    plain_xz = lzma.compress(plain, format=lzma.FORMAT_XZ)
    assert lzma_amd.xz_decode(ctx, plain_xz) == plain
    assert ctx.last_filter_stats()["device_steps"] == 0
    with pytest.raises(LzmaError) as e:
        lzma_amd.xz_decode_on([ctx], files[0])
    assert e.value.status == lzma_amd.ERR_UNSUPPORTED


def test_7z_front_end_with_filter_chains(ctx, fmode1):
    from sevenzip_craft import lzma_folder, copy_folder
    from test_filter_chains_cpu import FILTER_SETS
    code = R.machine_code(2 << 20, 1)
    folders, want = [], b""
    for k, fl in enumerate(FILTER_SETS):
        data = code[k * 1000: k * 1000 + 300_000] if k % 2 else R.opcode_soup(120_000 + k, 70 + k)
        rec, packed, nc = Z.chain_folder(data, fl, lzma2=bool(k & 1), lzma_first=bool(k & 2))
        files = [data[:5000], data[5000:5000], data[5000:]]   # (a solid folder: three files, one of them empty)
        folders.append((rec, packed, nc, files))
        want += data
    rec, packed = lzma_folder(R.text(50_000))
    folders.append((rec, packed, 1, [R.text(50_000)]))
    want += R.text(50_000)
    rec, packed = copy_folder(b"copy")
    folders.append((rec, packed, 1, [b"copy"]))
    want += b"copy"
    n_steps = sum(len(fl) for fl in FILTER_SETS)
    for folder_crc in (True, False):
        a = Z.archive(folders, folder_crc=folder_crc)
        ctx.set_filter_mode(0)
        with pytest.raises(LzmaError) as e:
            lzma_amd.sevenzip_decode(ctx, a)
        assert e.value.status == lzma_amd.ERR_UNSUPPORTED
        ctx.set_filter_mode(1)
        fo, _, steps, total = lzma_amd.sevenzip_index_chains(a)
        assert len(steps) == n_steps and total == len(want)
        for cmode in (0, 1):
            ctx.set_check_mode(cmode)
            assert lzma_amd.sevenzip_decode(ctx, a, verify=True) == want
            st = ctx.last_filter_stats()
            assert st["device_steps"] == n_steps and st["host_steps"] == 0 and st["empty_steps"] == 0, st
            if cmode == 1:
                assert ctx.last_check_stats()["device_ranges"] >= 2 * len(FILTER_SETS), ctx.last_check_stats()
            # a flipped payload byte in a chain folder is never silent; a flipped CRC is refused and passes unverified
            bad = bytearray(a)
            bad[fo[0]["pack_off"] + 40] ^= 0x10
            with pytest.raises(LzmaError) as e:
                lzma_amd.sevenzip_decode(ctx, bytes(bad))
            assert e.value.status == lzma_amd.ERR_RESULT
            at = a.rindex(struct.pack("<I", zlib.crc32(folders[0][3][0]) if not folder_crc else zlib.crc32(b"".join(folders[0][3]))))
            hdr_at = 32 + struct.unpack("<Q", a[12:20])[0]
            assert at >= hdr_at
            nh = bytearray(a[hdr_at:])
            nh[at - hdr_at] ^= 1
            start = struct.pack("<QQI", hdr_at - 32, len(nh), zlib.crc32(bytes(nh)))
            bad = a[:8] + struct.pack("<I", zlib.crc32(start)) + start + a[32:hdr_at] + bytes(nh)
            with pytest.raises(LzmaError) as e:
                lzma_amd.sevenzip_decode(ctx, bad)
            assert e.value.status == lzma_amd.ERR_RESULT
            assert lzma_amd.sevenzip_decode(ctx, bad, verify=False) == want
