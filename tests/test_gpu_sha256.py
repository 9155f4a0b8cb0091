"""GPU: SHA-256 of decoded ranges computed on the device, one lane per range (lzma_amd/csrc/xlz_sha256_dev.hip) --
Batch.digests on a device-resident batch, decode_batch_digests in the three forms of the host pipeline and with filter
steps, and the .xz front-end in check mode 2.  Expected digests are hashlib's SHA-256, zlib's CRC32 and liblzma's CRC64
over the ORACLE's bytes, never the library's own host code; who hashed what must be what sha256_plan says for the ranges
of every (sub-)batch: the plan sends long or few ranges to the host threads, so both sides are exercised here.

Times: a lane hashes some 20 MB/s (the instruction-count estimate of lzma_amd/csrc/xlz_sha256_dev.h), and no range the device
gets here is longer than 16 MiB (the plan's own cap is lower): no launch of this file runs longer than a second."""
import ctypes
import hashlib
import lzma
import random

import numpy as np
import pytest

import check_ref
import corpus
import lzma_amd
import pipeline_streams as ps
from check_ref import CRC32, CRC64
from lzma_amd import CHECK_SHA256 as SHA
from lzma_amd import FMT_LZMA2_RAW, FMT_LZMA_ALONE, LzmaError
from lzma_amd import _native as N

pytestmark = pytest.mark.gpu

SEG = 128 << 10
MAX_DEVICE_RANGE = 16 << 20


def _digest(kind, data):
    return hashlib.sha256(data).digest() if kind == SHA else check_ref.digest(kind, data)


def _cut(off, length, out_len):
    return min(off, out_len), min(off + length, out_len)


def _planned(lens):
    """how many of these (non-empty, in-arena) SHA-256 ranges of one (sub-)batch the built-in plan gives the device"""
    on = lzma_amd.sha256_plan(lens)
    assert all(n <= MAX_DEVICE_RANGE for n, d in zip(lens, on) if d)
    return sum(on), sum(n for n, d in zip(lens, on) if d)


def test_digests_on_a_device_resident_batch(ctx):
    """The stream set of test_gpu_checks.test_checks_on_a_device_resident_batch: outputs of 0 bytes to 20 MiB, a cut and a
    bit-flipped stream.  Whole-stream ranges (longer than the output), ranges with odd offsets and lengths, several per
    stream, a few hundred short ones at every start alignment, the three kinds mixed in one call in shuffled order."""
    rnd = random.Random(7117)
    sizes = [0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, SEG - 1, SEG, SEG + 1, 2 * SEG + 77, 1 << 20]
    jobs = [ps.alone_job(corpus.compress_alone(corpus.plain("TRMZ"[i % 4], 97_000 + i, n), preset=0), n) for i, n in enumerate(sizes)]
    big = [corpus.plain("TMZ"[k % 3], 97_100 + k, 1 << 20) for k in range(20)] + [corpus.plain("R", 97_130, 300_001)]
    jobs.append(ps.raw2_job(corpus.lzma2_concat(big, preset=0), sum(map(len, big))))
    good = corpus.compress_alone(corpus.plain("M", 97_200, 400_000), preset=0)
    flip = bytearray(good)
    flip[13 + (len(good) - 13) // 2] ^= 0x04
    jobs.append(ps.alone_job(bytes(flip), 400_000))
    jobs.append(ps.alone_job(good[: 13 + (len(good) - 13) * 2 // 3], 400_000))
    b = lzma_amd.Batch(ctx, [j[0] for j in jobs])
    b.run()
    res = b.results()
    ranges = []
    for i, (s, want) in enumerate(jobs):
        w, w_st, w_in = want()
        assert res[i] == (len(w), w_st, w_in), (i, res[i])
        n = len(w)
        for kind in (CRC32, CRC64, SHA):
            ranges.append((i, 0, s.out_cap + 100, kind))
            ranges.append((i, n + 5, 10, kind))
        ranges.append((i, 3, max(n - 7, 0), SHA))
        ranges.append((i, (n // 3) | 1, n // 2, (CRC32, CRC64, SHA)[i % 3]))
        ranges.append((i, max(n - 1, 0), 1 << 62, SHA))
        if n > 2 * SEG:
            ranges.append((i, SEG - 1, SEG + 2, SHA))
            ranges.append((i, 17, 2 * SEG - 17, CRC32))
    # short ranges at every alignment and around the padding's corners, in the 1 MiB stream and the 20 MiB one
    for k in range(400):
        i = 15 if k % 2 else 16
        n = len(jobs[i][1]()[0])
        length = (0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128)[k % 11] + 64 * rnd.randrange(0, 80)
        ranges.append((i, rnd.randrange(0, n - length), length, SHA))
    ranges.append((16, len(jobs[16][1]()[0]) - 4099, 4099, SHA))   # (ends where its stream ends)
    ranges.append((18, 1, 1 << 40, SHA))
    rnd.shuffle(ranges)
    lens = []
    n_empty = n_sha_empty = 0
    for i, off, length, kind in ranges:
        lo, hi = _cut(off, length, len(jobs[i][1]()[0]))
        n_empty += hi <= lo
        n_sha_empty += hi <= lo and kind == SHA
        if kind == SHA and hi > lo:
            lens.append(hi - lo)
    n_dev, dev_bytes = _planned(lens)
    assert 0 < n_dev < len(lens)   # (both sides get work: the 20 MiB ranges are the host's, the short ones the device's)
    for run in range(2):   # (the second call finds the batch's buffers)
        got = b.digests(ranges)
        for (i, off, length, kind), g in zip(ranges, got):
            w = jobs[i][1]()[0]
            lo, hi = _cut(off, length, len(w))
            want = _digest(kind, w[lo:hi])
            assert g == want, (i, off, length, kind, g, want)
        st, c = ctx.last_sha256_stats(), ctx.last_check_stats()
        print("sha256 stats:", st, "check stats:", c)
        assert (st["device_ranges"], st["device_bytes"]) == (n_dev, dev_bytes), st
        assert (st["host_ranges"], st["host_bytes"]) == (len(lens) - n_dev, sum(lens) - dev_bytes), st
        assert st["empty_ranges"] == n_sha_empty and st["launches"] == 1 and st["kernel_ms"] > 0 and st["threshold"] > 0, st
        n_crc = sum(1 for r in ranges if r[3] != SHA)
        assert c["empty_ranges"] == n_empty and c["device_ranges"] + c["host_ranges"] == len(ranges) - n_empty, c
        assert c["host_ranges"] == st["host_ranges"] and c["device_ranges"] == st["device_ranges"] + n_crc - (n_empty - n_sha_empty), c
    # the bytes are still where they were; the older call refuses the new kind, the new one refuses bad ranges
    assert b.download(15, 1 << 20) == jobs[15][1]()[0]
    assert b.digests([(0, 0, 5, SHA), (0, 0, 5, CRC32), (0, 0, 5, CRC64)]) == [hashlib.sha256(b"").digest(), 0, 0]
    for bad in ((len(jobs), 0, 1, SHA), (0, 0, 1, 2), (0, 0, 1, 11)):
        with pytest.raises(LzmaError) as e:
            b.digests([bad])
        assert e.value.status == lzma_amd.ERR_BAD_ARG
    with pytest.raises(LzmaError) as e:
        b.checks([(0, 0, 1, SHA)])
    assert e.value.status == lzma_amd.ERR_BAD_ARG
    assert b.digests([]) == []
    b.close()


def _flat_call_digests(ctx, streams, steps, ranges):
    """pipeline_streams.flat_call through xlz_decode_batch_digests -> (status, out, offsets, results, xlz_digest array)"""
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
    dig = np.zeros((max(len(ranges), 1), 32), dtype=np.uint8)
    st = N.lib().xlz_decode_batch_digests(ctx._h, descs, n, res, lzma_amd._make_steps(steps), len(steps), arr, len(ranges),
                                          dig.ctypes.data_as(ctypes.POINTER(N.Digest)))
    return st, out, offs, [(r.out_len, r.status, r.in_consumed) for r in res], dig


def _digest_pipeline(ctx, jobs, stats_want):
    """one call over `jobs`, a whole-output range per stream (longer than the output), kinds CRC32 / CRC64 / SHA-256 in turn:
    bytes, status and in_consumed against the oracle, every digest against the digest of the oracle's bytes, and the
    SHA-256 ranges split between device and host as the plan splits the ranges of every piece"""
    kinds = [(CRC32, CRC64, SHA)[i % 3] for i in range(len(jobs))]
    ranges = [(i, 0, j[0].out_cap + 1, kinds[i]) for i, j in enumerate(jobs)]
    st, out, offs, res, dig = _flat_call_digests(ctx, [j[0] for j in jobs], [], ranges)
    assert st == 0
    s = ctx.last_call_stats()
    for k, v in stats_want.items():
        assert s[k] == v, s
    bad = ps.flat_mismatches(jobs, out, offs, res)
    assert bad == [], "%d streams differ from the oracle, first %s" % (len(bad), bad[:10])
    memo, bad = {}, []
    for i, (_, want) in enumerate(jobs):
        key = (id(want), kinds[i])
        if key not in memo:
            d = _digest(kinds[i], want()[0])
            memo[key] = d if kinds[i] == SHA else int(d).to_bytes(8, "little") + bytes(24)
        if bytes(dig[i]) != memo[key]:
            bad.append(i)
    assert bad == [], "%d digests differ from the digest of the oracle's bytes, first %s" % (len(bad), bad[:10])
    c, h = ctx.last_check_stats(), ctx.last_sha256_stats()
    print("check stats:", c, "sha256 stats:", h, "call stats:", s)
    cuts, _ = lzma_amd.decode_batch_plan([j[0].out_cap for j in jobs])
    n_dev = dev_bytes = 0
    for a, b in zip(cuts, cuts[1:]):
        nd, db = _planned([res[i][0] for i in range(a, b) if kinds[i] == SHA and res[i][0]])
        n_dev, dev_bytes = n_dev + nd, dev_bytes + db
    n_sha = sum(1 for i in range(len(jobs)) if kinds[i] == SHA and res[i][0])
    sha_bytes = sum(res[i][0] for i in range(len(jobs)) if kinds[i] == SHA)
    assert (h["device_ranges"], h["device_bytes"]) == (n_dev, dev_bytes) and n_dev > 0 and h["kernel_ms"] > 0, h
    assert (h["host_ranges"], h["host_bytes"]) == (n_sha - n_dev, sha_bytes - dev_bytes), h
    n_empty = sum(1 for r in res if r[0] == 0)
    assert c["empty_ranges"] == n_empty and c["device_ranges"] + c["host_ranges"] == len(jobs) - n_empty, c
    assert c["host_ranges"] == h["host_ranges"] and c["device_bytes"] + c["host_bytes"] == sum(r[0] for r in res), c
    return s, c, h


def test_digest_call_of_one_sliced_piece(ctx):
    """Mode 0, three slices over the mixed-kind set among 1200 streams of 256 KiB: the set holds streams that collect()
    decodes again after their slices went out -- a hash queued before that reads stale bytes"""
    mixed = ps.mixed_kind_jobs()
    fill = [ps.alone_job(corpus.compress_alone(corpus.plain("TMZR"[d % 4], 95_800 + d, 256 << 10), preset=0), 256 << 10)
            for d in range(24)]
    jobs = [fill[i % 24] for i in range(1200 + len(mixed))]
    for k, j in enumerate(mixed):
        jobs[k * len(jobs) // len(mixed)] = j
    assert lzma_amd.decode_batch_plan([j[0].out_cap for j in jobs])[1] == 0
    ctx.set_slicing(1, 1 << 20, 3)
    try:
        s, c, h = _digest_pipeline(ctx, jobs, {"slices": 3, "sub_batches": 1})
        assert s["refetched"] >= ps.MIXED_REFETCHED_AT_LEAST and h["launches"] == 1, (s, h)
    finally:
        ctx.set_slicing(0, 0, 0)


def test_digest_call_of_overlapping_pieces(ctx):
    """Mode 1: 16 384 streams of 32-128 KiB from 48 plaintexts, a special stream of every kind at the edges of and inside
    every piece (tests/test_gpu_checks.py's shape)"""
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
        at |= {a, b - 1, a + 1, b - 2} | {a + (b - a) * q // 7 for q in range(1, 7)}
    at |= set(range(333, n, 2011))
    rnd = random.Random(6006)
    for k, i in enumerate(sorted(at)):
        jobs[i] = _specials(rnd, jobs[i][0].out_cap, 94_000 + 10 * k)[k % 8]
    assert lzma_amd.decode_batch_plan([j[0].out_cap for j in jobs]) == (cuts, mode)
    s, c, h = _digest_pipeline(ctx, jobs, {"sub_batches": len(cuts) - 1, "streams": n})
    assert h["launches"] == len(cuts) - 1, h


def test_digest_call_of_one_round_pieces(ctx):
    """Mode 2: 8193 streams of 256 KiB and 300 KiB, LZMA1 and LZMA2 of 2-4 units, damaged streams at the pieces' edges"""
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
    for i in (4095, 4096, 8191, 8192):
        s, _ = jobs[i]
        c = bytearray(s.data)
        if i % 2:
            c[len(c) // 2] ^= 0x55
        else:
            del c[len(c) * 2 // 3:]
        jobs[i] = (ps.raw2_job if s.fmt != FMT_LZMA_ALONE else ps.alone_job)(bytes(c), s.out_cap)
    assert lzma_amd.decode_batch_plan([j[0].out_cap for j in jobs]) == ([0, 4096, 8192, 8193], 2)
    _digest_pipeline(ctx, jobs, {"sub_batches": 3, "streams": n})


def test_digest_call_with_filter_steps(ctx):
    """the digest is over the FILTERED bytes: 600 raw LZMA2 streams of opcode soup, an x86 and a Delta step on every other
    one; expected bytes are liblzma's own filters over the oracle's bytes"""
    import filter_ref as R
    plains = [R.opcode_soup(40_000 + 4001 * d, 300 + d) for d in range(12)]
    comps = [corpus.compress_raw_lzma2(p, dict_size=1 << 16, preset=0) for p in plains]
    n = 600
    streams = [lzma_amd.Stream(comps[i % 12], FMT_LZMA2_RAW, out_cap=len(plains[i % 12]), dict_size=1 << 16) for i in range(n)]
    chain = [(R.X86, 4096), (R.DELTA, 3)]
    steps = [(i, f, p) for i in range(0, n, 2) for f, p in chain]
    ranges = [(i, 0, 1 << 30, SHA) for i in range(n)] + [(i, 5, 1001, CRC32) for i in range(n)]
    got, dig = lzma_amd.decode_batch_digests(ctx, streams, ranges, steps)
    filtered = [R.apply_steps(chain, p) for p in plains]
    assert any(f != p for f, p in zip(filtered, plains))
    for i in range(n):
        w = filtered[i % 12] if i % 2 == 0 else plains[i % 12]
        assert got[i][0] == w and got[i][1] >= 0, i
        assert dig[i] == hashlib.sha256(w).digest(), i
        assert dig[n + i] == check_ref.crc32(w[5:1006]), i
    h = ctx.last_sha256_stats()
    n_dev, dev_bytes = _planned([len(plains[i % 12]) for i in range(n)])
    assert (h["device_ranges"], h["device_bytes"]) == (n_dev, dev_bytes) and n_dev > 0, h
    assert ctx.last_filter_stats()["device_steps"] == len(steps)
    # argument errors
    for bad in ((n, 0, 1, SHA), (0, 0, 1, 3)):
        with pytest.raises(LzmaError) as e:
            lzma_amd.decode_batch_digests(ctx, streams[:2], [bad])
        assert e.value.status == lzma_amd.ERR_BAD_ARG
    with pytest.raises(LzmaError) as e:
        lzma_amd.decode_batch_checked(ctx, streams[:2], [(0, 0, 1, SHA)])
    assert e.value.status == lzma_amd.ERR_BAD_ARG


# ---- the .xz front-end in check mode 2 --------------------------------------------------------------------------------
def _sha_file(n_blocks, block_bytes, distinct=16):
    """n_blocks one-block .xz streams with a SHA-256 check, concatenated"""
    ps_ = [corpus.plain("TMZR"[d % 4], 98_000 + d, block_bytes) for d in range(min(distinct, n_blocks))]
    cs = [lzma.compress(p, format=lzma.FORMAT_XZ, check=lzma.CHECK_SHA256, preset=0) for p in ps_]
    return b"".join(cs[k % len(cs)] for k in range(n_blocks)), b"".join(ps_[k % len(ps_)] for k in range(n_blocks))


@pytest.fixture
def modes(ctx):
    yield ctx
    ctx.set_check_mode(0)


def _decode_in_modes(ctx, f, **kw):
    """xz_decode in modes 0, 1, 2 -> [bytes or the refusing status] per mode, and the statistics of the mode 2 call"""
    got = []
    for mode in (0, 1, 2):
        ctx.set_check_mode(mode)
        assert ctx.check_mode() == mode
        try:
            got.append(lzma_amd.xz_decode(ctx, f, **kw))
        except LzmaError as e:
            got.append(e.status)
    return got, ctx.last_sha256_stats(), ctx.last_check_stats()


def test_xz_front_end_hashes_on_the_device(ctx, modes):
    from test_xz_container import _three_streams
    for f, p in (_sha_file(64, 256 << 10), _sha_file(1024, 64 << 10), _three_streams()):
        blocks, _ = lzma_amd.xz_index(f)
        got, h, c = _decode_in_modes(ctx, f)
        assert got == [p, p, p]
        sha_lens = [b["uncomp_len"] for b in blocks if b["check_type"] == 10]
        n_crc = sum(1 for b in blocks if b["check_type"] in (1, 4))
        n_dev, dev_bytes = _planned(sha_lens)
        print("%d blocks: sha256 stats %s, check stats %s" % (len(blocks), h, c))
        assert (h["device_ranges"], h["device_bytes"], h["host_ranges"]) == (n_dev, dev_bytes, len(sha_lens) - n_dev), h
        assert (c["device_ranges"], c["host_ranges"], c["empty_ranges"]) == (n_crc + n_dev, len(sha_lens) - n_dev, 0), c
        if len(blocks) == 1024:
            assert n_dev == 1024 and h["kernel_ms"] > 0, h   # (a thousand short blocks: the device's, whatever the rates)
        # mode 1 keeps the SHA-256 blocks on the host
        ctx.set_check_mode(1)
        assert lzma_amd.xz_decode(ctx, f) == p
        c1 = ctx.last_check_stats()
        assert (c1["device_ranges"], c1["host_ranges"]) == (n_crc, len(sha_lens)), c1
        # a flipped byte of a stored SHA-256: refused alike in all modes, passes unverified; a flipped payload byte too
        hit = [b for b in blocks if b["check_type"] == 10]
        bad = bytearray(f)
        bad[hit[len(hit) // 2]["check_off"] + 13] ^= 0x40
        got, _, _ = _decode_in_modes(ctx, bytes(bad))
        assert got == [lzma_amd.ERR_RESULT] * 3, got
        got, _, _ = _decode_in_modes(ctx, bytes(bad), verify=False)
        assert got == [p, p, p]
        bad = bytearray(f)
        bad[hit[len(hit) // 2]["comp_off"] + 40] ^= 0x10
        got, _, _ = _decode_in_modes(ctx, bytes(bad))
        assert got[0] == got[1] == got[2] and isinstance(got[0], int) and got[0] < 0, got


def test_xz_front_end_leaves_few_long_blocks_to_the_host(ctx, modes):
    f, p = _sha_file(4, 8 << 20, distinct=1)
    got, h, c = _decode_in_modes(ctx, f)
    assert got == [p, p, p]
    assert (h["device_ranges"], h["host_ranges"], h["host_bytes"], h["launches"]) == (0, 4, 32 << 20, 0), h
    assert (c["device_ranges"], c["host_ranges"]) == (0, 4), c
    bad = bytearray(f)
    bad[lzma_amd.xz_index(f)[0][2]["check_off"]] ^= 1
    got, _, _ = _decode_in_modes(ctx, bytes(bad))
    assert got == [lzma_amd.ERR_RESULT] * 3, got


def test_xz_front_end_empty_file(ctx, modes):
    f = lzma.compress(b"", format=lzma.FORMAT_XZ, check=lzma.CHECK_SHA256)
    got, h, _ = _decode_in_modes(ctx, f)
    assert got == [b"", b"", b""] and h["device_ranges"] == h["host_ranges"] == 0
