"""GPU: CRC32 / CRC64 computed on the device next to the decode (lzma_amd/csrc/xlz_check_dev.hip) -- Batch.checks on a
device-resident batch, decode_batch_checked in the three forms of the host pipeline, and the container front-ends in
check mode 1.  Everything is bit-exact: expected digests are zlib's CRC32 and liblzma's CRC64 (tests/check_ref.py) over
the ORACLE's bytes, and Context.last_check_stats must show that the device did the work."""
import ctypes
import lzma
import random
import shutil
import struct
import zlib

import numpy as np
import pytest

import check_ref
import corpus
import lzma_amd
import pipeline_streams as ps
from check_ref import CRC32, CRC64
from lzma_amd import FMT_LZMA_ALONE, LzmaError
from lzma_amd import _native as N

pytestmark = pytest.mark.gpu

SEG = 128 << 10  # xlzchk::kSegBytes (lzma_amd/csrc/xlz_check_dev.h): one wave's share of a range


def _expect(kind, data, off, length, out_len):
    lo, hi = min(off, out_len), min(off + length, out_len)
    return check_ref.digest(kind, data[lo:hi])


def test_checks_on_a_device_resident_batch(ctx):
    """Outputs of 0 bytes to 20 MiB (an LZMA2 stream of many units), a cut and a bit-flipped stream; whole-stream ranges
    (longer than the output: cut to out_len) and ranges with odd offsets and lengths, several per stream, both kinds, in
    shuffled order; a range behind the output is the CRC of nothing.  Only digests leave the device."""
    rnd = random.Random(7007)
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
        for kind in (CRC32, CRC64):
            ranges.append((i, 0, s.out_cap + 100, kind))
            ranges.append((i, n + 5, 10, kind))
        ranges.append((i, 3, max(n - 7, 0), CRC32 if i % 2 else CRC64))
        ranges.append((i, (n // 3) | 1, n // 2, CRC64 if i % 2 else CRC32))
        ranges.append((i, max(n - 1, 0), 1 << 62, CRC32))
        if n > 2 * SEG:
            ranges.append((i, SEG - 1, SEG + 2, CRC64))
            ranges.append((i, 17, 2 * SEG - 17, CRC32))
    assert jobs[-1][1]()[0] != jobs[-2][1]()[0] and 0 < len(jobs[-1][1]()[0]) < 400_000   # (the damaged ones did stop short)
    rnd.shuffle(ranges)
    for run in range(2):   # (the second call finds the batch's check buffers)
        got = b.checks(ranges)
        for (i, off, length, kind), g in zip(ranges, got):
            w = jobs[i][1]()[0]
            want = _expect(kind, w, off, length, len(w))
            print("stream %d off %d len %d kind %d: %016x want %016x" % (i, off, length, kind, g, want))
            assert g == want, (i, off, length, kind, hex(g), hex(want))
        st = ctx.last_check_stats()
        n_empty = sum(1 for i, off, length, _ in ranges if min(off + length, len(jobs[i][1]()[0])) <= min(off, len(jobs[i][1]()[0])))
        assert st["host_ranges"] == 0 and st["empty_ranges"] == n_empty and st["device_ranges"] == len(ranges) - n_empty, st
        assert st["launches"] == 1 and st["kernel_ms"] > 0 and st["device_bytes"] > 40 << 20, st
    # the bytes are still where they were, and a bad range fails the call
    assert b.download(15, 1 << 20) == jobs[15][1]()[0]
    for bad in ((len(jobs), 0, 1, CRC32), (0, 0, 1, 2), (0, 0, 1, 10)):
        with pytest.raises(LzmaError) as e:
            b.checks([bad])
        assert e.value.status == lzma_amd.ERR_BAD_ARG
    assert b.checks([]) == []
    b.close()


def _flat_call_checked(ctx, streams, ranges):
    """pipeline_streams.flat_call through xlz_decode_batch_checked -> (status, out, offsets, results, digests)"""
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
    st = N.lib().xlz_decode_batch_checked(ctx._h, descs, n, res, arr, len(ranges), dig.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
    return st, out, offs, [(r.out_len, r.status, r.in_consumed) for r in res], dig


def _whole_output_digests_match(jobs, kinds, dig):
    """indices of the streams whose whole-output digest differs from the CRC of the oracle's bytes (streams repeated in a
    corpus share one oracle result and one expected digest per kind)"""
    memo, bad = {}, []
    for i, (_, want) in enumerate(jobs):
        key = (id(want), kinds[i])
        if key not in memo:
            memo[key] = check_ref.digest(kinds[i], want()[0])
        if int(dig[i]) != memo[key]:
            bad.append(i)
    return bad


def _check_pipeline(ctx, jobs, stats_want):
    """one checked call over `jobs`, a whole-output range per stream (CRC32 on even streams, CRC64 on odd ones, longer than
    the output): bytes, status and in_consumed against the oracle as tests/test_gpu_pipeline.py demands, every digest
    against the CRC of the oracle's bytes, and nothing checked on the host"""
    kinds = [CRC64 if i % 2 else CRC32 for i in range(len(jobs))]
    ranges = [(i, 0, j[0].out_cap + 1, kinds[i]) for i, j in enumerate(jobs)]
    st, out, offs, res, dig = _flat_call_checked(ctx, [j[0] for j in jobs], ranges)
    assert st == 0
    s = ctx.last_call_stats()
    for k, v in stats_want.items():
        assert s[k] == v, s
    bad = ps.flat_mismatches(jobs, out, offs, res)
    assert bad == [], "%d streams differ from the oracle, first %s" % (len(bad), bad[:10])
    bad = _whole_output_digests_match(jobs, kinds, dig)
    assert bad == [], "%d digests differ from the CRC of the oracle's bytes, first %s" % (len(bad), bad[:10])
    c = ctx.last_check_stats()
    n_empty = sum(1 for r in res if r[0] == 0)
    print("check stats:", c, "call stats:", s)
    assert c["host_ranges"] == 0 and c["empty_ranges"] == n_empty and c["device_ranges"] == len(jobs) - n_empty, c
    assert c["device_bytes"] == sum(r[0] for r in res) and c["kernel_ms"] > 0, c
    return s, c


def test_checked_call_of_one_sliced_piece(ctx):
    """Mode 0, three slices over the mixed-kind set among 1200 streams of 256 KiB: it holds streams that collect() decodes
    again after their slices went out (exact re-runs, models beyond LDS) -- a check queued before that reads stale bytes"""
    mixed = ps.mixed_kind_jobs()
    fill = [ps.alone_job(corpus.compress_alone(corpus.plain("TMZR"[d % 4], 95_800 + d, 256 << 10), preset=0), 256 << 10)
            for d in range(24)]
    jobs = [fill[i % 24] for i in range(1200 + len(mixed))]
    for k, j in enumerate(mixed):
        jobs[k * len(jobs) // len(mixed)] = j
    assert lzma_amd.decode_batch_plan([j[0].out_cap for j in jobs])[1] == 0
    ctx.set_slicing(1, 1 << 20, 3)
    try:
        for run in range(2):
            s, c = _check_pipeline(ctx, jobs, {"slices": 3, "sub_batches": 1})
            assert s["refetched"] >= ps.MIXED_REFETCHED_AT_LEAST and c["launches"] == 1, (s, c)
    finally:
        ctx.set_slicing(0, 0, 0)


def test_checked_call_of_overlapping_pieces(ctx):
    """Mode 1: 16 384 streams of 32-128 KiB from 48 plaintexts, a special stream of every kind at the edges of and inside
    every piece (tests/test_gpu_pipeline.py's shape); the digests of piece k are fetched while piece k + 1 decodes"""
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
    for run in range(2):
        s, c = _check_pipeline(ctx, jobs, {"sub_batches": len(cuts) - 1, "streams": n})
        assert c["launches"] == len(cuts) - 1, c


def test_checked_call_of_one_round_pieces(ctx):
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
    s, c = _check_pipeline(ctx, jobs, {"sub_batches": 3, "streams": n})
    assert c["launches"] == 3, c


def test_checked_call_argument_errors(ctx):
    s = lzma_amd.Stream(corpus.compress_alone(b"abc" * 100, preset=0), out_cap=300)
    for bad in ((1, 0, 1, CRC32), (0, 0, 1, 3)):
        with pytest.raises(LzmaError) as e:
            lzma_amd.decode_batch_checked(ctx, [s], [bad])
        assert e.value.status == lzma_amd.ERR_BAD_ARG
    got, dig = lzma_amd.decode_batch_checked(ctx, [s, s], [(1, 1, 298, CRC64), (0, 0, 300, CRC32), (0, 300, 5, CRC32)])
    assert got[0][0] == got[1][0] == b"abc" * 100
    assert dig == [check_ref.crc64((b"abc" * 100)[1:299]), zlib.crc32(b"abc" * 100), 0]


# ---- the container front-ends in check mode 1 -------------------------------------------------------------------------
@pytest.fixture
def mode1(ctx):
    ctx.set_check_mode(1)
    assert ctx.check_mode() == 1
    yield ctx
    ctx.set_check_mode(0)


def _xz_files():
    from test_xz_container import _three_streams
    files = [_three_streams()]
    p = corpus.plain("M", 8, 1_000_000)
    if shutil.which("xz"):
        import subprocess
        for bs in (131072, 65536):
            files.append((subprocess.run(["xz", "-c", "-T2", "--block-size=%d" % bs], input=p, capture_output=True, check=True).stdout, p))
    else:   # (no xz tool: a file of many one-block streams has as many blocks)
        files.append((b"".join(lzma.compress(p[o:o + 131072], format=lzma.FORMAT_XZ, check=lzma.CHECK_CRC64) for o in range(0, len(p), 131072)), p))
    return files


def test_xz_front_end_checks_on_the_device(ctx, mode1):
    for f, p in _xz_files():
        blocks, _ = lzma_amd.xz_index(f)
        ctx.set_check_mode(0)
        assert lzma_amd.xz_decode(ctx, f) == p
        ctx.set_check_mode(1)
        assert lzma_amd.xz_decode(ctx, f) == p
        c = ctx.last_check_stats()
        n_dev = sum(1 for b in blocks if b["check_type"] in (1, 4))
        n_sha = sum(1 for b in blocks if b["check_type"] == 10)
        assert (c["device_ranges"], c["host_ranges"], c["empty_ranges"]) == (n_dev, n_sha, 0) and n_dev > 0, c
        assert c["device_bytes"] == sum(b["uncomp_len"] for b in blocks if b["check_type"] in (1, 4)), c
        # a flipped check field (of every device-checked kind in the file) is refused as in mode 0 and passes unverified;
        # a flipped payload byte is never silent
        for kind in (1, 4):
            hit = [b for b in blocks if b["check_type"] == kind]
            if not hit:
                continue
            bad = bytearray(f)
            bad[hit[len(hit) // 2]["check_off"]] ^= 0x40
            st = []
            for mode in (0, 1):
                ctx.set_check_mode(mode)
                with pytest.raises(LzmaError) as e:
                    lzma_amd.xz_decode(ctx, bytes(bad))
                st.append(e.value.status)
                assert lzma_amd.xz_decode(ctx, bytes(bad), verify=False) == p
            assert st[0] == st[1] == lzma_amd.ERR_RESULT, st
        bad = bytearray(f)
        bad[blocks[len(blocks) // 2]["comp_off"] + 40] ^= 0x10
        st = []
        for mode in (0, 1):
            ctx.set_check_mode(mode)
            with pytest.raises(LzmaError) as e:
                lzma_amd.xz_decode(ctx, bytes(bad))
            st.append(e.value.status)
        assert st[0] == st[1], st
    ctx.set_check_mode(1)
    assert lzma_amd.xz_decode(ctx, lzma.compress(b"", format=lzma.FORMAT_XZ)) == b""


def _rewrite_7z_header(a, edit):
    """the archive `a` (plain header) with its header bytes passed through edit(bytearray) and the CRCs made right again"""
    hdr_at = 32 + struct.unpack("<Q", bytes(a[12:20]))[0]
    nh = bytearray(a[hdr_at:])
    edit(nh)
    start = struct.pack("<QQI", hdr_at - 32, len(nh), zlib.crc32(bytes(nh)))
    return bytes(a[:8]) + struct.pack("<I", zlib.crc32(start)) + start + bytes(a[32:hdr_at]) + bytes(nh)


def test_7z_front_end_checks_on_the_device(ctx, mode1):
    import hashlib
    from sevenzip_craft import archive
    from test_7z_container import _folders, _golden_libarchive
    fo, want = _folders()
    for enc in (False, True):
        a = archive(fo, encoded_header=enc)
        ctx.set_check_mode(0)
        assert lzma_amd.sevenzip_decode(ctx, a) == want
        ctx.set_check_mode(1)
        assert lzma_amd.sevenzip_decode(ctx, a) == want
        c = ctx.last_check_stats()
        # files with a CRC in the three folders the device decodes: four (one of them empty) + one + one; the Copy
        # folder's file on the host; the encoded header is one more folder with a CRC of its own
        assert (c["empty_ranges"], c["host_ranges"], c["host_bytes"]) == (1, 1, 4) and c["device_ranges"] >= 5 + enc, c
    # folder CRCs instead of per-file ones
    a = archive([fo[1], fo[3]], with_substreams=False, folder_crc=True)
    assert lzma_amd.sevenzip_decode(ctx, a) == fo[1][2][0] + fo[3][2][0]
    c = ctx.last_check_stats()
    assert c["device_ranges"] >= 2 and c["host_ranges"] == 0, c
    # a flipped per-file CRC: refused with the same status as in mode 0, passes with verify=False
    bad = _rewrite_7z_header(bytearray(archive(fo)), lambda nh: nh.__setitem__(len(nh) - 20, nh[-20] ^ 1))
    st = []
    for mode in (0, 1):
        ctx.set_check_mode(mode)
        with pytest.raises(LzmaError) as e:
            lzma_amd.sevenzip_decode(ctx, bad)
        st.append(e.value.status)
        assert lzma_amd.sevenzip_decode(ctx, bad, verify=False) == want
    assert st[0] == st[1] == lzma_amd.ERR_RESULT, st
    # a flipped payload byte is never silent
    dmg = bytearray(archive(fo))
    dmg[40] ^= 0xFF
    for mode in (0, 1):
        ctx.set_check_mode(mode)
        with pytest.raises(LzmaError):
            lzma_amd.sevenzip_decode(ctx, bytes(dmg))
    # the archive libarchive wrote: a solid LZMA folder, per-file CRCs, an LZMA-encoded header
    ctx.set_check_mode(1)
    g, exp = _golden_libarchive()
    assert hashlib.sha256(lzma_amd.sevenzip_decode(ctx, g, verify=True)).hexdigest() == exp["sha256"]
    c = ctx.last_check_stats()
    n_files = sum(1 for size, _ in exp["substreams"])
    assert c["host_ranges"] == 0 and c["device_ranges"] + c["empty_ranges"] >= n_files and c["device_ranges"] >= 2, c
    assert c["device_bytes"] >= exp["folder"]["unpack_size"], c
    dmg = bytearray(g)
    dmg[exp["folder"]["pack_off"] + exp["folder"]["pack_len"] // 2] ^= 0x20
    with pytest.raises(LzmaError):
        lzma_amd.sevenzip_decode(ctx, bytes(dmg), verify=True)
