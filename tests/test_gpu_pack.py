"""GPU: decoded bytes packed into the caller's device memory (lzma_amd/csrc/xlz_pack_dev.hip) -- Batch.pack on a
device-resident batch, and the container front-ends xz_decode_device / sevenzip_decode_device / *_decode_tensor, which
decode, filter, check and pack without the bytes leaving the device.  Everything is bit-exact.  The judge of the bytes
is liblzma; the judge of status, size and unverified count is the host-destination form on the same context."""
import ctypes
import json
import lzma
import os
import random
import zlib

import pytest

import corpus
import filter_ref as R
import lzma_amd
import sevenzip_chains as Z
import sevenzip_craft as C
import xz_chains as X
from lzma_amd import FMT_LZMA2_RAW, LzmaError
from lzma_amd import _native as N
from pack_edges import FILL, expect_pack

pytestmark = pytest.mark.gpu

DICT = 1 << 16
SIZES = ([0] + list(range(1, 19)) + [31, 33, 255, 256, 257] + list(range(4095, 4102)) + list(range(16379, 16390)) +
         list(range(65531, 65542)) + [(1 << 20) + 16385, 3_000_001])
L2 = {"id": lzma.FILTER_LZMA2}


def _torch():
    import torch
    return torch


def _filled(n):
    torch = _torch()
    t = torch.full((max(n, 1),), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _raw_lzma2(plain):
    segs = [plain[o:o + (1 << 20)] for o in range(0, len(plain), 1 << 20)] or [b""]
    return corpus.lzma2_concat(segs, dict_size=DICT, preset=0)


@pytest.fixture(scope="module")
def streams300():
    """about 300 raw LZMA2 streams of the sizes above, shuffled -> (streams, liblzma's decode of each)"""
    comp, plain = {}, {}
    for i, n in enumerate(SIZES):
        comp[n] = _raw_lzma2(corpus.plain("M", 700 + i, n) if n else b"")
        plain[n] = lzma.decompress(comp[n], format=lzma.FORMAT_RAW, filters=[dict(L2, dict_size=DICT)])
        assert len(plain[n]) == n
    order = [SIZES[i % len(SIZES)] for i in range(300)]
    random.Random(3131).shuffle(order)
    return [lzma_amd.Stream(comp[n], FMT_LZMA2_RAW, out_cap=n, dict_size=DICT) for n in order], [plain[n] for n in order]


def plan_items(sizes):
    """the items of the first test over streams of `sizes` -> (items, destination size): every (offset mod 16, dst_off mod
    16) pair at every length 0-40, whole streams back to back, ranges that reach past what a stream produced or start
    behind it; shuffled"""
    items, dst = [], 0
    big = [k for k, n in enumerate(sizes) if n >= 4095]
    j = 0
    for length in range(41):
        for s in range(16):
            for d in range(16):
                k = big[j % len(big)]
                j += 1
                dst += (d - dst) % 16
                items.append((k, 16 * ((7 * j) % 200) + s, length, dst))
                dst += length
    for k, n in enumerate(sizes):
        items.append((k, 0, n, dst))
        dst += n
    for k in range(0, len(sizes), 7):
        off = sizes[k] // 3
        length = sizes[k] - off + 1 + k
        items.append((k, off, length, dst))
        dst += length + k % 5
        items.append((k, sizes[k] + 5, 10, dst))
        dst += 10
    random.Random(99).shuffle(items)
    return items, dst + 33


def test_pack_of_a_device_resident_batch(ctx, streams300):
    streams, plains = streams300
    b = lzma_amd.Batch(ctx, streams)
    b.run()
    for k, (n, st, _) in enumerate(b.results()):
        assert n == len(plains[k]) and st >= 0, (k, n, st)
    items, cap = plan_items([len(p) for p in plains])
    pairs = {(off % 16, dst % 16, length) for _, off, length, dst in items if length <= 40}
    assert len(pairs) == 16 * 16 * 41
    dst = _filled(cap)
    want, copied, stats = expect_pack(items, plains, cap, dst.data_ptr() % 16)
    assert b.pack(items, dst.data_ptr(), cap) == copied
    got = _bytes(dst)
    if got != want:
        at = next(i for i in range(cap) if got[i] != want[i])
        raise AssertionError("the destination differs at byte %d of %d" % (at, cap))
    ps = ctx.last_pack_stats()
    print("Batch.pack: %s" % ps)
    assert {k: ps[k] for k in stats} == stats and ps["launches"] == 1 and ps["kernel_ms"] > 0, (ps, stats)
    assert 0 < stats["congruent_items"] < stats["items"] and stats["empty_items"] >= 256
    # a destination pointer that is no multiple of 16, whole streams back to back
    some, at = [], 0
    for k in range(60):
        some.append((k, 0, len(plains[k]), at))
        at += len(plains[k])
    dst = _filled(at + 64)
    want, copied, stats = expect_pack(some, plains, at + 59, (dst.data_ptr() + 5) % 16)
    assert b.pack(some, dst.data_ptr() + 5, at + 59) == copied
    assert _bytes(dst) == bytes([FILL]) * 5 + want
    ps = ctx.last_pack_stats()
    assert {k: ps[k] for k in stats} == stats, (ps, stats)
    # nothing to do
    assert b.pack([], dst.data_ptr(), 1) == [] and b.pack([(0, 0, 0, 0)], dst.data_ptr(), 1) == [0]
    b.close()


def test_pack_delivers_filtered_bytes(ctx):
    sizes = [0, 17, 4101, 65541, 300_001]
    plains = [R.opcode_soup(n, 40 + i) if n > 16 else bytes(n) for i, n in enumerate(sizes)]
    b = lzma_amd.Batch(ctx, [lzma_amd.Stream(_raw_lzma2(p), FMT_LZMA2_RAW, out_cap=len(p), dict_size=DICT) for p in plains])
    b.run()
    b.results()
    steps_of = {1: [(R.X86, 0)], 2: [(R.X86, 0), (R.DELTA, 3)], 3: [(R.X86, 4096), (R.DELTA, 3)], 4: [(R.X86, 0), (R.DELTA, 16)]}
    b.filter([(k, f, p) for k, st in steps_of.items() for f, p in st])
    filtered = [R.apply_steps(steps_of.get(k, []), p) for k, p in enumerate(plains)]
    assert sum(f != p for f, p in zip(filtered, plains)) >= 3
    items, at = [], 3
    for k, p in enumerate(plains):
        items.append((k, 0, len(p), at))
        at += len(p) + 1
    for want_of in (filtered, plains):   # (a new run decodes afresh: the pack delivers unfiltered bytes again)
        dst = _filled(at)
        want, copied, _ = expect_pack(items, want_of, at, 0)
        assert b.pack(items, dst.data_ptr(), at) == copied
        assert _bytes(dst) == want
        b.run()
        b.results()
    b.close()


def test_pack_argument_errors_write_nothing(ctx):
    plains = [corpus.plain("T", 5, 5000), corpus.plain("T", 6, 70_000)]
    b = lzma_amd.Batch(ctx, [lzma_amd.Stream(_raw_lzma2(p), FMT_LZMA2_RAW, out_cap=len(p), dict_size=DICT) for p in plains])
    b.run()
    b.results()
    cap = 100_000
    dst = _filled(cap)
    host = ctypes.create_string_buffer(cap)
    for what, items, ptr, c in (("overlap", [(0, 0, 100, 0), (1, 0, 100, 99)], dst.data_ptr(), cap),
                                ("overlap of declared ranges", [(0, 4990, 100, 0), (1, 0, 100, 50)], dst.data_ptr(), cap),
                                ("beyond dst_cap", [(0, 0, 100, cap - 99)], dst.data_ptr(), cap),
                                ("dst_off + len overflows", [(0, 0, (1 << 64) - 1, 2)], dst.data_ptr(), cap),
                                ("stream index", [(2, 0, 100, 0)], dst.data_ptr(), cap),
                                ("host pointer", [(0, 0, 100, 0)], ctypes.addressof(host), cap)):
        with pytest.raises(LzmaError) as e:
            b.pack(items, ptr, c)
        assert e.value.status == lzma_amd.ERR_BAD_ARG, what
    _torch().cuda.synchronize()
    assert _bytes(dst) == bytes([FILL]) * cap and host.raw == bytes(cap)
    assert b.pack([(0, 0, 100, 0), (1, 0, 100, 100)], dst.data_ptr(), cap) == [100, 100]   # (touching is no overlap)
    assert _bytes(dst)[:201] == plains[0][:100] + plains[1][:100] + bytes([FILL])
    b.close()


# ---- the container front-ends -----------------------------------------------------------------------------------------
def _both(ctx, name, data, cap, verify=1, shift=0):
    """the host form and the device form of front-end `name` ("xz" / "7z") on the same context -> (status, n, unverified,
    device bytes, host bytes); asserts that the three figures agree.  shift: move the device pointer off its alignment"""
    L = N.lib()
    host_fn, dev_fn = (L.xlz_xz_decode, L.xlz_xz_decode_device) if name == "xz" else (L.xlz_7z_decode, L.xlz_7z_decode_device)
    src = ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p)
    hbuf = ctypes.create_string_buffer(max(cap, 1))
    hn, hu = ctypes.c_uint64(77), ctypes.c_size_t(77)
    hst = host_fn(ctx._h, src, len(data), ctypes.cast(hbuf, ctypes.c_void_p), cap, ctypes.byref(hn), verify, ctypes.byref(hu))
    t = _filled(cap + shift)
    dn, du = ctypes.c_uint64(78), ctypes.c_size_t(78)
    dst = dev_fn(ctx._h, src, len(data), ctypes.c_void_p(t.data_ptr() + shift), cap, ctypes.byref(dn), verify, ctypes.byref(du))
    assert (dst, dn.value, du.value) == (hst, hn.value, hu.value), (name, len(data), cap)
    return dst, dn.value, du.value, _bytes(t)[shift:shift + dn.value], hbuf.raw[:hn.value]


def _xz_total(ctx, data):
    return lzma_amd.xz_index_chains(data)[2] if ctx.filter_mode() == 1 else lzma_amd.xz_index(data)[1]


def _xz_good(ctx, data, shift=0, unverified=0, want=None):
    total = _xz_total(ctx, data)
    st, n, u, dev, host = _both(ctx, "xz", data, total, shift=shift)
    assert (st, n, u) == (lzma_amd.OK, total, unverified)
    assert dev == (lzma.decompress(data) if want is None else want) == host


def _forty_blocks():
    sizes = list(range(1, 21)) + [65537 + k for k in range(20)]
    offs = [sum(sizes[:i]) % 16 for i in range(len(sizes))]
    assert set(offs[:20]) == set(range(16)) == set(offs[20:])   # (the small blocks' and the large blocks' offsets: every residue)
    return [(corpus.plain("M", 900 + i, n), [L2]) for i, n in enumerate(sizes)]


def test_xz_decode_device(ctx):
    one = [(corpus.plain("T", 1, 100_003), [L2])]
    forty = _forty_blocks()
    assert ctx.filter_mode() == 0 and ctx.check_mode() == 0
    for check in (lzma.CHECK_NONE, lzma.CHECK_CRC32, lzma.CHECK_CRC64):
        _xz_good(ctx, X.stream(one, check=check))
        _xz_good(ctx, X.stream(forty, check=check), shift=7 if check == lzma.CHECK_CRC32 else 0)
    first, second = X.stream(forty[:5], check=lzma.CHECK_CRC32), X.stream(one + forty[30:33], check=lzma.CHECK_CRC64)
    # (stream padding: Python's lzma module stops in front of it, so liblzma decodes the two streams one by one)
    _xz_good(ctx, first + bytes(8) + second + bytes(4), want=lzma.decompress(first) + lzma.decompress(second))
    sha = lzma.compress(corpus.plain("M", 2, 300_001), check=lzma.CHECK_SHA256, preset=0)
    _xz_good(ctx, sha)
    assert ctx.last_pack_stats()["bytes"] == 300_001 and ctx.last_check_stats()["device_ranges"] + ctx.last_check_stats()["host_ranges"] == 1
    empty = lzma.compress(b"")
    _xz_good(ctx, empty)
    try:   # the context's check mode says where a HOST destination verifies: the device form agrees with it in every mode
        for mode in (1, 2):
            ctx.set_check_mode(mode)
            _xz_good(ctx, X.stream(forty, check=lzma.CHECK_CRC64))
            _xz_good(ctx, sha)
    finally:
        ctx.set_check_mode(0)
    # without verify a damaged check is not looked at, by either form
    good = X.stream(one, check=lzma.CHECK_CRC32)
    blocks, total = lzma_amd.xz_index(good)
    bad_check = bytearray(good)
    bad_check[blocks[0]["check_off"]] ^= 1
    st, n, _, dev, _ = _both(ctx, "xz", bytes(bad_check), total, verify=0)
    assert (st, n) == (lzma_amd.OK, total) and dev == one[0][0]
    # the damaged cases: the status of the host form, nothing reported as decoded
    bad_payload = bytearray(good)
    bad_payload[blocks[0]["comp_off"] + blocks[0]["comp_len"] // 2] ^= 0x40
    chain = X.stream([(R.opcode_soup(50_000, 3), [{"id": lzma.FILTER_X86}, L2])], check=lzma.CHECK_CRC32)
    for what, data, cap, want in (("check byte", bytes(bad_check), total, lzma_amd.ERR_RESULT),
                                  ("payload byte", bytes(bad_payload), total, None),
                                  ("cut short", good[:-7], total, None),
                                  ("cut in the payload", good[:len(good) // 2], total, None),
                                  ("out_cap too small", good, total - 1, lzma_amd.ERR_OUT_CAP),
                                  ("chain in filter mode 0", chain, 50_000, lzma_amd.ERR_UNSUPPORTED)):
        st, n, _, _, _ = _both(ctx, "xz", data, cap)
        assert st < 0 and n == 0 and (want is None or st == want), (what, st)
    # python surface
    t = _filled(total)
    assert lzma_amd.xz_decode_device(ctx, good, t.data_ptr(), total) == total and _bytes(t) == one[0][0]
    with pytest.raises(LzmaError) as e:
        lzma_amd.xz_decode_device(ctx, bytes(bad_check), t.data_ptr(), total)
    assert e.value.status == lzma_amd.ERR_RESULT


def test_xz_decode_device_with_filter_chains(ctx):
    soup = [R.opcode_soup(n, 60 + i) for i, n in enumerate((70_001, 16_389, 200_000, 33))]
    blocks = [(soup[0], [{"id": lzma.FILTER_X86}, L2]),
              (soup[1], [{"id": lzma.FILTER_DELTA, "dist": 3}, {"id": lzma.FILTER_ARM}, L2]),
              (soup[2], [{"id": lzma.FILTER_DELTA, "dist": 1}, {"id": lzma.FILTER_X86, "start_offset": 4096}, {"id": lzma.FILTER_POWERPC}, L2]),
              (soup[3], [L2])]
    data = X.stream(blocks, check=lzma.CHECK_CRC64)
    assert lzma.decompress(data) == b"".join(soup)
    ctx.set_filter_mode(1)
    try:
        _xz_good(ctx, data)
        assert ctx.last_filter_stats()["device_steps"] == 6
        _xz_good(ctx, X.stream(blocks, check=lzma.CHECK_NONE), shift=3)
    finally:
        ctx.set_filter_mode(0)


def _sz_good(ctx, data, want, unverified=0):
    st, n, u, dev, host = _both(ctx, "7z", data, len(want))
    assert (st, n, u) == (lzma_amd.OK, len(want), unverified)
    assert dev == want == host


def test_sevenzip_decode_device(ctx):
    g = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    solid = open(os.path.join(g, "libarchive_solid.7z"), "rb").read()
    want = lzma_amd.sevenzip_decode(ctx, solid)
    exp = json.load(open(os.path.join(g, "libarchive_solid.json")))
    assert len(want) == lzma_amd.sevenzip_index(solid, ctx)[2] == sum(size for _name, size in exp["files"])
    _sz_good(ctx, solid, want)
    files = [corpus.plain("T", 40, 70_001), corpus.plain("R", 41, 9_000), corpus.plain("Z", 42, 150_000), b"",
             corpus.plain("M", 43, 200_003), b"tiny", corpus.plain("T", 44, 33_333)]
    r1, p1 = C.lzma_folder(b"".join(files[0:4]), dict_size=1 << 20)   # a solid folder: four files with CRCs of their own
    r2, p2 = C.lzma2_folder(files[4], dict_byte=12)
    r3, p3 = C.copy_folder(files[5])
    r4, p4 = C.lzma_folder(files[6], dict_size=4096, lc=0, lp=2, pb=0)
    fo = [(r1, p1, files[0:4]), (r2, p2, [files[4]]), (r3, p3, [files[5]]), (r4, p4, [files[6]])]
    for enc in (False, True):
        _sz_good(ctx, C.archive(fo, encoded_header=enc), b"".join(files))
    _sz_good(ctx, C.archive(fo, folder_crc=True), b"".join(files))
    _sz_good(ctx, C.archive([fo[2]]), files[5])                                       # nothing but a Copy folder
    _sz_good(ctx, C.archive([fo[1], fo[3]], with_substreams=False), files[4] + files[6], unverified=2)
    try:   # in check mode 1 the host form takes its CRCs from the device too
        ctx.set_check_mode(1)
        _sz_good(ctx, C.archive(fo), b"".join(files))
    finally:
        ctx.set_check_mode(0)
    # a wrong CRC: of a file in the solid folder, of the LZMA2 folder, of the Copy folder (which the host checks)
    other = lambda b: bytes([b[0] ^ 1]) + b[1:]
    for k, bad_files in ((0, [files[0], other(files[1]), files[2], b""]), (1, [other(files[4])]), (2, [other(files[5])])):
        bad = list(fo)
        bad[k] = (fo[k][0], fo[k][1], bad_files)
        st, n, _, _, _ = _both(ctx, "7z", C.archive(bad), len(b"".join(files)))
        assert (st, n) == (lzma_amd.ERR_RESULT, 0), k
    st, n, _, _, _ = _both(ctx, "7z", C.archive(fo), len(b"".join(files)) - 1)
    assert (st, n) == (lzma_amd.ERR_OUT_CAP, 0)
    # a chain: refused in filter mode 0, decoded in filter mode 1
    soup = R.opcode_soup(120_001, 77)
    rec, packed, nc = Z.chain_folder(soup, [{"id": lzma.FILTER_X86}])
    rec2, packed2, nc2 = Z.chain_folder(files[0], [{"id": lzma.FILTER_DELTA, "dist": 2}], lzma2=True)
    chained = Z.archive([(rec, packed, nc, [soup]), (rec2, packed2, nc2, [files[0][:100], files[0][100:]])])
    st, n, _, _, _ = _both(ctx, "7z", chained, len(soup) + len(files[0]))
    assert (st, n) == (lzma_amd.ERR_UNSUPPORTED, 0)
    ctx.set_filter_mode(1)
    try:
        _sz_good(ctx, chained, soup + files[0])
        t = _filled(len(soup) + len(files[0]))
        assert lzma_amd.sevenzip_decode_device(ctx, chained, t.data_ptr(), t.numel()) == t.numel() and _bytes(t) == soup + files[0]
        assert _bytes(lzma_amd.sevenzip_decode_tensor(ctx, chained)) == soup + files[0]
    finally:
        ctx.set_filter_mode(0)


def test_decode_tensor(ctx):
    torch = _torch()
    plain = corpus.plain("M", 11, 777_777)
    data = X.stream([(plain[:300_001], [L2]), (plain[300_001:], [L2])], check=lzma.CHECK_CRC64)
    t = lzma_amd.xz_decode_tensor(ctx, data)
    assert isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.device == torch.device("cuda", 0) and t.shape == (len(plain),)
    assert _bytes(t) == plain == lzma.decompress(data)
    out = _filled(len(plain) + 100)
    t = lzma_amd.xz_decode_tensor(ctx, data, out=out)
    assert t.data_ptr() == out.data_ptr() and t.shape == (len(plain),)
    assert _bytes(out) == plain + bytes([FILL]) * 100
    with pytest.raises(LzmaError) as e:
        lzma_amd.xz_decode_tensor(ctx, data, out=_filled(len(plain) - 1))
    assert e.value.status == lzma_amd.ERR_OUT_CAP
    with pytest.raises(ValueError):
        lzma_amd.xz_decode_tensor(ctx, data, out=torch.empty(len(plain), dtype=torch.int8, device="cuda"))
    r2, p2 = C.lzma2_folder(plain[:100_000], dict_byte=12)
    t = lzma_amd.sevenzip_decode_tensor(ctx, C.archive([(r2, p2, [plain[:100_000]])]))
    assert t.dtype == torch.uint8 and _bytes(t) == plain[:100_000]
