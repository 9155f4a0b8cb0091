"""CPU: the gzip / BGZF / zlib container layer (lzma_amd/csrc/xlz_gz.h) through xlz_gz_probe and xlz_gz_decode_host, on the
cases of tests/gz_files.py.  The judges are Python's gzip.decompress and zlib.decompressobj: every case agrees with them on
OK / not OK and, where OK, on every byte, out_len and in_consumed -- but the two classes gz_files.SPECIAL names, which are
asserted against the statuses the feature sets for them."""
import ctypes
import struct
import zlib

import pytest

import gz_files as G
from lzma_amd import _native as N
from lzma_amd import gz

HEADER_CASES = G.header_cases()
MEMBER_CASES = G.member_cases()


check = G.check


def test_the_new_symbols_and_struct_sizes(xlz_so):
    L = N.lib()
    for name in ("xlz_adler32_device", "xlz_adler32_host", "xlz_adler32_combine", "xlz_gz_probe", "xlz_gz_decode_host",
                 "xlz_gz_decode_many_device", "xlz_gz_decode_many", "xlz_ctx_last_gz_stats"):
        assert name in N.EXPORTS and hasattr(L, name), name
    sizes = {N.AdlerRange: 16, N.GzInfo: 40, N.GzFile: 40, N.GzResult: 24, N.GzStats: 80}
    for struct_, size in sizes.items():
        assert ctypes.sizeof(struct_) == size, struct_
        assert sum(ctypes.sizeof(t) for _, t in struct_._fields_) == size, struct_   # (no implicit padding)
    assert (gz.AUTO, gz.GZIP, gz.ZLIB) == (0, 1, 2) and (gz.F_BGZF, gz.F_NAME, gz.F_COMMENT, gz.F_HCRC) == (1, 2, 4, 8)


def test_arguments_that_need_no_context(xlz_so):
    L = N.lib()
    bad = -7
    assert L.xlz_gz_probe(None, 0, 0, None) == bad and L.xlz_gz_probe(None, 5, 0, ctypes.byref(N.GzInfo())) == bad
    assert L.xlz_gz_probe(None, 0, 3, ctypes.byref(N.GzInfo())) == bad
    assert L.xlz_gz_decode_host(None, 0, 0, None, 0, 1, None) == bad
    assert L.xlz_gz_decode_host(None, 0, 7, None, 0, 1, ctypes.byref(N.GzResult())) == bad
    assert L.xlz_gz_decode_many(None, None, 0, None, 0, 1, None) == bad and L.xlz_gz_decode_many_device(None, None, 0, None, 0, 1, None) == bad
    assert L.xlz_ctx_last_gz_stats(None, ctypes.byref(N.GzStats())) == bad
    assert L.xlz_adler32_device(None, None, 0, None, 0, None) == bad
    assert gz.decode_host(b"", out_cap=0)[1] == G.ERR_UNEXPECTED_EOF and gz.decode_host(b"\x1f", out_cap=0)[1] == G.ERR_UNEXPECTED_EOF
    assert gz.decode_host(b"\0\0", out_cap=0)[1] == G.ERR_RESULT   # AUTO: neither 1f 8b nor a zlib header


@pytest.mark.parametrize("c", HEADER_CASES, ids=[c.name for c in HEADER_CASES])
def test_header_matrix(xlz_so, c):
    check(c, gz.decode_host(c.data, out_cap=c.cap))
    check(c, gz.decode_host(c.data, out_cap=c.cap, verify=False), verify=False)
    info = gz.probe(c.data)
    assert info["format"] == gz.GZIP and not info["bgzf"] and info["members"] == 0 and info["size_hint"] == c.cap
    if c.name.startswith("flg_"):
        flg = int(c.name[4:])
        assert info["name"] == (b"file.txt" if flg & G.FNAME else None)
        assert info["flags"] == (gz.F_NAME if flg & G.FNAME else 0) | (gz.F_COMMENT if flg & G.FCOMMENT else 0) | (gz.F_HCRC if flg & G.FHCRC else 0)


def test_every_header_and_trailer_cut_at_every_byte(xlz_so):
    p = G.payload("cut", 300)
    whole = G.member(p, flg=31, extra=G.subfield(b"ab", b"xyz") + G.subfield(b"BC", b"\1\2"), name=b"name", comment=b"comment", mtime=77)
    hdr = len(G.header(flg=31, extra=G.subfield(b"ab", b"xyz") + G.subfield(b"BC", b"\1\2"), name=b"name", comment=b"comment", mtime=77))
    assert gz.decode_host(whole, out_cap=300)[:2] == (p, G.OK)
    for cut in list(range(0, hdr + 1)) + list(range(len(whole) - 8, len(whole))):
        got = gz.decode_host(whole[:cut], out_cap=300, format=gz.GZIP)
        assert got[1] == G.ERR_UNEXPECTED_EOF and got[0] is None, cut   # (cut == hdr: the deflate stream has no byte)
        if cut:
            assert not G.judge_gzip(whole[:cut])[0], cut
        if cut < hdr:
            with pytest.raises(gz.LzmaError) as e:
                gz.probe(whole[:cut], gz.GZIP)
            assert e.value.status == G.ERR_UNEXPECTED_EOF
    z = G.zlib_stream(p)
    for cut in (0, 1, len(z) - 4, len(z) - 3, len(z) - 2, len(z) - 1):
        assert gz.decode_host(z[:cut], out_cap=300, format=gz.ZLIB)[1] == G.ERR_UNEXPECTED_EOF, cut
        assert not G.judge_zlib(z[:cut])[0]


def test_all_65536_zlib_headers(xlz_so):
    """in front of one valid body (no distance above 256: every CINFO's window holds it); acceptance is zlib's, and a header
    that is sound but for FDICT is XLZ_ERR_UNSUPPORTED"""
    p = b"zlib header matrix " * 8
    body = G.zlib_stream(p)[2:]
    L = N.lib()
    out = ctypes.create_string_buffer(len(p))
    r = N.GzResult()
    accepted = 0
    for h in range(65536):
        data = struct.pack(">H", h) + body
        buf = ctypes.create_string_buffer(data, len(data))
        for fmt in (gz.ZLIB, gz.AUTO):
            assert L.xlz_gz_decode_host(ctypes.cast(buf, ctypes.c_void_p), len(data), fmt, ctypes.cast(out, ctypes.c_void_p), len(p), 1, ctypes.byref(r)) == 0
            cmf, flg = h >> 8, h & 255
            sound = (cmf & 15) == 8 and (cmf >> 4) <= 7 and h % 31 == 0
            if fmt == gz.AUTO and h == 0x1F8B:
                assert r.status != G.OK   # (AUTO reads 1f 8b as gzip; as a zlib header it is unsound anyway)
                continue
            ok = G.judge_zlib(data)[0]
            assert (r.status == G.OK) == ok, (hex(h), r.status)
            if sound and flg & 0x20:
                assert r.status == G.ERR_UNSUPPORTED, hex(h)
            elif not ok:
                assert r.status == G.ERR_RESULT, hex(h)
            else:
                assert sound and out.raw == p and r.in_consumed == len(data)
                accepted += fmt == gz.ZLIB
    assert accepted == sum(1 for h in range(65536) if (h >> 8) & 15 == 8 and (h >> 12) <= 7 and h % 31 == 0 and not h & 0x20) > 0


@pytest.mark.parametrize("verify", [True, False], ids=["verify", "no_verify"])
@pytest.mark.parametrize("c", MEMBER_CASES, ids=[c.name for c in MEMBER_CASES])
def test_members_bgzf_and_defects(xlz_so, c, verify):
    check(c, gz.decode_host(c.data, out_cap=c.cap, verify=verify), verify)
    check(c, gz.decode_host(c.data, out_cap=c.cap + 100, verify=verify), verify)   # (room to spare changes nothing)


def test_the_statuses_of_named_defects(xlz_so):
    by = {c.name: c for c in MEMBER_CASES}
    want = {"junk_behind_member": G.ERR_RESULT, "cut_second_member": G.ERR_UNEXPECTED_EOF, "cut_second_header": G.ERR_UNEXPECTED_EOF,
            "second_member_bad_data": G.ERR_RESULT, "method_7": G.ERR_UNSUPPORTED, "wrong_magic": G.ERR_RESULT, "flipped_crc": G.ERR_RESULT,
            "flipped_crc_first_of_two": G.ERR_RESULT, "flipped_isize": G.ERR_RESULT, "bgzf_isize_plus_1": G.ERR_RESULT,
            "bgzf_isize_minus_1": G.ERR_RESULT, "bgzf_body_ends_one_early": G.ERR_RESULT, "bgzf_flipped_crc": G.ERR_RESULT,
            "bgzf_bad_data_in_block": G.ERR_RESULT, "zlib_flipped_adler": G.ERR_RESULT, "zlib_cut_trailer": G.ERR_UNEXPECTED_EOF,
            "zlib_cut_body": G.ERR_UNEXPECTED_EOF, "zlib_fdict": G.ERR_UNSUPPORTED, "zlib_bad_header_check": G.ERR_RESULT,
            "wrong_fhcrc": G.ERR_RESULT, "wrong_fhcrc_second_member": G.ERR_RESULT, "reserved_flg_bit5": G.ERR_UNSUPPORTED,
            "reserved_flg_bit7": G.ERR_UNSUPPORTED}
    for name, status in want.items():
        assert gz.decode_host(by[name].data, out_cap=by[name].cap)[1] == status, name
    assert set(c.name for c in MEMBER_CASES if c.special) == {n for n in want if n.startswith(("wrong_fhcrc", "reserved_flg"))}
    # the ISIZE window of a BGZF block is its own: one that overflows it is a bad block, not a small destination
    assert gz.decode_host(by["bgzf_isize_minus_1"].data, out_cap=1 << 20)[1] == G.ERR_RESULT


def test_probe_tells_bgzf_from_gzip(xlz_so):
    by = {c.name: c for c in MEMBER_CASES}
    info = gz.probe(by["bgzf_5_blocks_eof"].data)
    assert info["bgzf"] and info["members"] == 6 and info["size_hint"] == by["bgzf_5_blocks_eof"].cap and info["format"] == gz.GZIP
    assert gz.probe(by["bgzf_no_eof"].data)["members"] == 5 and gz.probe(by["bgzf_eof_then_zeros"].data)["members"] == 6
    assert gz.probe(by["bgzf_bc_last_of_three"].data)["bgzf"]
    over = gz.probe(by["bgzf_chain_overshoots_by_one"].data)
    assert not over["bgzf"] and over["members"] == 0
    assert gz.decode_host(by["bgzf_5_blocks_eof"].data)[3] == 6 and gz.decode_host(by["three_members"].data, out_cap=by["three_members"].cap)[3] == 3
    z = gz.probe(by["zlib_one"].data)
    assert z["format"] == gz.ZLIB and z["size_hint"] == 0 and z["members"] == 0
    with pytest.raises(ValueError):
        gz.layout([by["zlib_one"].data])
    assert gz.layout([by["one_member"].data, by["zlib_one"].data, by["bgzf_no_eof"].data], caps=[None, 3000, None], align=64) == (
        [(0, 3000), (3008, 3000), (6016, by["bgzf_no_eof"].cap)], 6016 + by["bgzf_no_eof"].cap)


@pytest.mark.parametrize("name", ["one_member", "three_members", "bgzf_5_blocks_eof", "zlib_one"])
def test_dst_cap_exact_one_short_and_zero(xlz_so, name):
    c = {c.name: c for c in MEMBER_CASES}[name]
    ok, data, used = G.judge(c)[1:]
    assert ok and gz.decode_host(c.data, out_cap=len(data))[:3] == (data, G.OK, used)
    for cap in (len(data) - 1, 0):
        assert gz.decode_host(c.data, out_cap=cap)[:3] == (None, G.ERR_OUT_CAP, 0), cap
    empty = {c.name: c for c in MEMBER_CASES}["empty_member"]
    assert gz.decode_host(empty.data, out_cap=0)[:2] == (b"", G.OK)
