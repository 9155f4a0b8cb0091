"""CPU: the host walk along a .tar image's headers (lzma_amd.tar_parse: xlz_tar_parse_host, lzma_amd/csrc/xlz_tar_walk.h)
against Python's tarfile on the archives of tests/tar_archives.py: tarfile's three formats, each with an empty file, a
directory, a 513-byte file, a 180-byte name ustar can split, a 90-byte symlink target, a hard link, 512 bytes of 0xC8 and a
tar stored as a member; GNU long names; pax global and size records; libarchive's gnutar and pax writers; hand-built
headers; archives that are cut, damaged or unsupported; 2000 single-byte mutations."""
import ctypes
import os
import random
import sys
import tarfile

import pytest

import lzma_amd
from lzma_amd import _native as N

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tar_archives as T  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _built(xlz_so):
    return xlz_so


@pytest.mark.parametrize("name", ["ustar", "gnu", "pax", "gnu_long", "pax_global_size", "crafted", "empty", "libarchive_gnutar", "libarchive_pax"])
def test_table_is_what_tarfile_reports(name):
    image = T.everything()[name]
    table = lzma_amd.tar_parse(image)
    want = T.judge(image)
    assert table.end_status == lzma_amd.OK, (table.end_status, table.end_off)
    assert T.rows(table.entries) == want
    assert len(want) == {"ustar": 9, "gnu": 9, "pax": 9, "gnu_long": 4, "pax_global_size": 2, "crafted": 10, "empty": 0}.get(name, len(want))
    for e in table.entries:
        assert e.hdr_off % 512 == 0 and e.data_off % 512 == 0 and e.hdr_off < e.data_off <= len(image)


def test_what_the_archives_exercise():
    """the archives hold what their names promise: meta entries, a split name, false candidates"""
    gnu = lzma_amd.tar_parse(T.standard("gnu")).entries
    assert [e.name for e in gnu][3] == T.LONG and gnu[3].data_off - gnu[3].hdr_off == 3 * 512  # 'L' header, its data, the header
    ustar = lzma_amd.tar_parse(T.standard("ustar")).entries
    assert ustar[3].name == T.LONG and ustar[3].data_off - ustar[3].hdr_off == 512  # prefix + name
    pax = lzma_amd.tar_parse(T.standard("pax")).entries
    assert pax[3].name == T.LONG and pax[3].data_off - pax[3].hdr_off == 3 * 512  # 'x' header, its records, the header
    long = lzma_amd.tar_parse(T.gnu_long()).entries
    assert (len(long[1].name), len(long[1].linkname), long[1].type) == (300, 300, b"2") and long[1].data_off - long[1].hdr_off == 5 * 512
    assert long[2].name == "d" * 150 and long[2].type == b"5"
    p = lzma_amd.tar_parse(T.pax_global_size()).entries
    assert (p[0].name, p[0].size, p[0].uid, p[0].gid, p[0].mtime, p[0].hdr_off) == ("renamed/by/pax", 700, 70000, 4242, 1600000000.25, 1024)
    assert (p[1].name, p[1].size, p[1].gid) == ("plain", 10, 4242)
    c = {e.name: e for e in lzma_amd.tar_parse(T.crafted()).entries}
    assert c["big256"].size == 1000 and c["olddir"].type == b"5" and c["olddir"].size == 512
    assert [c["node%d" % t].size for t in (3, 4, 5, 6)] == [4096] * 4 and c["unknown"].type == b"Z" and c["unknown"].size == 600
    assert c["oldfile"].type == b"\0" and "some/prefix/leaf" in c and "dirs" in c
    # the tar stored as a member: its headers are candidates that the walk never reaches
    image = T.standard("gnu")
    cands = sum(1 for b in range(len(image) // 512) if T.serial_flag(image[512 * b:512 * b + 512]) == 1)
    assert cands > len(T.judge(image)) + 2 and len(T.judge(T.inner())) == 3


@pytest.mark.parametrize("name", sorted(T.damaged()))
def test_archives_that_do_not_end_cleanly(name):
    image, status, listed = T.damaged()[name]
    table = lzma_amd.tar_parse(image)
    assert table.end_status == getattr(lzma_amd, status), (table.end_status, table.end_off)
    assert len(table.entries) == listed
    if name in ("cut_in_header", "cut_in_data", "cut_behind_member", "flipped_third_header"):
        assert T.rows(table.entries) == T.judge(T.standard("gnu"))[:listed]
    for e in table.entries:
        assert e.data_off + e.size <= len(image)
    if name == "flipped_third_header":
        assert table.end_off == T.judge(T.standard("gnu"))[2][8]
    if name == "cut_behind_member":
        assert table.end_off == len(image) and T.rows(table.entries) == T.judge(image)


def test_more_ends():
    ok = T.member(b"ok", b"1")
    for image, status, listed in [
            (b"", "OK", 0), (b"\0" * 511, "ERR_UNEXPECTED_EOF", 0), (b"x" * 512, "ERR_RESULT", 0),
            (ok + T.header(b"f", size_field=b"\xff" * 12), "ERR_RESULT", 1),                           # a negative base-256 size
            (ok + T.member(b"m", b"x" * 10, type=b"M") + T.END, "ERR_UNSUPPORTED", 1),                  # multi-volume continuation
            (ok + T.member(b"x", T.pax_records([(b"GNU.sparse.major", b"1")]), type=b"x") + ok + T.END, "ERR_UNSUPPORTED", 1),
            (ok + T.member(b"L", b"name\0", type=b"L") + T.END, "ERR_RESULT", 1),                       # a long name that no member follows
            (ok + T.member(b"L", b"name\0", type=b"L"), "ERR_UNEXPECTED_EOF", 1),
            (ok + T.member(b"x", b"9 size=x\n", type=b"x") + ok + T.END, "ERR_RESULT", 1),              # a number that is none
            (ok + T.header(b"f", size_field=b"0000000001x\0"), "ERR_RESULT", 1),
            (ok + bytes(512) + b"junk" * 128, "OK", 1),                                                 # what follows a zero block is ignored
    ]:
        table = lzma_amd.tar_parse(image)
        assert (table.end_status, len(table.entries)) == (getattr(lzma_amd, status), listed), (image[:600], table)


def test_2000_single_byte_mutations():
    """no crash; every listed member with data lies inside the image; where the walk ends cleanly the table is tarfile's"""
    base = T.gnu_long()[:T.judge(T.gnu_long())[-1][9] + 1024] + T.standard("gnu")  # (one chain: the first archive's end blocks cut off)
    assert lzma_amd.tar_parse(base).end_status == lzma_amd.OK and len(T.judge(base)) == 13
    rng = random.Random(20261019)
    headers = [m[8] for m in T.judge(base)]
    clean = compared = 0
    for k in range(2000):
        image = bytearray(base)
        # half of the mutations go into header and meta blocks, where they matter
        at = rng.choice(headers) + rng.randrange(1536) if k % 2 else rng.randrange(len(base))
        at = min(at, len(base) - 1)
        image[at] ^= rng.randrange(1, 256)
        image = bytes(image)
        table = lzma_amd.tar_parse(image)
        for e in table.entries:
            assert e.hdr_off < e.data_off <= len(image) and (b"1" <= e.type <= b"6" or e.data_off + e.size <= len(image)), (at, e)
        assert table.end_off <= len(image)
        if table.end_status == lzma_amd.OK:
            clean += 1
            try:
                want = T.judge(image)
            except tarfile.TarError as err:
                raise AssertionError("mutation at %d: the walk ends cleanly, tarfile says %r" % (at, err))
            assert T.rows(table.entries) == want, at
            compared += 1
    assert clean > 500 and clean < 2000 and compared == clean


def test_entry_points_need_their_objects():
    L = N.lib()
    h = ctypes.c_void_p(7)
    assert L.xlz_tar_parse_host(None, 512, ctypes.byref(h)) == lzma_amd.ERR_BAD_ARG and not h.value
    assert L.xlz_tar_parse_host(ctypes.c_char_p(b"x"), 0, None) == lzma_amd.ERR_BAD_ARG
    assert L.xlz_tar_scan_device(None, None, 0, ctypes.byref(h)) == lzma_amd.ERR_BAD_ARG
    assert L.xlz_tar_scan_device(None, ctypes.c_void_p(4096), 512, None) == lzma_amd.ERR_BAD_ARG
    assert L.xlz_xz_tar_list(None, None, 1, ctypes.byref(h), None) == lzma_amd.ERR_BAD_ARG
    assert L.xlz_xz_tar_list(None, None, 1, None, None) == lzma_amd.ERR_BAD_ARG
    assert L.xlz_tar_entries(None, None, 0, None, 0) == lzma_amd.ERR_BAD_ARG
    assert L.xlz_ctx_last_tar_stats(None, None) == lzma_amd.ERR_BAD_ARG
    ms = ctypes.c_double()
    assert L.xlz_internal_tar_classify_device(None, None, 0, None, ctypes.byref(ms)) == lzma_amd.ERR_BAD_ARG
    n, end = ctypes.c_size_t(7), ctypes.c_int(0)
    L.xlz_tar_info(None, ctypes.byref(n), None, ctypes.byref(end), None)
    assert (n.value, end.value) == (0, lzma_amd.ERR_BAD_ARG)
    L.xlz_tar_close(None)
    # a table larger than the caller's arrays
    assert L.xlz_tar_parse_host(ctypes.c_char_p(T.standard("ustar")), len(T.standard("ustar")), ctypes.byref(h)) == lzma_amd.OK
    ents = (N.TarEntry * 2)()
    assert L.xlz_tar_entries(h, ents, 2, None, 0) == lzma_amd.ERR_OUT_CAP and ents[1].name_len == 3
    L.xlz_tar_close(h)
    assert ctypes.sizeof(N.TarEntry) == 72 and ctypes.sizeof(N.TarStats) == 64


def test_python_names():
    code = ("import sys, lzma_amd; assert 'torch' not in sys.modules; "
            "print(sorted(n for n in dir(lzma_amd) if 'tar' in n.lower()))")
    import subprocess
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0, r.stderr
    for name in ("TarEntry", "TarXzFile", "tar_parse", "tar_scan_device", "xz_tar_tensor"):
        assert name in r.stdout
    assert lzma_amd.TarEntry._fields == ("name", "linkname", "size", "type", "mode", "uid", "gid", "mtime", "hdr_off", "data_off")
    with pytest.raises(ValueError):
        lzma_amd.TarXzFile(__import__("lzma").compress(T.END)).index(0)
