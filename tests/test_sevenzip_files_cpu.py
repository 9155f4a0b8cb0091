"""CPU: the file table of a .7z archive (include/xlz.h: xlz_7z_open / xlz_7z_archive_* / xlz_7z_cover /
xlz_7z_extract_layout) and what an extraction settles before it uses its context.  The archives are written by
tests/sevenzip_files.py from 7-Zip's published format description, and by libarchive through `cmake -E tar`, whose own
listing is the independent judge of the names.  What a CUT folder's stream must end in is taken from the CPU oracle and
pinned here.  The shared header (lzma_amd/csrc/xlz_7z_files.h) runs in a g++ program of its own against brute-force
models, plain and under the host sanitizers, and a stand-alone fuzz program mutates headers through xlz_7z_open."""
import ctypes
import glob
import os
import shutil
import subprocess
import zlib

import pytest

import lzma_amd
import oracle
import sevenzip_bcj2 as B
import sevenzip_chains
import sevenzip_craft as C
import sevenzip_files as F
import sevenzip_read
from lzma_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

SOLID = [b"a", b"b" * 15, bytes(range(17)), bytes(4097), bytes((i * 7 + i // 251) & 0xFF for i in range(70001))]
PARTS = [bytes((i * 13 + i // 7) & 0xFF for i in range(3000)), b"z" * 5000, bytes(range(256)) * 20]
NAMES = ["plain.txt", "dir/é中.bin", "emoji-\U0001F600", "zeros", "big.bin"]
LONE = "lone-\ud800-surrogate"  # (the empty file's name)


def _archive(encoded_header=False, **kw):
    """one solid LZMA folder, one LZMA2 folder of three units, a Copy folder; a directory, an empty file and an anti item in
    between; names of every kind; times and attributes partly defined"""
    rec, pk = C.lzma_folder(b"".join(SOLID))
    rec2, pk2 = F.lzma2_units_folder(PARTS)
    rec3, pk3 = C.copy_folder(b"copied bytes")
    folders = [B.plain_folder(rec, pk, SOLID), B.plain_folder(rec2, pk2, PARTS), B.plain_folder(rec3, pk3, [b"copied", b" bytes"])]
    entries = [F.entry("top", "dir", mtime=F.filetime(1_600_000_000), attr=0x10),
               F.entry(NAMES[0], mtime=F.filetime(1_700_000_000.5), attr=0x20), F.entry(NAMES[1]), F.entry(NAMES[2], attr=0x21),
               F.entry(LONE, "empty"), F.entry(NAMES[3], mtime=F.filetime(0)), F.entry(NAMES[4]),
               F.entry("gone", "anti"), F.entry("p0"), F.entry("p1"), F.entry("p2"), F.entry("c0"), F.entry("c1")]
    return F.archive(folders, entries, encoded_header=encoded_header, **kw), folders, entries


def _open_status(data, ctx=None):
    h = ctypes.c_void_p()
    buf = ctypes.create_string_buffer(data, len(data))
    st = N.lib().xlz_7z_open(None, ctypes.cast(buf, ctypes.c_void_p), len(data), ctypes.byref(h))
    if st == lzma_amd.OK:
        N.lib().xlz_7z_close(h)
    else:
        assert not h
    return st


def _index_status(data):
    try:
        lzma_amd.sevenzip_index_bcj2(data)
        return lzma_amd.OK
    except lzma_amd.LzmaError as e:
        return e.status


def test_the_table_of_a_crafted_archive_is_what_went_in(xlz_so):
    arc, folders, entries = _archive()
    with lzma_amd.SevenZipFile(arc) as z:
        assert z.names == [F.as_utf8(e["name"]) for e in entries]
        assert "�" in z.names[4] and "\U0001F600" in z.names[3]
        files = [x for f in folders for x in f["files"]]
        at = 0
        for e, got in zip(entries, z.entries):
            assert got.has_stream == (e["kind"] == "file")
            assert got.is_dir == (e["kind"] == "dir") and got.is_anti == (e["kind"] == "anti")
            assert got.attributes == e["attr"]
            assert got.mtime == (None if e["mtime"] is None else (e["mtime"] - F.EPOCH) / 1e7)
            if got.has_stream:
                assert (got.size, got.crc) == (len(files[at]), zlib.crc32(files[at]))
                at += 1
            else:
                assert (got.size, got.crc, got.folder, got.folder_off) == (0, None, None, None)
        assert at == len(files) and z.total_size == sum(len(x) for x in files)
        # sizes, CRCs and offsets against the substream table of the index call
        fo, subs, steps, recs, total = lzma_amd.sevenzip_index_bcj2(arc)
        assert z.folders == fo and total == z.total_size
        with_stream = [e for e in z.entries if e.has_stream]
        assert [(e.size, e.crc) for e in with_stream] == [tuple(s) for s in subs]
        for k, f in enumerate(fo):
            off = 0
            for e in with_stream[f["first_substream"]:f["first_substream"] + f["n_substreams"]]:
                assert (e.folder, e.folder_off) == (k, off)
                off += e.size
            assert off == f["unpack_len"]
        assert z.index("p1") == 9 and z.index(3) == 3
        with pytest.raises(KeyError):
            z.index("no such name")
    with pytest.raises(lzma_amd.LzmaError) as ei:
        z.cover([1])
    assert ei.value.status == lzma_amd.ERR_CLOSED


def test_archives_without_names_or_without_files_info(xlz_so):
    rec, pk = C.lzma_folder(b"".join(SOLID[:3]))
    with lzma_amd.SevenZipFile(C.archive([(rec, pk, SOLID[:3])])) as z:  # the one-property section of the craft module
        assert z.names == ["", "", ""] and [e.size for e in z.entries] == [1, 15, 17]
    with lzma_amd.SevenZipFile(C.archive([(rec, pk, SOLID[:3])], junk_files_info=False)) as z:
        assert z.entries == [] and len(z.folders) == 1
    with lzma_amd.SevenZipFile(F.archive([], [F.entry("d", "dir"), F.entry("e", "empty")])) as z:  # no streams at all
        assert [(e.name, e.is_dir, e.has_stream) for e in z.entries] == [("d", True, False), ("e", False, False)] and z.folders == []


def _craft_archives():
    rec, pk = C.lzma_folder(b"".join(SOLID[:3]))
    rec2, pk2 = C.lzma2_folder(PARTS[0])
    x86 = bytes(range(256)) * 8
    ch = sevenzip_chains.chain_folder(x86, [{"id": 4}])
    yield "craft plain", C.archive([(rec, pk, SOLID[:3]), (rec2, pk2, [PARTS[0]])])
    yield "craft folder crc", C.archive([(rec2, pk2, [PARTS[0]])], folder_crc=True)
    yield "craft chain refused by the old index", C.archive([C.bcj_lzma_folder(x86) + ([x86],)])
    yield "chains", sevenzip_chains.archive([ch[:3] + ([x86],)], names=["x.exe"])
    yield "bcj2", B.archive([B.bcj2_folder([B.bcj2_ref.trap_data(3)[0]], form=4)], names=["t.exe"])
    yield "files", _archive()[0]
    yield "damaged signature", b"7z\xbc\xaf\x27\x1d" + _archive()[0][6:]
    yield "cut short", _archive()[0][:-9]


def test_open_returns_what_the_index_returns(xlz_so):
    """every committed .7z and every craft archive: the status of xlz_7z_index_bcj2 (an encoded header with ctx == NULL needs
    the device in both calls: the same archive with its header stored plainly is what is compared)"""
    seen = 0
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*.7z"))):
        a = open(path, "rb").read()
        st = _open_status(a)
        assert st == _index_status(a), path
        if st == lzma_amd.ERR_DEVICE:  # an encoded header (libarchive's): the same archive with its header stored plainly
            a = sevenzip_read.with_plain_header(a)
            st = _open_status(a)
            assert st == _index_status(a), path
        seen += st == lzma_amd.OK  # (7z_coder_without_input.7z is one both calls refuse)
    assert seen >= 1 and _open_status(open(os.path.join(GOLDEN, "libarchive_solid.7z"), "rb").read()) == lzma_amd.ERR_DEVICE
    for name, a in _craft_archives():
        assert _open_status(a) == _index_status(a), name


def _cmake_7z(files, tmp_path, name):
    if not shutil.which("cmake"):
        pytest.skip("no cmake on this box: nothing here writes a .7z archive")
    d = tmp_path / name
    d.mkdir()
    for n, b in files:
        (d / n).write_bytes(b)
    out = tmp_path / (name + ".7z")
    subprocess.check_call(["cmake", "-E", "tar", "cf", str(out), "--format=7zip"] + [n for n, _ in files], cwd=str(d))
    return out


def _cmake_listing(path):
    return subprocess.run(["cmake", "-E", "tar", "tf", str(path)], capture_output=True, text=True, check=True).stdout.splitlines()


def test_names_are_what_libarchive_lists(xlz_so, tmp_path):
    """libarchive's reader is the independent judge: the committed archive and one written here"""
    if not shutil.which("cmake"):
        pytest.skip("no cmake on this box: nothing here lists a .7z archive")
    golden = os.path.join(GOLDEN, "libarchive_solid.7z")
    files = [("one.txt", b"first file\n" * 40), ("two with space.bin", bytes(range(256)) * 3), ("empty.dat", b""), ("last", b"z")]
    for path, want in ((golden, None), (_cmake_7z(files, tmp_path, "listed"), files)):
        with lzma_amd.SevenZipFile(sevenzip_read.with_plain_header(open(path, "rb").read())) as z:
            assert z.names == _cmake_listing(path)
            if want:
                # (libarchive writes the entries without a stream behind the others)
                assert sorted((e.name, e.size, e.crc or 0) for e in z.entries) == sorted((n, len(b), zlib.crc32(b) if b else 0) for n, b in want)
                assert [e.has_stream for e in z.entries] == [e.size > 0 for e in z.entries] and not any(e.is_dir for e in z.entries)
                assert all(e.mtime is not None for e in z.entries)


def _with_files(section):
    rec, pk = C.lzma_folder(b"".join(SOLID[:2]))
    return F.archive([B.plain_folder(rec, pk, SOLID[:2])], files=section)


def _section(n, *props, end=True):
    return bytes([C.K_FILES]) + C.number(n) + b"".join(props) + (bytes([C.K_END]) if end else b"")


REFUSED = {
    "External names": (_section(2, F.prop(F.K_NAMES, b"\x01" + F.utf16("a\0b\0"))), lzma_amd.ERR_UNSUPPORTED),
    "External times": (_section(2, F.prop(F.K_MTIME, b"\x01\x01" + bytes(16))), lzma_amd.ERR_UNSUPPORTED),
    "a property that does not fill its size": (_section(2, F.prop(F.K_NAMES, b"\x00" + F.utf16("a\0b\0") + b"\0\0")), lzma_amd.ERR_RESULT),
    "a bit vector that does not fill its size": (_section(2, F.prop(F.K_ATTRIBUTES, b"\x00\x80\x00" + bytes(4) + b"\x00")), lzma_amd.ERR_RESULT),
    "a property that overruns its size": (_section(2, F.prop(F.K_MTIME, b"\x01\x00" + bytes(15))), lzma_amd.ERR_RESULT),
    "a size the header does not hold": (_section(2, bytes([F.K_DUMMY]) + C.number(200)), lzma_amd.ERR_RESULT),
    "one name too few": (_section(2, F.prop(F.K_NAMES, b"\x00" + F.utf16("a\0"))), lzma_amd.ERR_RESULT),
    "one name too many": (_section(2, F.prop(F.K_NAMES, b"\x00" + F.utf16("a\0b\0c\0"))), lzma_amd.ERR_RESULT),
    "an unterminated name": (_section(2, F.prop(F.K_NAMES, b"\x00" + F.utf16("a\0b"))), lzma_amd.ERR_RESULT),
    "more entries than substreams": (_section(3, F.prop(F.K_DUMMY, b"")), lzma_amd.ERR_RESULT),
    "fewer entries than substreams": (_section(3, F.prop(F.K_EMPTY_STREAM, b"\xc0")), lzma_amd.ERR_RESULT),
    "no end of the section": (_section(2, end=False)[:-1], lzma_amd.ERR_RESULT),
    "too many entries": (_section(1 << 25), lzma_amd.ERR_UNSUPPORTED),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals_and_the_old_calls_that_never_look(xlz_so, name):
    section, want = REFUSED[name]
    a = _with_files(section)
    assert _open_status(a) == want
    # xlz_7z_index* ignore FilesInfo exactly as before: the archive still indexes
    fo, subs, total = lzma_amd.sevenzip_index(a)
    assert total == 16 and [s[0] for s in subs] == [1, 15]
    assert lzma_amd.sevenzip_index_bcj2(a)[4] == 16 and lzma_amd.sevenzip_index_chains(a)[3] == 16


def test_a_good_section_next_to_the_refused_ones(xlz_so):
    a = _with_files(_section(3, F.prop(F.K_EMPTY_STREAM, b"\x40"), F.prop(0x77, b"unknown"), F.prop(F.K_NAMES, b"\x00" + F.utf16("a\0d\0b\0"))))
    with lzma_amd.SevenZipFile(a) as z:
        assert [(e.name, e.size, e.is_dir) for e in z.entries] == [("a", 1, False), ("d", 0, True), ("b", 15, False)]


def test_cover_and_layout_through_the_abi(xlz_so):
    arc, folders, entries = _archive()
    with lzma_amd.SevenZipFile(arc) as z:
        sizes = [len(x) for x in SOLID]
        solid_len, pack0, pack1 = sum(sizes), z.folders[0]["pack_len"], z.folders[1]["pack_len"]
        units = lzma_amd.lzma2_units(arc[z.folders[1]["pack_off"]:z.folders[1]["pack_off"] + pack1])
        assert [u["out_len"] for u in units] == [len(p) for p in PARTS]
        # an LZMA folder is cut where the last wanted file ends: 1 byte, odd offsets, whole for the last file
        assert z.cover("plain.txt") == [(0, 1, pack0)]
        assert z.cover([2, 1]) == [(0, 16, pack0)] and z.cover([3]) == [(0, 33, pack0)]
        assert z.cover("zeros") == [(0, 33 + 4097, pack0)] and z.cover("big.bin") == [(0, solid_len, pack0)]
        # an LZMA2 folder of several units: at the end of the unit that holds the last byte, input and output
        assert z.cover("p0") == [(1, 3000, units[1]["in_off"])] and z.cover("p1") == [(1, 8000, units[2]["in_off"])]
        assert z.cover("p2") == [(1, 13120, pack1)]
        # a Copy folder is never cut; entries without bytes need no folder; ascending and duplicate-free
        assert z.cover("c0") == [(2, 12, 12)] and z.cover(["top", 4, "gone"]) == [] and z.cover([]) == []
        assert z.cover(["c1", "p0", 1, "p0", 1]) == [(0, 1, pack0), (1, 3000, units[1]["in_off"]), (2, 12, 12)]
        with pytest.raises(lzma_amd.LzmaError) as ei:
            z.cover([len(z.entries)])
        assert ei.value.status == lzma_amd.ERR_BAD_ARG
        # the count protocol: NULL / 0 counts, a short array is XLZ_ERR_OUT_CAP with the full count
        L = N.lib()
        idx = (ctypes.c_uint64 * 3)(1, 8, 11)
        n = ctypes.c_size_t()
        assert L.xlz_7z_cover(z._h, idx, 3, None, 0, ctypes.byref(n)) == lzma_amd.OK and n.value == 3
        items = (N.SzCoverItem * 2)()
        assert L.xlz_7z_cover(z._h, idx, 3, items, 2, ctypes.byref(n)) == lzma_amd.ERR_OUT_CAP and n.value == 3
        assert (items[1].folder, items[1].decode_len) == (1, 3000)
        ents = (N.SzEntry * 3)()
        assert L.xlz_7z_archive_entries(z._h, ents, 3, None, 0) == lzma_amd.ERR_OUT_CAP and ents[1].size == 1
        fo = (N.SzFolder * 1)()
        assert L.xlz_7z_archive_folders(z._h, fo, 1) == lzma_amd.ERR_OUT_CAP and fo[0].unpack_len == solid_len
        assert L.xlz_7z_archive_info(None, None, None, None, None) == lzma_amd.ERR_BAD_ARG
        # the layout: sizes back to back, aligned
        assert z.layout([1, 2, "top", 3]) == ([(1, 0, 1), (2, 1, 15), (0, 16, 0), (3, 16, 17)], 33)
        assert z.layout([1, 2, 3], align=16) == ([(1, 0, 1), (2, 16, 15), (3, 32, 17)], 49)
        for bad, st in (((len(z.entries),), lzma_amd.ERR_BAD_ARG),):
            with pytest.raises(lzma_amd.LzmaError) as ei:
                z.layout(list(bad))
            assert ei.value.status == st
        total = ctypes.c_uint64(5)
        w = z._wants([(1, 0, 0)])
        assert L.xlz_7z_extract_layout(z._h, w, 1, 0, ctypes.byref(total)) == lzma_amd.ERR_BAD_ARG
        assert L.xlz_7z_extract_layout(z._h, w, 1, 1 << 63, ctypes.byref(total)) == lzma_amd.OK and total.value == 1
        w = z._wants([(1, 0, 0), (2, 0, 0), (3, 0, 0)])
        assert L.xlz_7z_extract_layout(z._h, w, 3, 1 << 63, ctypes.byref(total)) == lzma_amd.ERR_OUT_CAP and total.value == 0


def test_an_lzma2_folder_of_one_unit_is_cut_by_capacity(xlz_so):
    rec, pk = C.lzma2_folder(b"".join(SOLID))
    arc = F.archive([B.plain_folder(rec, pk, SOLID)], [F.entry("f%d" % i) for i in range(len(SOLID))])
    assert len(lzma_amd.lzma2_units(pk)) == 1
    with lzma_amd.SevenZipFile(arc) as z:
        assert z.cover(0) == [(0, 1, len(pk))] and z.cover(2) == [(0, 33, len(pk))] and z.cover(4) == [(0, len(b"".join(SOLID)), len(pk))]


def test_bad_arguments_are_settled_before_the_context_is_used(xlz_so):
    """the whole XLZ_ERR_BAD_ARG list with ctx == NULL: nothing is written, results[] included"""
    arc, _, _ = _archive()
    L = N.lib()
    with lzma_amd.SevenZipFile(arc) as z:
        out = ctypes.create_string_buffer(b"\xa5" * 64, 64)
        for name in ("xlz_7z_extract", "xlz_7z_extract_device"):
            fn = getattr(L, name)

            def call(wants, n=None, dst=out, cap=64, results=True, arch=z._h):
                res = (N.SzFileResult * max(len(wants), 1))()
                for r in res:
                    r.status, r.out_len = 77, 77
                st = fn(None, arch, z._wants(wants) if wants is not None else None, len(wants) if n is None else n,
                        ctypes.cast(dst, ctypes.c_void_p) if dst is not None else None, cap, 1, res if results else None)
                assert all(r.status == 77 and r.out_len == 77 for r in res) and out.raw == b"\xa5" * 64
                return st
            assert call([]) == lzma_amd.OK  # an empty want list: nothing to do, no context needed
            assert call([(1, 0, 1)], results=False) == lzma_amd.ERR_BAD_ARG
            assert call([(1, 0, 1)], arch=None) == lzma_amd.ERR_BAD_ARG
            assert fn(None, z._h, None, 1, ctypes.cast(out, ctypes.c_void_p), 64, 1, (N.SzFileResult * 1)()) == lzma_amd.ERR_BAD_ARG
            assert call([(1, 0, 1)], dst=None) == lzma_amd.ERR_BAD_ARG
            assert call([(len(z.entries), 0, 1)]) == lzma_amd.ERR_BAD_ARG            # an entry outside the table
            assert call([(1, 64, 1)]) == lzma_amd.ERR_BAD_ARG                        # a window that does not fit
            assert call([(1, 2 ** 64 - 1, 2)]) == lzma_amd.ERR_BAD_ARG               # ... and no sum is formed
            assert call([(2, 0, 15), (3, 14, 17)]) == lzma_amd.ERR_BAD_ARG           # two windows share a byte
            assert call([(2, 0, 15), (2, 10, 15)]) == lzma_amd.ERR_BAD_ARG           # the same entry twice, overlapping
            # a well-formed call is refused for its missing context, with nothing written either (that the windows of
            # entries without bytes declare nothing takes a real context to tell: tests/test_gpu_sevenzip_files.py::test_windows)
            assert call([(2, 0, 15), (3, 15, 17)]) == lzma_amd.ERR_BAD_ARG
        stats = N.SzExtractStats()
        assert L.xlz_ctx_last_7z_extract_stats(None, ctypes.byref(stats)) == lzma_amd.ERR_BAD_ARG


def test_what_a_cut_stream_ends_in_is_the_oracles_outcome():
    """The three kinds of xlz_7z_files.h, each with ONE outcome (status, out_len, in_consumed) in the CPU oracle: a folder cut
    by capacity -- LZMA, and LZMA2 of one unit -- ends in XLZ_ERR_OUT_CAP with out_len == out_cap (as
    test_oracle_golden.py::test_out_cap_too_small); an LZMA2 folder cut behind a unit, input too, ends in
    XLZ_ERR_UNEXPECTED_EOF with exactly the units' bytes and ALL of the cut input used.  The bytes are the folder's."""
    data = b"".join(SOLID)
    _, pk = C.lzma_folder(data)
    for cap in (1, 16, 33, 33 + 4097 - 1000, 33 + 4097, len(data) - 1):  # (a cut of one byte; inside the long run of zeros)
        out, st, _ = oracle.lzma1_raw(0x5D, 1 << 16, len(data), pk, cap)
        assert (st, out) == (oracle.ERR_OUT_CAP, data[:cap]), cap
    out, st, ic = oracle.lzma1_raw(0x5D, 1 << 16, len(data), pk, len(data))
    assert (st, out) == (oracle.OK, data)
    _, pk = C.lzma2_folder(data)
    for cap in (1, 33, 4000, len(data) - 1):
        out, st, _ = oracle.lzma2_raw(pk, 1 << 16, cap)
        assert (st, out) == (oracle.ERR_OUT_CAP, data[:cap]), cap
    _, pk = F.lzma2_units_folder(PARTS)
    units = lzma_amd.lzma2_units(pk)
    assert len(units) == 3
    whole = b"".join(PARTS)
    for k in (1, 2):
        end_in, end_out = units[k]["in_off"], units[k]["out_off"]
        out, st, ic = oracle.lzma2_raw(pk[:end_in], 1 << 17, end_out)
        assert (st, out, ic) == (oracle.ERR_UNEXPECTED_EOF, whole[:end_out], end_in), k
    assert oracle.lzma2_raw(pk, 1 << 17, len(whole))[:2] == (whole, oracle.OK)
    assert (lzma_amd.ERR_OUT_CAP, lzma_amd.ERR_UNEXPECTED_EOF) == (oracle.ERR_OUT_CAP, oracle.ERR_UNEXPECTED_EOF)


SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.mark.parametrize("flags", [["-O2"], SAN], ids=["plain", "asan_ubsan"])
def test_the_shared_header_against_brute_force_models(tmp_path, flags):
    exe = str(tmp_path / "sevenzip_files_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "lzma_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "sevenzip_files_selftest.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


def test_mutated_headers_through_open_under_the_sanitizers(tmp_path):
    """tests/c/sevenzip_files_fuzz.cpp: the parser compiled into a stand-alone program with AddressSanitizer and UBSan,
    4 x 15 000 headers; both outcomes must occur"""
    seeds = {"files": _archive()[0], "nameless": C.archive([C.lzma_folder(SOLID[1]) + ([SOLID[1]],)]),
             "empty_only": F.archive([], [F.entry("d", "dir", mtime=F.filetime(5)), F.entry("e", "empty", attr=1)]),
             "libarchive": sevenzip_read.with_plain_header(open(os.path.join(GOLDEN, "libarchive_solid.7z"), "rb").read())}
    paths = []
    for name, a in seeds.items():
        paths.append(str(tmp_path / (name + ".7z")))
        open(paths[-1], "wb").write(a)
    exe = str(tmp_path / "sevenzip_files_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-x", "c++"] + SAN + ["-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "sevenzip_files_fuzz.cpp"), "-o", exe])
    out = subprocess.run([exe, "15000"] + paths, capture_output=True, text=True, timeout=55)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    words = out.stdout.split()
    opened, refused = int(words[words.index("opened,") - 1]), int(words[words.index("refused,") - 1])
    assert opened > 100 and refused > 100, out.stdout
