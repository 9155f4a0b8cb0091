"""CPU: the table of a .zip archive (include/xlz.h: xlz_zip_open / xlz_zip_archive_* / xlz_zip_extract_layout) and what an
extraction settles before it uses its context.  The archives are written by tests/zip_files.py -- with Python's zipfile,
by hand from PKWARE's APPNOTE, and once by Info-ZIP (tests/golden/infozip.zip) --; zipfile's own listing is the
independent judge of the table, Python's lzma of where a method-14 payload begins.  The shared header
(lzma_amd/csrc/xlz_zip.h) runs in a g++ program of its own against brute-force models, and a stand-alone fuzz program
mutates archives through xlz_zip_open; both plain and under the host sanitizers."""
import ctypes
import io
import lzma
import os
import subprocess
import sys
import zipfile
import zlib

import pytest

import lzma_amd
from lzma_amd import _native as N

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zip_files as Z  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _archives():
    out = {"mixed": Z.mixed(), "descriptors": Z.descriptors(), "forced_zip64": Z.forced_zip64(), "residues": Z.residues()[0],
           "damaged": Z.damaged()[0], "both_markers": Z.both_markers()[0]}
    out.update(Z.end_variants())
    return out


@pytest.mark.parametrize("which", sorted(_archives()))
def test_the_table_is_what_zipfile_lists(xlz_so, which):
    arc = _archives()[which]
    with zipfile.ZipFile(io.BytesIO(arc)) as judge, lzma_amd.ZipFile(arc) as z:
        infos = judge.infolist()
        assert len(z.entries) == len(infos)
        shift = z.shift
        assert shift == (1000 if which.startswith("prepended") else 0)
        for e, zi in zip(z.entries, infos):
            assert (e["name"], e["size"], e["comp_size"], e["crc"], e["method"], e["gp_flags"], e["mtime"], e["external_attr"]) == \
                   (zi.filename, zi.file_size, zi.compress_size, zi.CRC, zi.compress_type, zi.flag_bits, zi.date_time, zi.external_attr), zi.filename
            # (zipfile has added what lies in front of the archive to header_offset already: ZipInfo.header_offset + the shift
            #  of an archive it read as if nothing lay in front)
            assert e["header_off"] == zi.header_offset
            assert e["is_dir"] == zi.is_dir()
            assert bool(e["flags"] & N.ZIP_ENTRY_UTF8) == bool(zi.flag_bits & 0x800)
            assert bool(e["flags"] & N.ZIP_ENTRY_HAS_DESCRIPTOR) == bool(zi.flag_bits & 8)
            if e["bad"] or not e["supported"] or not e["size"] or (which == "damaged" and not zi.filename.startswith("good")):
                continue
            # data_off: a stored entry's bytes lie there; a method-14 payload decodes from data_off + 9 with Python's lzma
            body = arc[e["data_off"]:e["data_off"] + e["comp_size"]]
            if e["method"] == 0:
                assert body == judge.read(zi)
            else:
                lc, rest = e["props"] % 9, e["props"] // 9
                flt = [{"id": lzma.FILTER_LZMA1, "dict_size": max(e["dict_size"], 4096), "lc": lc, "lp": rest % 5, "pb": rest // 5}]
                d = lzma.LZMADecompressor(lzma.FORMAT_RAW, filters=flt)
                assert d.decompress(body[9:], e["size"]) == judge.read(zi), zi.filename
        assert z.total_size == sum(zi.file_size for zi in infos if not zi.is_dir())
        assert z.names == [zi.filename for zi in infos]
    assert "世界" in lzma_amd.ZipFile(Z.mixed()).names[-1]


def test_the_local_header_decides_where_the_data_begins():
    arc, _ = Z.residues()
    with lzma_amd.ZipFile(arc) as z:
        for i, e in enumerate(z.entries):  # the local extra field is 4 + i % 5 bytes, the central one 0 or 4
            assert e["data_off"] == e["header_off"] + 30 + len(e["name"]) + 4 + i % 5
    with lzma_amd.ZipFile(Z.descriptors()) as z:  # local headers that hold zeros: sizes and CRC are the central directory's
        assert all(e["size"] and e["crc"] and e["flags"] & N.ZIP_ENTRY_HAS_DESCRIPTOR for e in z.entries)
        assert all(Z.descriptors()[e["header_off"] + 14:e["header_off"] + 26] == b"\0" * 12 for e in z.entries)


def test_65537_stored_entries_go_through_the_zip64_end_record():
    arc, plain = Z.many_stored(65537)
    assert arc[-22 - 20:-22 - 16] == b"PK\x06\x07" and arc[-22 + 8:-22 + 12] == b"\xff\xff\xff\xff"
    with lzma_amd.ZipFile(arc) as z, zipfile.ZipFile(io.BytesIO(arc)) as judge:
        infos = judge.infolist()
        assert len(z.entries) == len(infos) == 65537
        assert [(e["name"], e["header_off"], e["crc"]) for e in z.entries] == [(zi.filename, zi.header_offset, zi.CRC) for zi in infos]
        assert all(e["supported"] and e["size"] == 1 for e in z.entries) and z.total_size == 65537
        assert all(arc[e["data_off"]:e["data_off"] + 1] == p for e, p in zip(z.entries[::997], plain[::997]))


def test_the_info_zip_archive_is_read_as_its_recipe_wrote_it():
    """Info-ZIP's zip -fz -fd: ZIP64 extra fields everywhere, data descriptors on the deflate entries, and an all-ones
    directory offset that no ZIP64 end record explains (zipfile refuses the archive)"""
    sys.path.insert(0, Z.GOLDEN)
    import make_infozip_zip as R
    arc = Z.infozip()
    assert len(arc) < 8192
    with pytest.raises(Exception):
        zipfile.ZipFile(io.BytesIO(arc)).testzip()
    with lzma_amd.ZipFile(arc) as z:
        assert z.shift == 0 and z.names == ["sub/"] + sorted(R.STORED) + sorted(R.DEFLATED)
        by_name = dict(zip(z.names, z.entries))
        assert all(e["flags"] & N.ZIP_ENTRY_ZIP64 for e in z.entries)
        for name, data in R.STORED.items():
            e = by_name[name]
            assert (e["method"], e["size"], e["comp_size"], e["crc"], e["supported"]) == (0, len(data), len(data), zlib.crc32(data), True)
            assert arc[e["data_off"]:e["data_off"] + e["size"]] == data
        for name, data in R.DEFLATED.items():
            e = by_name[name]
            assert (e["method"], e["size"], e["crc"], e["supported"], e["bad"]) == (8, len(data), zlib.crc32(data), False, False)
            assert e["flags"] & N.ZIP_ENTRY_HAS_DESCRIPTOR
            assert zlib.decompress(arc[e["data_off"]:e["data_off"] + e["comp_size"]], -15) == data
        assert by_name["sub/"]["is_dir"] and by_name["sub/stored_1000.bin"]["mtime"] == (2024, 2, 29, 13, 37, 42)


def test_each_defect_lands_in_its_class_and_never_fails_open():
    arc, what, _ = Z.damaged()
    with lzma_amd.ZipFile(arc) as z:
        for name, (i, kind) in what.items():
            e = z.entries[i]
            assert e["name"] == name
            want = {"unsupported": (False, False), "bad": (False, True)}.get(kind, (True, False))  # (damage inside a payload is not seen at open)
            assert (e["supported"], e["bad"]) == want, name
        assert z.entries[what["encrypted"][0]]["flags"] & N.ZIP_ENTRY_ENCRYPTED
        assert z.entries[what["offset_out"][0]]["data_off"] == z.entries[what["no_local_sig"][0]]["data_off"] == 0
        assert z.entries[what["data_out"][0]]["data_off"] != 0
        assert all(e["supported"] for e in z.entries if e["name"].startswith("good"))
    # flag bits 5 (patched data) and 6 (strong encryption), a method of 4 GiB: unsupported; a directory has no bytes whatever it says
    h = Z.Hand()
    h.stored("patched", b"abc", flags=1 << 5)
    h.stored("strong", b"abc", flags=1 << 6)
    h.add("huge", Z.lzma_payload(Z.text(1, 300)), 0xFFFF0001, 0, 14, flags=2, zip64=True)
    h.add("almost", b"", 0xFFFF0000, 0, 0, zip64=True, comp_size=0xFFFF0000)
    h.add("dir/", b"xyz", 3, 0, 8)
    with lzma_amd.ZipFile(h.finish()) as z:
        assert [(e["supported"], e["bad"]) for e in z.entries] == [(False, False)] * 3 + [(False, True), (False, False)]
        assert z.layout([4, 0]) == ([(4, 0, 0), (0, 0, 3)], 3) and z.total_size == 3 + 3 + 0xFFFF0001 + 0xFFFF0000


@pytest.mark.parametrize("which", sorted(Z.end_defects()))
def test_each_end_record_defect_fails_open_with_its_status(xlz_so, which):
    arc, status = Z.end_defects()[which]
    with pytest.raises(lzma_amd.LzmaError) as ei:
        lzma_amd.ZipFile(arc)
    assert ei.value.status == getattr(lzma_amd, status)
    h = ctypes.c_void_p(5)
    buf = ctypes.create_string_buffer(arc, max(len(arc), 1))
    assert N.lib().xlz_zip_open(ctypes.cast(buf, ctypes.c_void_p), len(arc), ctypes.byref(h)) == getattr(lzma_amd, status) and not h.value


def test_layout_arithmetic_and_the_count_protocol(xlz_so):
    L = N.lib()
    with lzma_amd.ZipFile(Z.mixed()) as z:
        i1, i15, i17, d = z.index("dir/lzma_1.txt"), z.index("s15.bin"), z.index("dir/lzma_17.txt"), z.index("dir/")
        assert z.layout([i1, i15, d, i17]) == ([(i1, 0, 1), (i15, 1, 15), (d, 16, 0), (i17, 16, 17)], 33)
        assert z.layout([i1, i15, i17], align=16) == ([(i1, 0, 1), (i15, 16, 15), (i17, 32, 17)], 49)
        assert z.layout([]) == ([], 0)
        with pytest.raises(lzma_amd.LzmaError) as ei:
            z.layout([len(z.entries)])
        assert ei.value.status == lzma_amd.ERR_BAD_ARG
        with pytest.raises(KeyError):
            z.index("no such name")
        total = ctypes.c_uint64(5)
        w = z._wants([(i1, 0, 0)])
        assert L.xlz_zip_extract_layout(z._h, w, 1, 0, ctypes.byref(total)) == lzma_amd.ERR_BAD_ARG
        assert L.xlz_zip_extract_layout(z._h, w, 1, 1 << 63, ctypes.byref(total)) == lzma_amd.OK and total.value == 1
        w = z._wants([(i1, 0, 0), (i15, 0, 0), (i17, 0, 0)])
        assert L.xlz_zip_extract_layout(z._h, w, 3, 1 << 63, ctypes.byref(total)) == lzma_amd.ERR_OUT_CAP and total.value == 0
        assert L.xlz_zip_extract_layout(None, w, 3, 1, ctypes.byref(total)) == lzma_amd.ERR_BAD_ARG
        # NULL / 0 counts; a short array is XLZ_ERR_OUT_CAP with what fits
        ne, nb, tot, shift = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_uint64(), ctypes.c_uint64()
        assert L.xlz_zip_archive_info(z._h, ctypes.byref(ne), ctypes.byref(nb), ctypes.byref(tot), ctypes.byref(shift)) == lzma_amd.OK
        assert (ne.value, tot.value, shift.value) == (len(z.entries), z.total_size, 0)
        assert nb.value == sum(len(zi.filename.encode()) + 1 for zi in zipfile.ZipFile(io.BytesIO(Z.mixed())).infolist())
        assert L.xlz_zip_archive_info(z._h, None, None, None, None) == lzma_amd.OK
        assert L.xlz_zip_archive_info(None, None, None, None, None) == lzma_amd.ERR_BAD_ARG
        ents = (N.ZipEntry * 3)()
        assert L.xlz_zip_archive_entries(z._h, ents, 3, None, 0) == lzma_amd.ERR_OUT_CAP and ents[2].size == z.entries[2]["size"]
        assert ctypes.sizeof(N.ZipEntry) == 72 and ctypes.sizeof(N.ZipExtractStats) == 64
    assert N.lib().xlz_zip_open(None, 0, None) == lzma_amd.ERR_BAD_ARG
    z = lzma_amd.ZipFile(Z.mixed())
    z.close()
    z.close()
    with pytest.raises(lzma_amd.LzmaError) as ei:
        z.layout([0])
    assert ei.value.status == lzma_amd.ERR_CLOSED


def test_bad_arguments_are_settled_before_the_context_is_used(xlz_so):
    """the whole XLZ_ERR_BAD_ARG list with ctx == NULL: nothing is written, results[] included"""
    L = N.lib()
    with lzma_amd.ZipFile(Z.mixed()) as z:
        i1, i15, i17, d = z.index("dir/lzma_1.txt"), z.index("s15.bin"), z.index("dir/lzma_17.txt"), z.index("dir/")
        for fn in (L.xlz_zip_extract, L.xlz_zip_extract_device):
            def call(wants, dst=True, results=True, arch=z._h, cap=64):
                out = ctypes.create_string_buffer(b"\xa5" * 64, 64)
                res = (N.ZipFileResult * 4)()
                for r in res:
                    r.status, r.out_len = 77, 77
                st = fn(None, arch, z._wants(wants), len(wants), ctypes.cast(out, ctypes.c_void_p) if dst else None, cap, 1,
                        res if results else None)
                assert all(r.status == 77 and r.out_len == 77 for r in res) and out.raw == b"\xa5" * 64
                return st
            assert call([]) == lzma_amd.OK  # an empty want list: nothing to do, no context needed
            assert call([(i1, 0, 1)], results=False) == lzma_amd.ERR_BAD_ARG
            assert call([(i1, 0, 1)], arch=None) == lzma_amd.ERR_BAD_ARG
            assert fn(None, z._h, None, 1, None, 64, 1, (N.ZipFileResult * 1)()) == lzma_amd.ERR_BAD_ARG
            assert call([(i1, 0, 1)], dst=False) == lzma_amd.ERR_BAD_ARG
            assert call([(len(z.entries), 0, 1)]) == lzma_amd.ERR_BAD_ARG            # an entry outside the table
            assert call([(i1, 64, 1)]) == lzma_amd.ERR_BAD_ARG                       # a window that does not fit
            assert call([(i1, 2 ** 64 - 1, 2)]) == lzma_amd.ERR_BAD_ARG              # ... and no sum is formed
            assert call([(i15, 0, 15), (i17, 14, 17)]) == lzma_amd.ERR_BAD_ARG       # two windows share a byte
            assert call([(i15, 0, 15), (i15, 10, 15)]) == lzma_amd.ERR_BAD_ARG       # the same entry twice, overlapping
            # a well-formed call is refused for its missing context, with nothing written either; the window of a
            # directory declares nothing, wherever it points
            assert call([(i15, 0, 15), (i17, 15, 17), (d, 2 ** 64 - 1, 5)]) == lzma_amd.ERR_BAD_ARG
        stats = N.ZipExtractStats()
        assert L.xlz_ctx_last_zip_extract_stats(None, ctypes.byref(stats)) == lzma_amd.ERR_BAD_ARG


SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.mark.parametrize("flags", [["-O2"], SAN], ids=["plain", "asan_ubsan"])
def test_the_shared_header_against_brute_force_models(tmp_path, flags):
    exe = str(tmp_path / "zip_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "lzma_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "zip_selftest.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


@pytest.mark.parametrize("flags,rounds", [(["-O2"], 20000), (SAN, 4000)], ids=["plain", "asan_ubsan"])
def test_mutated_archives_through_open_entries_and_layout(tmp_path, flags, rounds):
    """tests/c/zip_fuzz.cpp: the parser compiled into a stand-alone program with a fixed seed; a few seconds of byte
    mutations of the fixtures, every table walked and every payload read"""
    seeds = {"mixed": Z.mixed(), "damaged": Z.damaged()[0], "descriptors": Z.descriptors(), "infozip": Z.infozip(),
             "prepended_zip64": Z.end_variants()["prepended_1000_zip64"]}
    paths = []
    for name, a in seeds.items():
        paths.append(str(tmp_path / (name + ".zip")))
        open(paths[-1], "wb").write(a)
    exe = str(tmp_path / "zip_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-x", "c++", *flags, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "zip_fuzz.cpp"), "-o", exe])
    out = subprocess.run([exe, str(rounds)] + paths, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    words = out.stdout.split()
    opened, refused, bad = (int(words[words.index(w) - 1]) for w in ("opened,", "refused,", "bad"))
    assert opened > rounds and refused > rounds and bad > rounds, out.stdout
