"""CPU: BCJ2 folders without a GPU.  xlz_bcj2_host (the serial merge, lzma_amd/csrc/xlz_bcj2_dev.h: host_merge) against
tests/bcj2_ref.py on machine code, random bytes, runs of candidates, short inputs and the edge cases of the format's
statement; xlz_7z_index_bcj2 on both folder forms and on the folders it must refuse; cmake's bundled libarchive as the
independent judge of the four-coder layout."""
import lzma
import random
import shutil
import subprocess
import zlib

import pytest

import bcj2_ref as B
import filter_ref as R
import lzma_amd
import sevenzip_bcj2 as Z
import sevenzip_craft
from lzma_amd import _native as N


def _host(streams, out_len):
    """-> (status, bytes or None)"""
    try:
        return lzma_amd.OK, lzma_amd.bcj2_host(*streams, out_len)
    except lzma_amd.LzmaError as e:
        return e.status, None


def _round_trip(data, convert=None):
    streams = B.encode(data, convert)
    st, ref = B.decode(*streams, len(data))
    assert st == B.OK and ref == data
    assert _host(streams, len(data)) == (lzma_amd.OK, data)
    return streams


def _inputs():
    rnd = random.Random(7)
    yield "machine code", R.machine_code(200_000)
    yield "random", rnd.randbytes(50_000)
    yield "soup", R.opcode_soup(50_000, 3)
    yield "adversarial", R.x86_adversarial(30_000, 5, 30, runs=True)
    yield "E8 x 4096", b"\xE8" * 4096
    yield "0F 8x runs", b"".join(bytes([0x0F, 0x80 | (k & 15)]) for k in range(3000))
    for n in (0, 1, 4, 5, 6):
        yield "length %d" % n, bytes([0xE8, 1, 0, 0, 0, 0x90])[:n]
        yield "length %d plain" % n, bytes(range(n))


@pytest.mark.parametrize("name,data", list(_inputs()), ids=[n for n, _ in _inputs()])
def test_host_merge_round_trips_and_equals_the_reference(xlz_so, name, data):
    main, call, jump, rc = _round_trip(data)
    if name in ("machine code", "soup", "adversarial"):
        assert call and len(main) + len(call) + len(jump) == len(data)  # conversions happened


def test_candidates_at_the_end(xlz_so):
    for lead in (0, 3, 1023):
        for op in (b"\xE8", b"\xE9", b"\x0F\x85"):
            for behind in range(0, 6):
                data = bytes(k % 0xE0 for k in range(lead)) + op + bytes(behind)
                main, call, jump, rc = _round_trip(data)
                assert (len(call) + len(jump) == 4) == (behind >= 4)  # four bytes follow: converted (top byte 00)


def test_the_prev_trap(xlz_so):
    """a conversion whose dest has top byte 0F, followed by 80: a candidate that a scan of the main stream does not see"""
    for lead in (0, 5, 1023, 1024):
        data, at = B.trap_data(lead)
        main, call, jump, rc = _round_trip(data, B.convert_0f_too)
        # the case really occurs: E8 and 80 lie side by side in the MAIN stream (E8 is not 0F), and both were converted
        assert main[at] == 0xE8 and main[at + 1] == 0x80 and len(call) == 4 and len(jump) == 4
        assert int.from_bytes(data[at + 1: at + 5], "little") >> 24 == 0x0F
        assert not B.is_j(main[at], main[at + 1]) and B.is_j(0x0F, main[at + 1])
        # without the re-test the 80's operand would stay in the jump stream: the output would be four bytes short
        assert len(main) == len(data) - 8


def test_a_bit_1_decision_with_less_than_four_bytes_of_room(xlz_so):
    data = bytes(range(100)) + b"\xE8\x10\x00\x00\x00"
    streams = B.encode(data)
    assert len(streams[1]) == 4
    for cut in (1, 2, 3):  # part of the operand is written, and that is OK
        assert B.decode(*streams, len(data) - cut) == (B.OK, data[:-cut])
        assert _host(streams, len(data) - cut) == (lzma_amd.OK, data[:-cut])
    assert _host(streams, len(data) - 4) == (lzma_amd.OK, data[:-4])  # the candidate is the last byte: no bit is read
    assert _host(streams, len(data) - 5) == (lzma_amd.OK, data[:-5])


def test_damaged_streams_are_result_errors(xlz_so):
    data = R.machine_code(40_000)
    main, call, jump, rc = B.encode(data)
    assert len(call) >= 8 and len(jump) >= 8
    bad = [(main[:-1], call, jump, rc), (main, call[:-1], jump, rc), (main, call[:len(call) // 8 * 4], jump, rc),
           (main, call, jump[:-4], rc), (main, call, jump, rc[:4]), (main, call, jump, rc[:len(rc) // 2]), (main, call, jump, b"")]
    for s in bad:
        assert B.decode(*s, len(data))[0] == B.ERR_RESULT
        assert _host(s, len(data))[0] == lzma_amd.ERR_RESULT
    assert _host((main, call, jump, rc), len(data) + 1)[0] == lzma_amd.ERR_RESULT  # the streams do not fill the output
    assert _host((b"", b"", b"", b""), 0) == (lzma_amd.OK, b"")
    assert N.lib().xlz_bcj2_host(None, 1, None, 0, None, 0, None, 0, None, 0) == lzma_amd.ERR_BAD_ARG


def _files():
    code = R.machine_code(60_000)
    return [code[:777], code[777:]]


def _lzma_raw(blob, sub):
    filt = {"id": lzma.FILTER_LZMA2, "dict_size": sub["dict_size"]} if sub["method"] == 2 else \
        {"id": lzma.FILTER_LZMA1, "dict_size": sub["dict_size"], "lc": 3, "lp": 0, "pb": 2}
    return lzma.decompress(blob, format=lzma.FORMAT_RAW, filters=[filt])


def _streams_of(arch, rec):
    """the four streams of a BCJ2 record, the coded ones decoded by liblzma"""
    out = []
    for key in ("main", "call", "jump"):
        sub = rec[key]
        blob = arch[sub["pack_off"]: sub["pack_off"] + sub["pack_len"]]
        out.append(blob if sub["method"] == 3 else _lzma_raw(blob, sub))
        assert len(out[-1]) == sub["unpack_len"]
    return out + [arch[rec["rc_off"]: rec["rc_off"] + rec["rc_len"]]]


@pytest.mark.parametrize("form,layout,lzma2", [(4, "libarchive", False), (4, "libarchive", True), (4, "7zip", False), (4, "7zip", True),
                                               (2, "", False), (2, "", True)])
def test_index_places_every_stream(xlz_so, form, layout, lzma2):
    files = _files()
    data = b"".join(files)
    text = R.text(9000)
    folders = [Z.plain_folder(*sevenzip_craft.lzma_folder(text), [text]), Z.bcj2_folder(files, form, lzma2, layout),
               Z.plain_folder(*sevenzip_craft.copy_folder(text[:100]), [text[:100]])]
    arch = Z.archive(folders)
    fo, subs, steps, recs, total = lzma_amd.sevenzip_index_bcj2(arch)
    assert [f["method"] for f in fo] == [1, N.SZ_BCJ2, 3] and total == len(text) + len(data) + 100 and steps == []
    f = fo[1]
    assert f["unpack_len"] == len(data) and f["unpack_off"] == len(text) and f["n_substreams"] == 2
    assert f["has_crc"] and f["crc"] == zlib.crc32(data)
    assert subs[1:3] == [(777, zlib.crc32(files[0])), (len(data) - 777, zlib.crc32(files[1]))]
    assert len(recs) == 1 and recs[0]["folder"] == 1
    want = 2 if lzma2 else 1
    assert recs[0]["main"]["method"] == want
    assert [recs[0][k]["method"] for k in ("call", "jump")] == ([want, want] if form == 4 else [3, 3])
    if not lzma2:
        assert recs[0]["main"]["dict_size"] == 1 << 18 and recs[0]["main"]["props"] == 0x5D
    streams = _streams_of(arch, recs[0])
    assert tuple(streams) == folders[1]["streams"]
    assert lzma_amd.bcj2_host(*streams, len(data)) == data
    # the older index calls: the same archive, the BCJ2 folder as method 0.  (They take the size the folder's LAST coder
    # announces for the folder's, as ever: where BCJ2 is listed first that is the jump stream's, smaller than the files of
    # this solid folder, and they answer ERR_RESULT as they always did.)
    if layout == "7zip":
        for index in (lzma_amd.sevenzip_index, lzma_amd.sevenzip_index_chains):
            with pytest.raises(lzma_amd.LzmaError) as e:
                index(arch)
            assert e.value.status == lzma_amd.ERR_RESULT
    else:
        fo0, _, _ = lzma_amd.sevenzip_index(arch)
        foc, _, _, _ = lzma_amd.sevenzip_index_chains(arch)
        assert [f["method"] for f in fo0] == [1, 0, 3] == [f["method"] for f in foc]


def test_folders_that_are_neither_form_stay_unsupported(xlz_so):
    files = [R.machine_code(20_000)]

    def method(**kw):
        fo, _, _, recs, _ = lzma_amd.sevenzip_index_bcj2(Z.archive([Z.bcj2_folder(files, **kw)]))
        assert len(recs) == (fo[0]["method"] == N.SZ_BCJ2)
        return fo[0]["method"]

    assert method() == N.SZ_BCJ2 and method(form=2) == N.SZ_BCJ2
    assert method(binds=[(5, 0), (5, 1), (3, 2)]) == 0                     # an input bound twice
    assert method(binds=[(5, 0), (4, 0), (3, 2)]) == 0                     # an output bound twice
    assert method(binds=[(5, 0), (4, 1), (6, 2)], index=[2, 3, 1, 0]) == 0  # rc fed by a coder
    assert method(binds=[(5, 0), (4, 1), (2, 3)], index=[3, 6, 1, 0]) == 0  # BCJ2's output bound: a filter behind BCJ2
    assert method(index=[2, 6, 1, 1]) == 0                                 # a packed stream named twice
    assert method(index=[2, 6, 1, 5]) == 0                                 # a packed stream into a bound input
    assert method(bcj2_coder=bytes([0x34]) + b"\x03\x03\x01\x1b" + Z.number(4) + Z.number(1) + Z.number(1) + b"\0") == 0  # properties
    assert method(bcj2_coder=bytes([0x14]) + b"\x03\x03\x01\x03" + Z.number(4) + Z.number(1)) == 0  # not BCJ2's id
    assert method(main_coder=bytes([0x01]) + b"\x00") == 0                 # a sub-coder that is neither LZMA nor LZMA2 (Copy)
    assert method(main_coder=bytes([0x04]) + b"\x03\x03\x01\x03") == 0     # ... (x86: a filter in front of BCJ2)
    assert method(form=2, binds=[(2, 0)], index=[0, 1, 3, 4]) == 0         # two coders: the coder must feed the main stream
    # BCJ2 with other stream counts: three inputs
    assert method(form=2, bcj2_coder=bytes([0x14]) + b"\x03\x03\x01\x1b" + Z.number(3) + Z.number(1), index=[0, 2, 3]) == 0
    # a call / jump size that is no multiple of 4
    main, call, jump, rc = B.encode(files[0])
    assert method(streams=(main, call + b"\0", jump, rc)) == 0
    assert method(form=2, streams=(main, call, jump + b"\0\0", rc)) == 0


def test_new_entry_points_need_their_objects(xlz_so):
    L = N.lib()
    item, res = (N.Bcj2Item * 1)(), (N.Bcj2Result * 1)()
    assert L.xlz_batch_bcj2(None, item, 1, None, 0, res) == lzma_amd.ERR_BAD_ARG
    assert L.xlz_ctx_set_bcj2_mode(None, 1) == lzma_amd.ERR_BAD_ARG and L.xlz_ctx_bcj2_mode(None) == lzma_amd.ERR_BAD_ARG
    assert L.xlz_ctx_last_bcj2_stats(None, None) == lzma_amd.ERR_BAD_ARG
    assert L.xlz_7z_index_bcj2(None, None, 0, None, 0, None, None, 0, None, None, 0, None, None, 0, None, None) == lzma_amd.ERR_BAD_ARG


def test_cmake_extracts_the_four_coder_layout(xlz_so, tmp_path):
    """cmake's bundled libarchive reads BCJ2 folders of the layout tests/sevenzip_bcj2.py calls "libarchive".  Its bytes must
    be the files, and xlz_bcj2_host over the liblzma-decoded streams of the index must give the same.  This layout MUST
    extract: an archive that stops extracting fails, it does not skip."""
    if not shutil.which("cmake"):
        pytest.skip("no cmake on this box: nothing here extracts a .7z archive")
    code = R.machine_code(300_000)
    files = [code[:100_001], code[100_001:]]
    arch = Z.archive([Z.bcj2_folder(files, 4, False, "libarchive")], names=["a.bin", "b.bin"])
    (tmp_path / "x.7z").write_bytes(arch)
    r = subprocess.run(["cmake", "-E", "tar", "xf", "x.7z"], cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stdout + r.stderr
    got = (tmp_path / "a.bin").read_bytes() + (tmp_path / "b.bin").read_bytes()
    assert (tmp_path / "a.bin").read_bytes() == files[0] and got == code
    _, _, _, recs, _ = lzma_amd.sevenzip_index_bcj2(arch)
    assert lzma_amd.bcj2_host(*_streams_of(arch, recs[0]), len(code)) == got
