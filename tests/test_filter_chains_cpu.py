"""CPU: the container front-ends' view of filter chains.  xz_index_chains against .xz files written by liblzma
(lzma.compress with each filter) and by tests/xz_chains.py (several blocks, concatenated streams, block headers liblzma
would not write); sevenzip_index_chains against archives of tests/sevenzip_chains.py, and against what `cmake -E tar xf`
(libarchive) extracts from them where it can.  No decode here: that needs the GPU (tests/test_gpu_filters.py)."""
import ctypes
import lzma
import os
import shutil
import struct
import subprocess
import zlib

import pytest

import filter_ref as R
import lzma_amd
import sevenzip_chains as Z
import xz_chains as X
from lzma_amd import _native as N

L2 = {"id": lzma.FILTER_LZMA2, "preset": 1}


def _status(fn, *args):
    try:
        fn(*args)
    except lzma_amd.LzmaError as e:
        return e.status
    return lzma_amd.OK


def test_xz_single_filters_written_by_liblzma(xlz_so):
    data = R.machine_code(150_000, 1)
    for fid in R.ALL:
        for prm in R.params(fid)[:2]:
            xz = lzma.compress(data, format=lzma.FORMAT_XZ, check=lzma.CHECK_CRC64, filters=[R.filter_dict(fid, prm), L2])
            assert _status(lzma_amd.xz_index, xz) == lzma_amd.ERR_UNSUPPORTED          # (the plain index keeps refusing it)
            blocks, steps, total = lzma_amd.xz_index_chains(xz)
            assert total == len(data) and len(blocks) == 1 and blocks[0]["check_type"] == 4
            assert steps == [(0, fid, prm)], (fid, prm)
            # the block's payload is raw LZMA2; the steps undo the chain
            b = blocks[0]
            raw = lzma.decompress(xz[b["comp_off"]: b["comp_off"] + b["comp_len"]], format=lzma.FORMAT_RAW,
                                  filters=[{"id": lzma.FILTER_LZMA2, "dict_size": max(b["dict_size"], 4096)}])
            assert R.apply_steps([(f, p) for _, f, p in steps], raw) == data
            assert lzma_amd.filter_host(fid, prm, raw) == data


def test_xz_plain_files_have_no_steps(xlz_so):
    xz = lzma.compress(b"plain " * 1000, format=lzma.FORMAT_XZ)
    blocks, steps, total = lzma_amd.xz_index_chains(xz)
    assert steps == [] and total == 6000 and blocks == lzma_amd.xz_index(xz)[0]


def test_xz_chains_of_two_and_three(xlz_so):
    data = R.machine_code(100_000, 0)
    for filters in ([{"id": lzma.FILTER_DELTA, "dist": 4}, {"id": lzma.FILTER_X86}, L2],
                    [{"id": lzma.FILTER_X86, "start_offset": 4096}, {"id": lzma.FILTER_DELTA, "dist": 256}, {"id": lzma.FILTER_ARM}, L2],
                    [{"id": lzma.FILTER_ARMTHUMB}, {"id": lzma.FILTER_IA64, "start_offset": 32}, {"id": lzma.FILTER_SPARC}, L2]):
        xz = lzma.compress(data, format=lzma.FORMAT_XZ, filters=filters)
        blocks, steps, total = lzma_amd.xz_index_chains(xz)
        want = X.decoder_steps([(data, filters)])
        assert steps == want and total == len(data)
        b = blocks[0]
        raw = lzma.decompress(xz[b["comp_off"]: b["comp_off"] + b["comp_len"]], format=lzma.FORMAT_RAW,
                              filters=[{"id": lzma.FILTER_LZMA2, "dict_size": max(b["dict_size"], 4096)}])
        got = raw
        for _, fid, prm in steps:
            got = lzma_amd.filter_host(fid, prm, got)
        assert got == data


def _blocks():
    return [(R.machine_code(70_000, 1), [{"id": lzma.FILTER_X86}, L2]),
            (R.text(30_000), [L2]),
            (R.opcode_soup(50_000, 5), [{"id": lzma.FILTER_DELTA, "dist": 3}, {"id": lzma.FILTER_POWERPC, "start_offset": 8}, L2]),
            (b"", [{"id": lzma.FILTER_ARM}, L2]),
            (R.machine_code(20_000, 0), [{"id": lzma.FILTER_SPARC}, {"id": lzma.FILTER_ARMTHUMB, "start_offset": 2}, {"id": lzma.FILTER_IA64}, L2])]


def test_xz_several_blocks_and_concatenated_streams(xlz_so):
    blocks = _blocks()
    one = X.stream(blocks)
    assert lzma.decompress(one) == b"".join(d for d, _ in blocks)       # (liblzma reads what the writer assembled)
    got_blocks, steps, total = lzma_amd.xz_index_chains(one)
    assert len(got_blocks) == len(blocks) and total == sum(len(d) for d, _ in blocks)
    assert steps == X.decoder_steps(blocks)
    # two streams with different chains and checks, stream padding between them
    a, b = blocks[:2], blocks[2:]
    sa, sb = X.stream(a, check=lzma.CHECK_CRC32), X.stream(b, check=lzma.CHECK_CRC64)
    assert lzma.decompress(sa + sb) == b"".join(d for d, _ in blocks)   # (Python's one-shot call stops at stream padding)
    two = sa + bytes(8) + sb
    got_blocks, steps, total = lzma_amd.xz_index_chains(two)
    assert [g["check_type"] for g in got_blocks] == [1, 1, 4, 4, 4]
    assert steps == X.decoder_steps(blocks)
    # capacity: the count comes back with XLZ_ERR_OUT_CAP
    buf = ctypes.create_string_buffer(two, len(two))
    nb, ns, tot = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_uint64()
    arr = (N.XzBlock * 8)()
    st1 = (N.FilterStep * 1)()
    st = N.lib().xlz_xz_index_chains(ctypes.cast(buf, ctypes.c_void_p), len(two), arr, 8, ctypes.byref(nb), st1, 1, ctypes.byref(ns), ctypes.byref(tot))
    assert st == lzma_amd.ERR_OUT_CAP and ns.value == len(steps) and nb.value == 5
    assert N.lib().xlz_xz_index_chains(ctypes.cast(buf, ctypes.c_void_p), len(two), None, 0, ctypes.byref(nb), None, 0, None, None) == lzma_amd.ERR_BAD_ARG


def test_xz_block_header_mutations(xlz_so):
    data = R.machine_code(40_000, 1)
    good = [(data, [{"id": lzma.FILTER_X86}, L2])]
    lz2 = (0x21, bytes([X.DICT_BYTE]))

    def status(header):
        xz = X.stream(good, header_of={0: header})
        st = _status(lzma_amd.xz_index_chains, xz)
        if st != lzma_amd.OK:   # liblzma refuses the same file
            with pytest.raises(lzma.LZMAError):
                lzma.decompress(xz)
        return st

    assert status([(0x04, b""), lz2]) == lzma_amd.OK
    assert status([(0x04, struct.pack("<I", 4096)), lz2]) == lzma_amd.OK
    assert status([(0x04, b"\x00\x10"), lz2]) == lzma_amd.ERR_UNSUPPORTED             # a wrong property size
    assert status([(0x03, b""), lz2]) == lzma_amd.ERR_UNSUPPORTED                       # Delta without its distance
    assert status([(0x03, b"\x00\x00"), lz2]) == lzma_amd.ERR_UNSUPPORTED
    assert status([(0x07, struct.pack("<I", 2)), lz2]) == lzma_amd.ERR_UNSUPPORTED      # a misaligned start offset
    assert status([(0x06, struct.pack("<I", 8)), lz2]) == lzma_amd.ERR_UNSUPPORTED
    assert status([(0x08, struct.pack("<I", 1)), lz2]) == lzma_amd.ERR_UNSUPPORTED
    assert status([lz2, (0x04, b"")]) == lzma_amd.ERR_UNSUPPORTED                       # LZMA2 not last / a filter last
    assert status([(0x04, b"")]) == lzma_amd.ERR_UNSUPPORTED
    assert status([lz2, lz2]) == lzma_amd.ERR_UNSUPPORTED
    assert status([(0x0A, b""), lz2]) == lzma_amd.ERR_UNSUPPORTED                       # ARM64: nothing here can judge it
    assert status([(0x0B, b""), lz2]) == lzma_amd.ERR_UNSUPPORTED
    assert status([(0x02, b""), lz2]) == lzma_amd.ERR_UNSUPPORTED
    # a flipped bit in the header: its CRC32 no longer holds
    xz = bytearray(X.stream(good))
    xz[12 + 2] ^= 0x01
    assert _status(lzma_amd.xz_index_chains, bytes(xz)) == lzma_amd.ERR_RESULT
    # ... and the plain index refuses every chain, well-formed or not
    assert _status(lzma_amd.xz_index, X.stream(good)) == lzma_amd.ERR_UNSUPPORTED


FILTER_SETS = [[{"id": lzma.FILTER_X86}], [{"id": lzma.FILTER_DELTA, "dist": 4}], [{"id": lzma.FILTER_DELTA, "dist": 1}],
               [{"id": lzma.FILTER_ARM}], [{"id": lzma.FILTER_ARMTHUMB}], [{"id": lzma.FILTER_POWERPC}], [{"id": lzma.FILTER_SPARC}],
               [{"id": lzma.FILTER_IA64}], [{"id": lzma.FILTER_DELTA, "dist": 2}, {"id": lzma.FILTER_X86}],
               [{"id": lzma.FILTER_ARM}, {"id": lzma.FILTER_DELTA, "dist": 256}, {"id": lzma.FILTER_X86}]]


def _want_steps(k, filters):
    return [(k, f["id"], f.get("dist", 1) if f["id"] == lzma.FILTER_DELTA else 0) for f in reversed(filters)]


def test_7z_chain_folders(xlz_so):
    data = R.machine_code(120_000, 1)
    folders, want = [], []
    for k, fl in enumerate(FILTER_SETS):
        rec, packed, nc = Z.chain_folder(data[k * 100:], fl, lzma2=bool(k & 1), lzma_first=bool(k & 2))
        folders.append((rec, packed, nc, [data[k * 100: 5000], data[5000:]]))
        want += _want_steps(k, fl)
    arch = Z.archive(folders)
    fo, files, steps, total = lzma_amd.sevenzip_index_chains(arch)
    assert steps == want
    assert total == sum(len(data) - k * 100 for k in range(len(FILTER_SETS)))
    for k, f in enumerate(fo):
        assert f["method"] == (2 if k & 1 else 1) and f["unpack_len"] == len(data) - k * 100 and f["n_substreams"] == 2
        assert f["has_crc"] and f["crc"] == zlib.crc32(data[k * 100:])
        if not k & 1:
            assert f["dict_size"] == 1 << 16 and f["props"] == 0x5D
        # the payload decodes with liblzma to bytes the steps turn into the files
        raw = lzma.decompress(arch[f["pack_off"]: f["pack_off"] + f["pack_len"]], format=lzma.FORMAT_RAW,
                              filters=[{"id": lzma.FILTER_LZMA2, "dict_size": f["dict_size"]} if k & 1 else
                                       {"id": lzma.FILTER_LZMA1, "dict_size": f["dict_size"], "lc": 3, "lp": 0, "pb": 2}])
        for _, fid, prm in [s for s in steps if s[0] == k]:
            raw = lzma_amd.filter_host(fid, prm, raw)
        assert raw == data[k * 100:]
    # the plain index: the same archive, every chain method 0, the same sizes and files
    fo0, files0, total0 = lzma_amd.sevenzip_index(arch)
    assert all(f["method"] == 0 for f in fo0) and files0 == files and total0 == total


def test_7z_folders_that_are_no_chain_stay_unsupported(xlz_so):
    data = R.text(20_000)

    def method(folder, **kw):
        rec, packed, nc = folder
        fo, _, steps, _ = lzma_amd.sevenzip_index_chains(Z.archive([(rec, packed, nc, [data])], **kw))
        return fo[0]["method"], steps

    x86 = [{"id": lzma.FILTER_X86}]
    assert method(Z.chain_folder(data, x86)) == (1, [(0, 4, 0)])
    assert method(Z.chain_folder(data, x86, binds=[(1, 0)])) == (0, [])                   # the filter reads the packed stream
    assert method(Z.chain_folder(data, x86 * 2, binds=[(0, 2), (1, 2)]))[0] == 0          # one output bound twice
    assert method(Z.chain_folder(data, x86 * 2, binds=[(0, 1), (0, 2)]))[0] == 0          # one input bound twice
    assert method(Z.chain_folder(data, x86), sizes_override={0: [len(data), len(data) - 1]})[0] == 0   # an intermediate size differs
    # four filters: one more than a stream may have steps
    assert method(Z.chain_folder(data, x86 * 3))[0] == 1
    assert method(Z.chain_folder(data, x86 * 3, listed=x86 * 4))[0] == 0
    # an unknown method (ARM64 in 7-Zip's table: 0xA) and BCJ2's id in the line
    rec, packed, nc = Z.chain_folder(data, x86)
    for bad in (b"\x0a", b"\x03\x03\x01\x1b"):
        raw = rec[1].replace(bytes([4]) + b"\x03\x03\x01\x03", bytes([len(bad)]) + bad)
        assert method((("raw", raw), packed, nc)) == (0, [])
    # x86 with a property (7-Zip writes none)
    raw = rec[1].replace(bytes([4]) + b"\x03\x03\x01\x03", bytes([0x24]) + b"\x03\x03\x01\x03" + Z.number(4) + bytes(4))
    assert method((("raw", raw), packed, nc)) == (0, [])
    # Delta takes exactly one property byte: none, or two, is refused (7-Zip's decoder refuses both)
    delta = [{"id": lzma.FILTER_DELTA, "dist": 1}]
    rec, packed, nc = Z.chain_folder(data, delta)
    good = bytes([0x21]) + b"\x03" + Z.number(1) + bytes(1)
    assert good in rec[1] and method((rec, packed, nc)) == (1, [(0, 3, 1)])
    for bad in (bytes([0x01]) + b"\x03", bytes([0x21]) + b"\x03" + Z.number(2) + bytes(2)):
        assert method((("raw", rec[1].replace(good, bad)), packed, nc)) == (0, [])


def test_7z_chains_against_cmake_extraction(xlz_so, tmp_path):
    """`cmake -E tar xf` (cmake's bundled libarchive) extracts these archives when the LZMA / LZMA2 coder is listed first
    and there is ONE filter: behind LZMA2 all seven filters come out right; behind LZMA it returns the right bytes for x86,
    Delta, ARM-Thumb and IA-64 and reports a bad CRC for ARM, PowerPC and SPARC (liblzma decodes those payloads bit for
    bit: the reader's fault, not the archive's); folders of two and more filters it refuses ("many filters").  Where it
    extracts without complaint, its bytes must be what the index's payload and steps give, and exactly the pairs named
    here must extract: an archive that stops extracting does not pass unnoticed."""
    if not shutil.which("cmake"):
        pytest.skip("no cmake on this box: nothing here extracts a .7z archive")
    data = R.machine_code(90_000, 1)
    agreed = set()
    for k, fl in enumerate(FILTER_SETS):
        for l2 in (False, True):
            rec, packed, nc = Z.chain_folder(data, fl, lzma2=l2, lzma_first=True)
            arch = Z.archive([(rec, packed, nc, [data[:777], data[777:]])], names=["a.bin", "b.bin"])
            d = tmp_path / ("x%d_%d" % (k, l2))
            d.mkdir()
            (d / "x.7z").write_bytes(arch)
            r = subprocess.run(["cmake", "-E", "tar", "xf", "x.7z"], cwd=str(d), capture_output=True, text=True)
            if r.returncode != 0 or r.stderr.strip() or not (d / "b.bin").exists():
                continue
            fo, _, steps, _ = lzma_amd.sevenzip_index_chains(arch)
            raw = lzma.decompress(arch[fo[0]["pack_off"]: fo[0]["pack_off"] + fo[0]["pack_len"]], format=lzma.FORMAT_RAW,
                                  filters=[{"id": lzma.FILTER_LZMA2, "dict_size": fo[0]["dict_size"]} if l2 else
                                           {"id": lzma.FILTER_LZMA1, "dict_size": fo[0]["dict_size"], "lc": 3, "lp": 0, "pb": 2}])
            for _, fid, prm in steps:
                raw = lzma_amd.filter_host(fid, prm, raw)
            assert (d / "a.bin").read_bytes() + (d / "b.bin").read_bytes() == raw == data, (fl, l2)
            agreed.add((k, l2))
    # FILTER_SETS[0 .. 7] are the single filters: all behind LZMA2; x86, Delta (twice), ARM-Thumb and IA-64 behind LZMA
    assert agreed == {(k, True) for k in range(8)} | {(k, False) for k in (0, 1, 2, 4, 7)}, sorted(agreed)


def test_decode_batch_filtered_without_a_device(xlz_so):
    L = N.lib()
    if L.xlz_device_count() > 0:
        pytest.skip("a GPU is present: the filtered call is covered by tests/test_gpu_filters.py")
    comp = lzma.compress(b"x" * 100, format=lzma.FORMAT_ALONE)
    descs, keep, outs = lzma_amd._make_descs([lzma_amd.Stream(comp, lzma_amd.FMT_LZMA_ALONE, out_cap=100)])
    res = (N.Result * 1)()
    steps = lzma_amd._make_steps([(0, R.X86, 0)])
    assert L.xlz_decode_batch_filtered(None, descs, 1, res, steps, 1, None, 0, None) == lzma_amd.ERR_DEVICE
    with pytest.raises(lzma_amd.LzmaError) as e:
        lzma_amd.Context(0)
    assert e.value.status == lzma_amd.ERR_DEVICE
