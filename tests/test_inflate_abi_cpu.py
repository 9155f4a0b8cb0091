"""CPU: the C ABI of the deflate feature as far as it needs no device -- the symbols, what the calls settle before they use a
context, the new entry flag of the ZIP table, and the plan of an extraction in deflate mode 0, 1 and 2 (through a g++
program over lzma_amd/csrc/xlz_zip.h).  What needs a context (a new one has mode 0, the mode round-trips, mode 3 is
refused) is in tests/test_gpu_zip_deflate.py: a context is a device."""
import ctypes
import os
import subprocess
import sys
import zipfile
import zlib

import pytest

import lzma_amd
from lzma_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INFOZIP = os.path.join(ROOT, "tests", "golden", "infozip.zip")
NEW = ["xlz_inflate_host", "xlz_inflate_batch", "xlz_ctx_set_deflate_mode", "xlz_ctx_deflate_mode", "xlz_ctx_last_inflate_stats"]


def test_the_new_symbols_are_exported(xlz_so):
    L = N.lib()
    for name in NEW:
        assert name in N.EXPORTS and hasattr(L, name), name
    assert N.ZIP_ENTRY_DEFLATE == 256 == lzma_amd.ZIP_ENTRY_DEFLATE
    assert ctypes.sizeof(N.InflateItem) == 32 and ctypes.sizeof(N.InflateResult) == 24 and ctypes.sizeof(N.InflateStats) == 48


def test_without_a_context_every_call_is_a_bad_argument(xlz_so):
    L = N.lib()
    assert L.xlz_ctx_set_deflate_mode(None, 1) == lzma_amd.ERR_BAD_ARG and L.xlz_ctx_deflate_mode(None) == lzma_amd.ERR_BAD_ARG
    assert L.xlz_ctx_last_inflate_stats(None, ctypes.byref(N.InflateStats())) == lzma_amd.ERR_BAD_ARG
    assert L.xlz_inflate_batch(None, None, 0, None, 0, None) == lzma_amd.ERR_BAD_ARG


def test_inflate_host_arguments_and_outputs(xlz_so):
    L = N.lib()
    produced, consumed = ctypes.c_size_t(9), ctypes.c_size_t(9)
    out = ctypes.create_string_buffer(16)
    assert L.xlz_inflate_host(None, 5, ctypes.cast(out, ctypes.c_void_p), 16, ctypes.byref(produced), ctypes.byref(consumed)) == lzma_amd.ERR_BAD_ARG
    assert (produced.value, consumed.value) == (0, 0)
    data = zlib.compress(b"deflate " * 40)[2:-4]
    buf = ctypes.create_string_buffer(data, len(data))
    assert L.xlz_inflate_host(ctypes.cast(buf, ctypes.c_void_p), len(data), None, 5, None, None) == lzma_amd.ERR_BAD_ARG
    assert L.xlz_inflate_host(ctypes.cast(buf, ctypes.c_void_p), len(data), None, 0, None, None) == lzma_amd.ERR_OUT_CAP
    assert L.xlz_inflate_host(None, 0, None, 0, None, None) == lzma_amd.ERR_UNEXPECTED_EOF
    assert lzma_amd.inflate_host(data, 320) == (b"deflate " * 40, len(data))
    assert lzma_amd.inflate_host(data + b"tail", 400) == (b"deflate " * 40, len(data))
    for cap, status in ((319, lzma_amd.ERR_OUT_CAP), (0, lzma_amd.ERR_OUT_CAP)):
        with pytest.raises(lzma_amd.LzmaError) as e:
            lzma_amd.inflate_host(data, cap)
        assert e.value.status == status
    with pytest.raises(lzma_amd.LzmaError) as e:
        lzma_amd.inflate_host(data[:-1], 320)
    assert e.value.status == lzma_amd.ERR_UNEXPECTED_EOF
    with pytest.raises(lzma_amd.LzmaError) as e:
        lzma_amd.inflate_host(b"\x07", 320)
    assert e.value.status == lzma_amd.ERR_RESULT


def test_the_table_marks_deflate_entries_beside_their_class(xlz_so):
    """Info-ZIP wrote the archive (Python's zipfile lists it but cannot read it: tests/golden/make_infozip_zip.py says why and
    holds the contents)"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_infozip_zip as R
    data = open(INFOZIP, "rb").read()
    with lzma_amd.ZipFile(data) as z, zipfile.ZipFile(INFOZIP) as ref:
        by_name = {i.filename: i for i in ref.infolist()}
        deflated = [e for e in z.entries if e["deflate"]]
        assert sorted(e["name"] for e in deflated) == sorted(R.DEFLATED) == ["deflated_3000.txt", "sub/deflated_257.txt"]
        for e in z.entries:
            assert e["deflate"] == (by_name[e["name"]].compress_type == zipfile.ZIP_DEFLATED) == bool(e["flags"] & lzma_amd.ZIP_ENTRY_DEFLATE)
            assert not (e["deflate"] and (e["supported"] or e["bad"])), e["name"]
            assert e["deflate"] or e["is_dir"] or e["supported"], e["name"]
        for e in deflated:   # where the table says the payload lies, the decoder finds the entry, and so does zlib
            raw = data[e["data_off"]:e["data_off"] + e["comp_size"]]
            assert lzma_amd.inflate_host(raw, e["size"]) == (R.DEFLATED[e["name"]], len(raw))
            assert zlib.decompressobj(-15).decompress(raw) == R.DEFLATED[e["name"]] and zlib.crc32(R.DEFLATED[e["name"]]) == e["crc"]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "sanitizers"])
def test_the_plan_in_every_deflate_mode(tmp_path, flags):
    exe = str(tmp_path / "zip_deflate_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", os.path.join(ROOT, "lzma_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "zip_deflate_selftest.cpp"), "-o", exe])
    run = subprocess.run([exe, INFOZIP], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().endswith("checks, 0 failures"), run.stdout[-3000:] + run.stderr[-3000:]
