"""CPU: the device steps of the .tar listing without a GPU.  The shared header (lzma_amd/csrc/xlz_tar_dev.h) runs its lane
scheme in a g++ program against a serial classifier, with the load helper's assertion that no load leaves the complete
blocks of the image; the walk's own serial classifier (xlz_tar_walk.h), which the host form uses, agrees with the same
judge on the same blocks.  The decode kernels' id is what it was: the listing is new files beside them."""
import os
import subprocess
import sys

import pytest

from lzma_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def test_decode_kernel_id_is_unchanged():
    assert build.source_id(build.KERNEL_FILES) == "6dd215c46ed5"
    assert "xlz_tar_dev.hip" in build.SOURCES and "xlz_tar_dev.h" in build.HEADERS and "xlz_tar_walk.h" in build.HEADERS
    assert not any(f.startswith("xlz_tar") for f in build.KERNEL_FILES)


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tar") / "tar_dev_selftest")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lzma_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "tar_dev_selftest.cpp"), "-o", exe])
    return exe


def test_lane_scheme_on_the_cpu(selftest):
    """images of 0, 1, 2, 63, 64, 65, 127, 128 and 129 blocks of zero runs, random bytes, headers and near-headers; lengths
    511, 512, 513, 1023, 1024, 1025 (the tail is never loaded: the bounds assertion is on); every form of the checksum field
    in each half of a wave and alone in the last pair; signed and unsigned sums; a block that is nothing but its field; sums
    off by one; all bytes 0xFF; gathers of no, one, 65 and repeated / descending indices into a sentinel-filled buffer"""
    out = subprocess.run([selftest], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")


def test_header_asserts_are_compiled_in():
    """the self-test is built without NDEBUG: the bounds assertion of load16 is part of the program"""
    text = open(os.path.join(ROOT, "lzma_amd", "csrc", "xlz_tar_dev.h")).read()
    assert "assert((off & 15) == 0 && off < (len & ~(uint64_t)511) && (len & ~(uint64_t)511) - off >= 16);" in text
    assert "NDEBUG" not in open(os.path.join(ROOT, "tests", "c", "tar_dev_selftest.cpp")).read()


def test_the_walks_classifier_is_the_same_judge(xlz_so):
    """xlz_tar_walk.h's classify_block, through tar_parse: a block is taken for a header exactly when the Python form of
    the serial classifier says 1 -- every form of the field, in front of a zero block"""
    import lzma_amd
    import tar_archives as T
    good = T.header(b"f")
    total = int(good[148:154], 8)
    assert 0o1000 <= total < 0o100000
    for field in [b"%07o\0" % total, b"%06o\0 " % total, b"%6o \0" % total, b" %07o" % total, b" " * 8, bytes(8),
                  (b"%07o\0" % total).replace(b"0", b"8", 1), b"%06o\0x" % total, b"%08o" % total, b"%07o\0" % (total + 1),
                  b"%07o\0" % (total - 1)]:
        assert len(field) == 8, field
        block = good[:148] + field + good[156:]
        table = lzma_amd.tar_parse(block + T.END)
        assert (len(table.entries) == 1) == (T.serial_flag(block) == 1), field
        assert table.end_status == (lzma_amd.OK if T.serial_flag(block) == 1 else lzma_amd.ERR_RESULT), field
    signed = bytearray(T.header(b"\xc8" * 40))
    assert T.serial_flag(bytes(signed)) == 1
    signed[148:156] = b"%06o\0 " % (sum(signed[:148]) + sum(signed[156:]) + 256 - 256 * 40)
    assert T.serial_flag(bytes(signed)) == 1 and len(lzma_amd.tar_parse(bytes(signed) + T.END).entries) == 1
