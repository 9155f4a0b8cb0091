"""CPU: the BCJ2 merge's wave scheme without a GPU.  The shared header (lzma_amd/csrc/xlz_bcj2_dev.h) runs phase by phase,
lanes in descending order, in a g++ program against the serial merge of the same header; the decode kernels' id is what it
was: the merge is new files beside them."""
import os
import subprocess
import sys

import pytest

from lzma_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decode_kernel_id_is_unchanged():
    assert build.source_id(build.KERNEL_FILES) == "6dd215c46ed5"
    assert "xlz_bcj2_dev.hip" in build.SOURCES and "xlz_bcj2_dev.h" in build.HEADERS
    assert not any(f.startswith("xlz_bcj2") for f in build.KERNEL_FILES)


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bcj2") / "bcj2_dev_selftest")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lzma_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "bcj2_dev_selftest.cpp"), "-o", exe])
    return exe


def test_wave_scheme_on_the_cpu(selftest):
    """random bytes with E8 / E9 / 0F 8x at three densities x four conversion policies x lengths 0-17, 1023-1025, 2047-2049,
    5000, 65 539; runs of E8 and of 0F 8x all taken / none taken; a candidate as the last byte and with one to five bytes
    behind it, also as a window's last byte; the prev trap inside a lane, across lanes and across windows; a window
    without candidates; a conversion that ends at out_len; less room than the streams fill by one to nine bytes; damaged
    call / jump / rc / main streams; machine code (the Python binary).  Destinations at 0, 1, 7, 13 modulo 16 and more, with
    guard bytes compared; every stream in a heap block of its length rounded up to 16."""
    out = subprocess.run([selftest, sys.executable], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_wave_scheme_under_the_sanitizers(tmp_path):
    """the same program -- a stand-alone one, with its own main -- built with AddressSanitizer and UBSan: every stream lies
    in a heap block of exactly its length rounded up to 16, so a load the alignment rule does not cover is seen"""
    exe = str(tmp_path / "bcj2_dev_selftest_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17"] + SAN + ["-I", os.path.join(ROOT, "lzma_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "bcj2_dev_selftest.cpp"), "-o", exe])
    out = subprocess.run([exe, sys.executable], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip().endswith("ok")


def test_mutated_bcj2_headers_through_the_index_call(tmp_path):
    """a seeded mutation loop over the headers of three archives with BCJ2 folders (both forms, both listings of the four
    coders) through xlz_7z_index_bcj2 and the older index calls: the parser of xlz_7z.hip compiled into a stand-alone
    program with AddressSanitizer and UBSan (tests/c/bcj2_index_fuzz.cpp), 3 x 20 000 headers, each parsed twice"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import filter_ref as R
    import sevenzip_bcj2 as Z
    import sevenzip_craft as C
    code, text = R.machine_code(20_000), R.text(3000)
    seeds = []
    for k, (form, l2, layout) in enumerate([(4, False, "libarchive"), (4, True, "7zip"), (2, False, "")]):
        arch = Z.archive([Z.plain_folder(*C.lzma_folder(text), [text]), Z.bcj2_folder([code[:700], code[700:]], form, l2, layout)])
        seeds.append(str(tmp_path / ("seed%d.7z" % k)))
        with open(seeds[-1], "wb") as f:
            f.write(arch)
    exe = str(tmp_path / "bcj2_index_fuzz")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-x", "c++"] + SAN + ["-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "bcj2_index_fuzz.cpp"), "-o", exe])
    out = subprocess.run([exe, "20000"] + seeds, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip().endswith("ok") and "60000 mutated headers" in out.stdout
    indexed = int(out.stdout.split("mutated headers, ")[1].split()[0])
    assert 1000 < indexed < 60000  # the mutations reach the parser: some headers survive them, most do not


def test_the_merge_rate_is_marked_as_an_estimate():
    """until tools/bcj2_bench.py has run on an MI355X the launch-length cap rests on an estimate, and says so"""
    text = open(os.path.join(ROOT, "lzma_amd", "csrc", "xlz_bcj2_dev.h")).read()
    assert "AN ESTIMATE" in text and "kMaxDeviceLen = (uint64_t)(0.5 * kWaveBytesPerS)" in text
