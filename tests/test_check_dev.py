"""CPU: the device checks' arithmetic without a GPU.  The shared header (lzma_amd/csrc/xlz_check_dev.h) runs its 64-lane
scheme lane by lane in a g++ program against a bit-by-bit CRC; the exported folds xlz_crc32_combine / xlz_crc64_combine
against zlib and liblzma; and the decode kernels' id is what it was: the checks are new files beside them."""
import os
import random
import subprocess

import check_ref
import lzma_amd
from lzma_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decode_kernel_id_is_unchanged():
    assert build.source_id(build.KERNEL_FILES) == "6dd215c46ed5"
    assert "xlz_check_dev.hip" in build.SOURCES and "xlz_check_dev.h" in build.HEADERS
    assert not any(f.startswith("xlz_check") for f in build.KERNEL_FILES)


def test_lane_scheme_on_the_cpu(tmp_path):
    """lengths 0-300 at every start alignment 0-15, lengths around one row and one segment, several segments, more
    segments than the fold has threads; both CRCs; bytes outside a range must not reach its digest"""
    exe = str(tmp_path / "check_dev_selftest")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lzma_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "check_dev_selftest.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")


def test_liblzma_crc64_helper_known_answers():
    assert check_ref.crc64(b"123456789") == 0x995DC9BBDF1939FA
    assert check_ref.crc32(b"123456789") == 0xCBF43926
    assert check_ref.crc64(b"") == 0


def test_exported_combine(xlz_so):
    rnd = random.Random(4242)
    for n in (0, 1, 2, 17, 4097, 100_000, 1 << 20):
        data = rnd.randbytes(n)
        for cut in sorted({0, min(1, n), n // 3, n}):
            a, b = data[:cut], data[cut:]
            assert lzma_amd.crc32_combine(check_ref.crc32(a), check_ref.crc32(b), len(b)) == check_ref.crc32(data), (n, cut)
            assert lzma_amd.crc64_combine(check_ref.crc64(a), check_ref.crc64(b), len(b)) == check_ref.crc64(data), (n, cut)
    # compressible data beyond a few MiB: 48 MiB in three parts, folded left to right
    parts = [bytes([i]) * (16 << 20) + rnd.randbytes(1000) for i in range(3)]
    c32, c64 = 0, 0
    for p in parts:
        c32 = lzma_amd.crc32_combine(c32, check_ref.crc32(p), len(p))
        c64 = lzma_amd.crc64_combine(c64, check_ref.crc64(p), len(p))
    whole = b"".join(parts)
    assert c32 == check_ref.crc32(whole) and c64 == check_ref.crc64(whole)


def test_check_mode_and_stats_need_a_context():
    """the context entry points refuse a NULL context instead of touching a device"""
    from lzma_amd import _native as N
    L = N.lib()
    assert L.xlz_ctx_set_check_mode(None, 1) == lzma_amd.ERR_BAD_ARG
    assert L.xlz_ctx_check_mode(None) == lzma_amd.ERR_BAD_ARG
    assert L.xlz_ctx_last_check_stats(None, None) == lzma_amd.ERR_BAD_ARG
    assert L.xlz_batch_checks(None, None, 0, None) == lzma_amd.ERR_BAD_ARG
