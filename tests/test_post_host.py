"""CPU: what the post-decode stage (filters, CRC32 / CRC64, SHA-256 behind a decoded batch) decides without a device.
The shared header (lzma_amd/csrc/xlz_post.h) runs in a g++ program: the clip of a range to what its stream produced and
where those bytes lie -- off behind and at the end, lengths up to 2^64 - 1, sums that wrap, nothing produced, out_len above
out_cap inside and outside the arena, and the streams of 4 GiB and more that no short GPU test reaches --, and the one
statistics add: seven sums, SHA-256's threshold a maximum."""
import os
import subprocess

from lzma_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_post_header_is_host_code():
    assert "xlz_post.h" in build.HEADERS and "xlz_post.h" not in build.KERNEL_FILES


def test_clip_and_statistics_on_the_cpu(tmp_path):
    exe = str(tmp_path / "post_selftest")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lzma_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "post_selftest.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")
