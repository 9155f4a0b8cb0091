"""CPU: what the post-decode stage (filters, CRC32 / CRC64, SHA-256 behind a decoded batch) decides without a device.
The shared header (lzma_amd/csrc/xlz_post.h) runs in a g++ program: the clip of a range to what its stream produced and
where those bytes lie -- off behind and at the end, lengths up to 2^64 - 1, sums that wrap, nothing produced, out_len above
out_cap inside and outside the arena, and the streams of 4 GiB and more that no short GPU test reaches --, the one
statistics add: seven sums, SHA-256's threshold a maximum, the pack's and the BCJ2 merge's counters; where a range of a
device destination lies for the check kernels (every misalignment, the ends, sums that wrap); and the host-thread helper
(every index once for n = 0, 1, n < k, n >> k).  The same program is built with the host sanitizers too, stand-alone."""
import os
import subprocess

import pytest

from lzma_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_post_header_is_host_code():
    assert "xlz_post.h" in build.HEADERS and "xlz_post.h" not in build.KERNEL_FILES


def _selftest(tmp_path, flags, args=()):
    exe = str(tmp_path / "post_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-pthread", *flags, "-I", os.path.join(ROOT, "lzma_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "post_selftest.cpp"), "-o", exe])
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)


def test_clip_and_statistics_on_the_cpu(tmp_path):
    out = _selftest(tmp_path, ["-O2"])
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")


@pytest.mark.parametrize("flags,args", [(["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], []),
                                        (["-fsanitize=thread"], ["threads"])], ids=["asan_ubsan", "tsan_threads"])
def test_selftest_under_the_host_sanitizers(tmp_path, flags, args):
    out = _selftest(tmp_path, ["-O1", "-g"] + flags, args)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")
