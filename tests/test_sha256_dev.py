"""CPU: the device's SHA-256 without a GPU.  The shared header (lzma_amd/csrc/xlz_sha256_dev.h) runs one lane's code in a
g++ program against the FIPS 180-4 known answers and the host's xlzcheck::sha256; the host-only plan that splits a call's
ranges between the device and the host threads (xlz_sha256_plan) with explicit rates; the new entry points are exported
and refuse NULL handles; and the decode kernels' id is what it was: the SHA-256 kernel is new files beside them."""
import ctypes
import os
import subprocess

import lzma_amd
from lzma_amd import _native as N
from lzma_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20
# the issue's rates: one GPU lane, one host thread of sixteen (explicit, so that no measured constant is pinned here)
LANE, HOST, THREADS = 25e6, 350e6, 16


def test_decode_kernel_id_is_unchanged():
    assert build.source_id(build.KERNEL_FILES) == "6dd215c46ed5"
    assert "xlz_sha256_dev.hip" in build.SOURCES and "xlz_sha256_dev.h" in build.HEADERS
    assert not any(f.startswith("xlz_sha256") for f in build.KERNEL_FILES)


def test_lane_code_on_the_cpu(tmp_path):
    """FIPS 180-4 known answers (empty, "abc", the 56-byte two-block message, a million 'a') at every start alignment;
    every length 0-300 at every start alignment 0-15 against xlzcheck::sha256, in an arena with room and in one that ends
    with the range; lengths around 55 / 56 / 63 / 64 / 119 / 120; bytes outside a range must not reach its digest"""
    exe = str(tmp_path / "sha256_dev_selftest")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "lzma_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "sha256_dev_selftest.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")


def test_plan_many_short_ranges_go_to_the_device(xlz_so):
    assert lzma_amd.sha256_plan([MIB] * 4096, THREADS, LANE, HOST) == [True] * 4096


def test_plan_few_long_ranges_stay_on_the_host(xlz_so):
    assert lzma_amd.sha256_plan([64 * MIB] * 16, THREADS, LANE, HOST) == [False] * 16


def test_plan_takes_the_long_range_out(xlz_so):
    for at in (0, 1000, 4095):
        lens = [MIB] * 4095
        lens.insert(at, 256 * MIB)
        want = [True] * 4095
        want.insert(at, False)
        assert lzma_amd.sha256_plan(lens, THREADS, LANE, HOST) == want


def test_plan_edges(xlz_so):
    L = N.lib()
    assert lzma_amd.sha256_plan([]) == []
    assert L.xlz_sha256_plan(None, 0, 0, 0, 0, None) == lzma_amd.OK
    lens = (ctypes.c_uint64 * 3)(1, 2, 3)
    on = (ctypes.c_uint8 * 3)()
    assert L.xlz_sha256_plan(None, 3, 0, 0, 0, on) == lzma_amd.ERR_BAD_ARG
    assert L.xlz_sha256_plan(lens, 3, 0, 0, 0, None) == lzma_amd.ERR_BAD_ARG


def _built_in_rates():
    """kLaneBytesPerS of lzma_amd/csrc/xlz_sha256_dev.h"""
    import re
    src = open(os.path.join(ROOT, "lzma_amd", "csrc", "xlz_sha256_dev.h")).read()
    return float(re.search(r"constexpr double kLaneBytesPerS = ([0-9.e+]+);", src).group(1))


def test_plan_never_gives_the_device_half_a_second(xlz_so):
    """with the built-in rates, whatever the mix and however fast the caller says a lane is: no device range is longer
    than 0.5 s of the built-in lane rate (a launch takes one round of lanes, so that bounds the launch)"""
    lane = _built_in_rates()
    cap = 0.5 * lane
    assert 1e6 < lane < 1e9
    mixes = [[MIB] * 100_000 + [int(cap) - 1, int(cap) + 1, 2 * int(cap)],
             [int(cap) + 1] * 200_000,
             [int(cap * f) for f in (0.1, 0.5, 0.99, 1.01, 1.5, 4, 100)] * 3000,
             [1 << 40, 5, 0]]
    for lens in mixes:
        for rates in ((0, 0), (1e12, 1.0)):   # (built in; a caller who claims a very fast lane and a very slow host)
            on = lzma_amd.sha256_plan(lens, 0, *rates)
            assert all(n <= cap for n, d in zip(lens, on) if d), rates
    assert any(lzma_amd.sha256_plan(mixes[0]))   # (and the device does get work)


def test_new_symbols_are_exported(xlz_so):
    L = N.lib()
    for name in ("xlz_batch_digests", "xlz_decode_batch_digests", "xlz_sha256_plan", "xlz_ctx_last_sha256_stats"):
        assert name in N.EXPORTS and hasattr(L, name), name
    assert lzma_amd.CHECK_SHA256 == 10
    assert ctypes.sizeof(N.Digest) == 32


def test_digest_entry_points_need_their_handles(xlz_so):
    """a NULL batch / context is refused instead of touching a device"""
    L = N.lib()
    assert L.xlz_batch_digests(None, None, 0, None) == lzma_amd.ERR_BAD_ARG
    assert L.xlz_decode_batch_digests(None, None, 0, None, None, 0, None, 0, None) == lzma_amd.ERR_BAD_ARG
    assert L.xlz_ctx_last_sha256_stats(None, None) == lzma_amd.ERR_BAD_ARG
    assert L.xlz_ctx_set_check_mode(None, 2) == lzma_amd.ERR_BAD_ARG
