"""CPU: the filters (Delta, BCJ) without a GPU.  The shared header (lzma_amd/csrc/xlz_filter_dev.h) runs its per-lane,
per-window and per-chunk scheme in a g++ program against its own serial form; that serial form is what the library exports
as xlz_filter_host, and it is compared here with liblzma (tests/filter_ref.py) -- and so is the lane scheme itself, bytes
exchanged through files.  The decode kernels' id is what it was: the filters are new files beside them."""
import os
import subprocess
import sys

import pytest

import filter_ref as R
import lzma_amd
from lzma_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decode_kernel_id_is_unchanged():
    assert build.source_id(build.KERNEL_FILES) == "6dd215c46ed5"
    assert "xlz_filter_dev.hip" in build.SOURCES and "xlz_filter_dev.h" in build.HEADERS
    assert not any(f.startswith("xlz_filter") for f in build.KERNEL_FILES)


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("flt") / "filter_dev_selftest")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lzma_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "filter_dev_selftest.cpp"), "-o", exe])
    return exe


def test_lane_scheme_on_the_cpu(selftest):
    """every filter, every start offset and distance, on seeded text, random bytes, zeros, opcodes of all seven filters,
    adversarial x86 buffers (runs of E8 / E9, densities 1-100 %, opcodes in the last eight bytes) and alternating Thumb
    halves; lengths 0-40 and around every window, tile and chunk size +- 5: the device scheme, lanes and chunks in
    descending order, against the serial form"""
    out = subprocess.run([selftest], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")


def test_lane_scheme_on_machine_code(selftest, xlz_so):
    """the same over real machine code: the bytes of libxlz.so and of the Python binary"""
    out = subprocess.run([selftest, xlz_so, sys.executable], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")


def _buffers():
    yield "text", R.text(70_000)
    yield "random", __import__("random").Random(7).randbytes(70_000)
    yield "python", R.machine_code(300_000, 0)
    yield "libxlz", R.machine_code(300_000, 1)
    yield "zeros", bytes(40_000)
    yield "soup", R.opcode_soup(120_000, 11)
    yield "soup dense", R.opcode_soup(50_001, 12, density=90)


def test_host_filter_against_liblzma(xlz_so):
    """xlz_filter_host on every filter x parameter x buffer, whole and cut to lengths 0-40 and odd ends"""
    changed = 0
    for name, buf in _buffers():
        for fid in R.ALL:
            for prm in R.params(fid):
                want = R.apply(fid, prm, buf)
                assert lzma_amd.filter_host(fid, prm, buf) == want, (name, fid, prm)
                changed += want != buf
    soup = R.opcode_soup(4096, 13, density=60)
    for n in list(range(41)) + [255, 256, 257, 261, 4091]:
        for fid in R.ALL:
            for prm in R.params(fid):
                assert lzma_amd.filter_host(fid, prm, soup[:n]) == R.apply(fid, prm, soup[:n]), (n, fid, prm)
    assert changed > 100   # (the buffers give every filter work)


def test_host_x86_adversarial_against_liblzma(xlz_so):
    """runs of E8 / E9, every density of the issue's experiment and beyond, opcodes in the last eight bytes"""
    for density in (5, 10, 15, 20, 25, 30, 60, 100):
        for runs in (False, True):
            buf = R.x86_adversarial(20_000, 100 * density + runs, density, runs)
            for prm in R.OFFSETS:
                assert lzma_amd.filter_host(R.X86, prm, buf) == R.apply(R.X86, prm, buf), (density, runs, prm)
            for k in range(1, 9):
                b = bytearray(buf[:600])
                b[-k] = 0xE8
                if k > 4:
                    b[-k + 4] = 0
                assert lzma_amd.filter_host(R.X86, 0, b) == R.apply(R.X86, 0, bytes(b)), (density, k)


def test_lane_scheme_against_liblzma_through_files(selftest, tmp_path, xlz_so):
    """the g++ program's lane scheme applied to files, judged by liblzma directly"""
    src = tmp_path / "in.bin"
    dst = tmp_path / "out.bin"
    for name, buf in (("libxlz", R.machine_code(200_000, 1)), ("soup", R.opcode_soup(100_003, 21)),
                      ("e8 runs", R.x86_adversarial(50_000, 22, 20, True))):
        src.write_bytes(buf)
        for fid in R.ALL:
            for prm in (R.params(fid)[1], R.params(fid)[-1]):
                subprocess.check_call([selftest, "--apply", str(fid), str(prm), str(src), str(dst)])
                assert dst.read_bytes() == R.apply(fid, prm, buf), (name, fid, prm)


def test_host_filter_argument_errors(xlz_so):
    from lzma_amd import _native as N
    L = N.lib()
    import ctypes
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.xlz_filter_host(R.X86, 0, p, 64) == lzma_amd.OK
    assert L.xlz_filter_host(R.X86, 0, None, 0) == lzma_amd.OK
    assert L.xlz_filter_host(R.X86, 0, None, 8) == lzma_amd.ERR_BAD_ARG
    for fid in (0, 1, 2, 10, 11, 0x21, 0xFFFFFFFF):                      # ARM64 and RISC-V are not implemented
        assert L.xlz_filter_host(fid, 0, p, 64) == lzma_amd.ERR_BAD_ARG, fid
    for dist in (0, 257, 1 << 20):
        assert L.xlz_filter_host(R.DELTA, dist, p, 64) == lzma_amd.ERR_BAD_ARG
    for fid, off in ((R.ARM, 2), (R.POWERPC, 1), (R.SPARC, 6), (R.ARMTHUMB, 1), (R.IA64, 8), (R.IA64, 4)):
        assert L.xlz_filter_host(fid, off, p, 64) == lzma_amd.ERR_BAD_ARG, (fid, off)
    assert L.xlz_filter_host(R.IA64, 0xFFFFFFF0, p, 64) == lzma_amd.OK


def test_filter_entry_points_need_their_objects(xlz_so):
    from lzma_amd import _native as N
    L = N.lib()
    assert L.xlz_ctx_set_filter_mode(None, 1) == lzma_amd.ERR_BAD_ARG
    assert L.xlz_ctx_filter_mode(None) == lzma_amd.ERR_BAD_ARG
    assert L.xlz_ctx_last_filter_stats(None, None) == lzma_amd.ERR_BAD_ARG
    assert L.xlz_batch_filter(None, None, 0) == lzma_amd.ERR_BAD_ARG
