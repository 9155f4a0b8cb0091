"""CPU: the pack into device memory without a GPU.  The shared header (lzma_amd/csrc/xlz_pack_dev.h) runs its tile / lane
scheme in a g++ program against memcpy per item, with the load helper's assertion that no aligned load leaves the arena;
the entry points refuse to work without their objects; importing the package does not import torch.  The decode kernels'
id is what it was: the pack is new files beside them."""
import os
import subprocess
import sys

import pytest

import lzma_amd
from lzma_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decode_kernel_id_is_unchanged():
    assert build.source_id(build.KERNEL_FILES) == "6dd215c46ed5"
    assert "xlz_pack_dev.hip" in build.SOURCES and "xlz_pack_dev.h" in build.HEADERS
    assert not any(f.startswith("xlz_pack") for f in build.KERNEL_FILES)


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pack") / "pack_dev_selftest")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lzma_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "pack_dev_selftest.cpp"), "-o", exe])
    return exe


def test_tile_and_lane_scheme_on_the_cpu(selftest):
    """all 256 (source mod 16, destination mod 16) pairs x lengths 0-48, lengths 16 384 +- 5 and 32 768 +- 5, items that
    start in the last 1-17 bytes of a tile, 40 items of 1-7 bytes inside one tile, items in the arena's first and last
    region with the bounds assertion on, a shuffled table of mixed sizes; every byte of a sentinel-filled destination is
    compared, so nothing outside the items may be touched"""
    out = subprocess.run([selftest], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")


def test_header_asserts_are_compiled_in():
    """the self-test is built without NDEBUG: the bounds assertion of load16 is part of the program"""
    text = open(os.path.join(ROOT, "lzma_amd", "csrc", "xlz_pack_dev.h")).read()
    assert "assert((off & 15) == 0 && off < arena_bytes && arena_bytes - off >= 16);" in text
    assert "NDEBUG" not in open(os.path.join(ROOT, "tests", "c", "pack_dev_selftest.cpp")).read()


def test_pack_entry_points_need_their_objects(xlz_so):
    from lzma_amd import _native as N
    L = N.lib()
    assert L.xlz_batch_pack(None, None, 0, None, 0, None) == lzma_amd.ERR_BAD_ARG
    item = (N.PackItem * 1)()
    assert L.xlz_batch_pack(None, item, 1, None, 0, None) == lzma_amd.ERR_BAD_ARG
    assert L.xlz_ctx_last_pack_stats(None, None) == lzma_amd.ERR_BAD_ARG
    import ctypes
    n = ctypes.c_uint64(7)
    for f in (L.xlz_xz_decode_device, L.xlz_7z_decode_device):
        assert f(None, None, 0, None, 0, ctypes.byref(n), 1, None) == lzma_amd.ERR_BAD_ARG


def test_importing_the_package_does_not_import_torch():
    code = "import sys, lzma_amd; assert 'torch' not in sys.modules; print(sorted(n for n in dir(lzma_amd) if 'tensor' in n))"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert "xz_decode_tensor" in r.stdout and "sevenzip_decode_tensor" in r.stdout
