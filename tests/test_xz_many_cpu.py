"""CPU: many .xz files as one batch (include/xlz.h: xlz_xz_many_layout / xlz_xz_decode_many / xlz_xz_decode_many_device;
DESIGN.md section 3.16) as far as no device is needed.  The layout: per-file status against xlz_xz_index /
xlz_xz_index_chains, windows back to back at align 1, 256 and 4096, sizes that overflow 64 bits.  The argument errors of
both decode forms, which are settled before the context is used.  The layout of the new structs against a C program.
The buffers of a call are borrowed, not copied.  And the shared header (lzma_amd/csrc/xlz_xz_many.h) in a g++ program of
its own -- windows, layout, stream map and the fold of per-block outcomes into per-file verdicts against byte-wise models
--, plain and under the host sanitizers."""
import ctypes
import lzma
import os
import subprocess
import sys

import pytest

import lzma_amd
from lzma_amd import _native as N
from lzma_amd import LzmaError, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import xz_many_files as M  # noqa: E402
import xz_ranges_files as X  # noqa: E402


def _layout_files():
    good = lzma.compress(M.text(5000), format=lzma.FORMAT_XZ, check=lzma.CHECK_CRC64)
    flip = bytearray(good)
    flip[-6] ^= 1                                   # the footer's backward size: its CRC32 no longer holds
    return [("good", good), ("checked", X.checked()[0]), ("empty", lzma.compress(b"")), ("flipped_footer", bytes(flip)),
            ("cut_in_index", good[:-16]), ("chained", X.chained()[0]), ("good_again", good)]


@pytest.mark.parametrize("align", [1, 256, 4096])
@pytest.mark.parametrize("chains", [0, 1])
def test_layout_is_the_index_of_every_file_back_to_back(xlz_so, align, chains):
    names, datas = zip(*_layout_files())
    laid, total = lzma_amd.xz_many_layout(datas, chains=chains, align=align)
    assert len(laid) == len(datas)
    end, statuses = 0, {}
    for name, data, (off, cap, st) in zip(names, datas, laid):
        want_st, want_total = M.index_status(data, chains)
        assert st == want_st, name
        assert cap == (want_total if want_st == N.OK else 0), name
        assert off % align == 0 and off == (end + align - 1) // align * align, name  # aligned, ascending, no more room than that
        end = off + cap
        statuses[name] = st
    assert total == end
    assert statuses["good"] == statuses["checked"] == statuses["empty"] == N.OK
    assert statuses["flipped_footer"] == N.ERR_RESULT and statuses["cut_in_index"] < 0
    assert statuses["chained"] == (N.OK if chains else N.ERR_UNSUPPORTED)
    assert laid[2][1] == 0 and laid[0][1] == 5000 and laid[1][1] == len(X.checked()[1])


def test_layout_takes_the_filter_mode_from_a_context(xlz_so):
    class Mode:
        def __init__(self, mode):
            self.mode = mode

        def filter_mode(self):
            return self.mode
    data = X.chained()[0]
    assert lzma_amd.xz_many_layout([data])[0][0][2] == N.ERR_UNSUPPORTED
    assert lzma_amd.xz_many_layout([data], ctx=Mode(0))[0][0][2] == N.ERR_UNSUPPORTED
    assert lzma_amd.xz_many_layout([data], ctx=Mode(1))[0][0] == (0, len(X.chained()[1]), N.OK)
    assert lzma_amd.xz_many_layout([data], chains=False, ctx=Mode(1))[0][0][2] == N.ERR_UNSUPPORTED
    assert lzma_amd.xz_many_layout([]) == ([], 0)


def test_layout_sizes_that_overflow_64_bits(xlz_so):
    huge = M.announces(1 << 62)
    assert M.index_status(huge, 0) == (N.OK, 1 << 62)
    laid, total = lzma_amd.xz_many_layout([huge] * 3)
    assert total == 3 << 62 and [w[0] for w in laid] == [0, 1 << 62, 2 << 62]
    small = lzma.compress(b"x")
    laid, total = lzma_amd.xz_many_layout([huge, huge, huge, M.announces((1 << 62) - 1)])
    assert total == (1 << 64) - 1                   # the largest set that fits
    for datas, align in (([huge] * 4, 1), ([huge] * 3 + [small], 1 << 63), ([small, huge, huge, huge, huge], 1), ([small, small], (1 << 64) - 1)):
        with pytest.raises(LzmaError) as e:
            lzma_amd.xz_many_layout(datas, align=align)
        assert e.value.status == N.ERR_OUT_CAP, align
    # the raw call: the per-file statuses are there, no window is filled in, *total is 0
    with lzma_amd._ManyFiles([huge] * 4, [(7, 7)] * 4) as m:
        total = ctypes.c_uint64(5)
        assert N.lib().xlz_xz_many_layout(m.arr, 4, 0, 1, m.res, ctypes.byref(total)) == N.ERR_OUT_CAP
        assert total.value == 0 and all(m.res[i].status == N.OK and (m.arr[i].dst_off, m.arr[i].dst_cap) == (7, 7) for i in range(4))
        assert N.lib().xlz_xz_many_layout(m.arr, 4, 0, 0, m.res, ctypes.byref(total)) == N.ERR_BAD_ARG  # align 0
        assert N.lib().xlz_xz_many_layout(None, 4, 0, 1, m.res, ctypes.byref(total)) == N.ERR_BAD_ARG
        assert N.lib().xlz_xz_many_layout(m.arr, 4, 0, 1, None, ctypes.byref(total)) == N.ERR_BAD_ARG
        assert N.lib().xlz_xz_many_layout(m.arr, 4, 0, 1, m.res, None) == N.ERR_BAD_ARG
        assert N.lib().xlz_xz_many_layout(None, 0, 0, 1, None, ctypes.byref(total)) == N.OK and total.value == 0


def test_argument_errors_of_a_decode_need_no_device(xlz_so):
    """NULLs, a window past out_cap, overlapping windows, windows of no bytes beside such a fault: XLZ_ERR_BAD_ARG before
    the context is looked at (the one passed here is 64 KiB of zeros that no library call may touch), nothing written --
    not the destination, not results[]; n == 0 is XLZ_OK"""
    L = N.lib()
    a, b = lzma.compress(b"a" * 40), lzma.compress(b"b" * 24)
    not_a_context = ctypes.create_string_buffer(1 << 16)
    big = 1 << 64
    bad = [
        [(0, 40), (39, 24)],                  # the last byte of one is the first of the other
        [(8, 40), (8, 40)],                   # the same window twice
        [(0, 64), (20, 24)],                  # one inside the other
        [(25, 40), (0, 24)],                  # [25, 65) past a capacity of 64
        [(0, 65), (0, 0)],
        [(64, 1), (0, 24)],
        [(big - 1, 2), (0, 24)],              # dst_off + dst_cap wraps
        [(0, 40), (20, big - 1)],
        [(0, 0), (5, big - 6)],               # (no window of bytes may end past out_cap, however far)
        [(0, 40), (10, 0), (64, 0), (big - 1, 0), (30, 24)],  # windows of no bytes overlap nothing: what is left still does
    ]
    for form in ("xlz_xz_decode_many", "xlz_xz_decode_many_device"):
        call = getattr(L, form)
        for windows in bad:
            datas = [a, b] + [a] * (len(windows) - 2)
            out = ctypes.create_string_buffer(b"\xA5" * 64, 64)
            with lzma_amd._ManyFiles(datas, windows) as m:
                for i in range(m.n):
                    m.res[i].status, m.res[i].out_len = 77, 78
                assert call(not_a_context, m.arr, m.n, out, 64, 1, m.res) == N.ERR_BAD_ARG, (form, windows)
                assert all((m.res[i].status, m.res[i].out_len) == (77, 78) for i in range(m.n))
            assert out.raw == b"\xA5" * 64
        with lzma_amd._ManyFiles([a, b], [(0, 40), (40, 24)]) as m:
            out = ctypes.create_string_buffer(b"\xA5" * 64, 64)
            m.res[0].status = 77
            assert call(None, m.arr, 2, out, 64, 1, m.res) == N.ERR_BAD_ARG           # no context
            assert call(not_a_context, None, 2, out, 64, 1, m.res) == N.ERR_BAD_ARG   # no files
            assert call(not_a_context, m.arr, 2, out, 64, 1, None) == N.ERR_BAD_ARG   # no results
            assert call(not_a_context, m.arr, 2, None, 64, 1, m.res) == N.ERR_BAD_ARG  # no destination for 64 bytes
            assert m.res[0].status == 77 and out.raw == b"\xA5" * 64
            # nothing to do: XLZ_OK, whatever else is passed
            assert call(not_a_context, m.arr, 0, out, 64, 1, m.res) == N.OK
            assert call(None, None, 0, None, 0, 1, None) == N.OK
            assert m.res[0].status == 77 and out.raw == b"\xA5" * 64
    assert L.xlz_ctx_last_xz_many_stats(None, None) == N.ERR_BAD_ARG
    assert not_a_context.raw == bytes(1 << 16)


_ABI_PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "xlz.h"
#define S(t) printf(#t " size %zu\n", sizeof(t))
#define F(t, f) printf(#t " " #f " %zu %zu\n", offsetof(t, f), sizeof(((t *)0)->f))
int main(void)
{
    S(xlz_xz_many_file); F(xlz_xz_many_file, file); F(xlz_xz_many_file, len); F(xlz_xz_many_file, dst_off); F(xlz_xz_many_file, dst_cap);
    S(xlz_xz_many_result); F(xlz_xz_many_result, status); F(xlz_xz_many_result, unverified); F(xlz_xz_many_result, out_len);
    F(xlz_xz_many_result, blocks); F(xlz_xz_many_result, comp_bytes);
    S(xlz_xz_many_stats); F(xlz_xz_many_stats, files); F(xlz_xz_many_stats, failed_files); F(xlz_xz_many_stats, blocks);
    F(xlz_xz_many_stats, comp_bytes); F(xlz_xz_many_stats, decoded_bytes);
    return 0;
}
"""


def test_struct_sizes_and_field_offsets_against_a_c_program(tmp_path):
    """include/xlz.h as a C99 compiler lays the new structs out, lzma_amd/_native.py as ctypes does"""
    src, exe = tmp_path / "abi.c", str(tmp_path / "abi")
    src.write_text(_ABI_PROGRAM)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    c = {}
    for line in filter(None, lines):
        t, f, *v = line.split()
        c[(t, f)] = tuple(int(x) for x in v)
    py = {}
    for name, cls in (("xlz_xz_many_file", N.XzManyFile), ("xlz_xz_many_result", N.XzManyResult), ("xlz_xz_many_stats", N.XzManyStats)):
        py[(name, "size")] = (ctypes.sizeof(cls),)
        for f, _ in cls._fields_:
            py[(name, f)] = (getattr(cls, f).offset, getattr(cls, f).size)
    assert py == c
    assert py[("xlz_xz_many_file", "size")] == (32,) and py[("xlz_xz_many_result", "size")] == (32,) and py[("xlz_xz_many_stats", "size")] == (40,)


def test_inputs_are_borrowed_not_copied(tmp_path):
    """bytes, bytearray, memoryview and a read-only mmap: the array points at the callers' own bytes, which stay exported
    until release(); 5000 files make 5000 pointers, no copies"""
    import mmap
    data = lzma.compress(M.text(700))
    arr = bytearray(data)
    path = tmp_path / "f.xz"
    path.write_bytes(data)
    with open(path, "rb") as fh, mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ) as mm:
        srcs = [data, arr, memoryview(data), memoryview(arr)[:], mm]
        assert [w[1:] for w in lzma_amd.xz_many_layout(srcs)[0]] == [(700, N.OK)] * 5
        m = lzma_amd._ManyFiles(srcs)
        assert m.arr[1].file == m.arr[3].file == ctypes.addressof((ctypes.c_char * len(arr)).from_buffer(arr))  # the bytearray's own bytes
        assert all(m.arr[i].len == len(data) for i in range(5))
        with pytest.raises(BufferError):
            arr.append(0)  # (exported: the call reads these very bytes)
        with pytest.raises(BufferError):
            mm.close()
        m.release()
        m.release()
        del srcs  # (its memoryviews export the bytearray too)
        arr.append(0)
    many = lzma_amd._ManyFiles([data] * 5000)
    assert len({many.arr[i].file for i in range(5000)}) == 1
    many.release()
    with pytest.raises(TypeError):
        lzma_amd.xz_many_layout([data, 12345])
    with pytest.raises(BufferError):
        lzma_amd._ManyFiles([memoryview(bytes(64))[::2]])  # not contiguous
    with pytest.raises(ValueError):
        lzma_amd._ManyFiles([data], [])


def test_many_header_is_host_code():
    assert "xlz_xz_many.h" in build.HEADERS and "xlz_xz_many.h" not in build.KERNEL_FILES
    text = open(os.path.join(ROOT, "lzma_amd", "csrc", "xlz_xz_many.h")).read()
    assert "hip" not in text.lower().replace("xlz_xz.hip", "")  # plain C++: nothing of the runtime


def _selftest(tmp_path, flags):
    exe = str(tmp_path / "xz_many_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "lzma_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "xz_many_selftest.cpp"), "-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_windows_layout_map_and_fold_against_a_byte_model(tmp_path, flags):
    out = _selftest(tmp_path, flags)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")
