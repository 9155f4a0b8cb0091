"""GPU: the Adler-32 kernels (lzma_amd/csrc/xlz_adler_dev.hip) through gz.adler32_device.  The judge is zlib.adler32.  The
whole edge list of tests/adler_edges.py is ONE call over one buffer of 4 MiB; then a call of so many short ranges that
every workgroup of the segment kernel makes three grid-stride trips; then the argument rules.  Every range is checked
against the buffer's length before anything is launched: nothing here reads out of range."""
import ctypes
import random
import zlib

import pytest
import torch   # (before libxlz.so is loaded: torch brings its own HIP runtime, which must be the one that initialises the device)

import adler_edges as E
import lzma_amd
from lzma_amd import gz

pytestmark = pytest.mark.gpu

WG_PER_CU, WAVES_PER_WG = 8, 4   # xlz_adler_dev.hip: adler_grid, the segment kernel's workgroup


def _on_device(data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def test_the_whole_edge_list_in_one_call(ctx):
    buf, rs = E.buffer(), E.ranges()
    want = E.expected(buf, rs)
    d = _on_device(buf)
    got = gz.adler32_device(ctx, d.data_ptr(), len(buf), [(off, ln) for off, ln, _ in rs])
    bad = [(rs[k][0], rs[k][1], sorted(rs[k][2]), hex(got[k]), hex(want[k])) for k in range(len(rs)) if got[k] != want[k]]
    assert not bad, bad[:10]
    # the same ranges seen from a pointer that is 5 modulo 16: the kernels round it down and shift the ranges
    shifted = [(off - 5, ln) for off, ln, _ in rs]
    assert gz.adler32_device(ctx, d.data_ptr() + 5, len(buf) - 5, shifted) == want


def test_every_workgroup_makes_three_trips(ctx):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 3 * WG_PER_CU * WAVES_PER_WG * cus + 517
    r = random.Random("adler-trips")
    buf = r.randbytes(1 << 20)
    rs = [(r.randrange(len(buf) - 2048), r.randrange(1024, 2049)) for _ in range(n)]   # they overlap, in no order
    d = _on_device(buf)
    got = gz.adler32_device(ctx, d.data_ptr(), len(buf), rs)
    view = memoryview(buf)
    assert got == [zlib.adler32(view[off:off + ln]) for off, ln in rs]


def test_argument_rules(ctx):
    buf = bytes(range(256)) * 16
    d = _on_device(buf)

    def bad(ptr, buf_len, rs):
        with pytest.raises(lzma_amd.LzmaError) as e:
            gz.adler32_device(ctx, ptr, buf_len, rs)
        assert e.value.status == lzma_amd.ERR_BAD_ARG

    bad(d.data_ptr(), len(buf), [(0, 16), (len(buf) - 10, 11)])       # a range past the end
    bad(d.data_ptr(), len(buf), [(len(buf) + 1, 0)])                  # an empty one outside
    bad(d.data_ptr(), len(buf), [(1, 2 ** 64 - 1)])                   # off + len wraps
    host = ctypes.create_string_buffer(buf, len(buf))
    bad(ctypes.addressof(host), len(buf), [(0, 16)])                  # a host pointer
    bad(0, len(buf), [(0, 16)])                                       # no pointer
    assert gz.adler32_device(ctx, d.data_ptr(), len(buf), []) == []
    assert gz.adler32_device(ctx, d.data_ptr(), len(buf), [(len(buf), 0), (7, 0), (0, len(buf))]) == [1, 1, zlib.adler32(buf)]
