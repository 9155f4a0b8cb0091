"""GPU: byte ranges of an .xz file (XzFile: xlz_xz_read / xlz_xz_read_device).  The judge is
liblzma through Python: lzma.decompress of the file, sliced.  The files (tests/xz_ranges_files.py) are three concatenated
streams -- CRC64, CRC32, an empty one, SHA-256 -- with stream padding, block sizes on the edges of the 16-byte lane, the
256-byte arena alignment and the 16 KiB pack tile; the same without checks; the same with filter chains on two blocks."""
import ctypes
import os
import sys

import pytest

import lzma_amd
from lzma_amd import LzmaError
from lzma_amd import _native as N

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xz_ranges_files as X  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 64


def _torch():
    import torch
    return torch


def _filled(n):
    torch = _torch()
    t = torch.full((max(n, 1),), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _raw_read(ctx, f, ranges, dptr, cap, verify=True, form="xlz_xz_read_device"):
    """the C call as it is -> (status, copied[], unverified)"""
    copied = (ctypes.c_uint64 * max(len(ranges), 1))(*([7] * max(len(ranges), 1)))
    unverified = ctypes.c_size_t(7)
    st = getattr(N.lib(), form)(ctx._h, f._h, f._ranges(ranges), len(ranges), dptr, cap, copied, 1 if verify else 0, ctypes.byref(unverified))
    return st, list(copied[:len(ranges)]), unverified.value


def _device_read(ctx, f, ranges, verify=True):
    """[(off, n), ...] one behind the other into a filled tensor -> (status, [bytes per range], copied[], unverified)"""
    laid, at = [], 0
    for off, n in ranges:
        laid.append((off, n, at))
        at += max(min(n, f.size - off), 0)
    t = _filled(at)
    st, copied, unverified = _raw_read(ctx, f, laid, ctypes.c_void_p(t.data_ptr()), at, verify)
    got = _bytes(t)
    return st, [got[d:d + c] for (_, _, d), c in zip(laid, copied)], copied, unverified


@pytest.fixture
def mode1(ctx):
    ctx.set_filter_mode(1)
    yield ctx
    ctx.set_filter_mode(0)


def _pairs(f):
    e = X.edges(f.blocks, f.size)
    return [(a, b - a) for a in e for b in e if a <= b]


def test_every_boundary_range_in_one_call(ctx):
    """every (a, b) of block starts and ends +-1 as ONE read_device: destinations one behind the other with 3 bytes between
    them, at an allocation's base + GUARD + 1 (source and destination not congruent), the allocation filled with 0xA5"""
    data, plain = X.checked()
    with lzma_amd.XzFile(data) as f:
        pairs = _pairs(f)
        assert len(pairs) == 861 and sum(n for _, n in pairs) < 48 << 20
        laid, at = [], 0
        for off, n in pairs:
            laid.append((off, n, at))
            at += n + 3
        t = _filled(GUARD + 1 + at + GUARD)
        copied = f.read_device(ctx, laid, t.data_ptr() + GUARD + 1, at)
        assert copied == [n for _, n in pairs]
        got = _bytes(t)
        want = bytearray([FILL]) * len(got)
        for off, n, d in laid:
            want[GUARD + 1 + d: GUARD + 1 + d + n] = plain[off:off + n]
        assert got == bytes(want)  # every range the judge's slice; every gap and guard byte still 0xA5
        rs = ctx.last_xz_read_stats()
        assert rs == {"ranges": 861, "empty_ranges": len([1 for _, n in pairs if n == 0]), "blocks": 14,
                      "comp_bytes": sum(b["comp_len"] for b in f.blocks), "decoded_bytes": f.size, "copied_bytes": sum(copied)}
        assert ctx.last_pack_stats()["bytes"] == sum(copied)


def test_ranges_clipped_at_the_end_in_the_device_form(ctx):
    data, plain = X.checked()
    size = len(plain)
    with lzma_amd.XzFile(data) as f:
        ranges = [(size - 1, 11), (size, 5), (size + 9, 5), (0, 0), (size - 70000, 1 << 63), (5, (1 << 64) - 1)]
        laid, at = [], 0
        for off, n in ranges:
            laid.append((off, n, at))
            at += len(plain[off:off + n]) + 3
        t = _filled(GUARD + at)
        copied = f.read_device(ctx, laid, t.data_ptr() + GUARD, at)
        assert copied == [len(plain[off:off + n]) for off, n in ranges] == [1, 0, 0, 0, 70000, size - 5]
        got = _bytes(t)[GUARD:]
        for (off, n, d), c in zip(laid, copied):
            assert got[d:d + c] == plain[off:off + n] and got[d + c:d + c + 3] == bytes([FILL]) * 3


def test_single_reads_into_host_memory(ctx):
    data, plain = X.checked()
    size = len(plain)
    with lzma_amd.XzFile(data) as f:
        for off, n in _pairs(f)[:12] + [(0, size), (size - 1, 11), (size, 5), (size + 100, 5), (777, 0), (16384, 16385)]:
            assert f.read(ctx, off, n) == plain[off:off + n], (off, n)
        assert f.read(ctx, 0, 1 << 62) == plain
        # several ranges, destinations in another order than the sources, and one staging run where they touch
        ranges = [(70000, 3000), (0, 17), (size - 5, 50), (31, 0), (16, 70000), (0, 17)]
        assert f.read_ranges(ctx, ranges) == [plain[o:o + n] for o, n in ranges]
        assert ctx.last_xz_read_stats()["copied_bytes"] == sum(len(plain[o:o + n]) for o, n in ranges)
        # raw: destinations apart from each other in the caller's buffer, what lies between them is not written
        buf = ctypes.create_string_buffer(bytes([FILL]) * 4096, 4096)
        st, copied, _ = _raw_read(ctx, f, [(300, 100, 1000), (size - 3, 9, 7), (40000, 1, 999), (0, 0, 5000)], buf, 4096, form="xlz_xz_read")
        assert (st, copied) == (N.OK, [100, 3, 1, 0])
        want = bytearray([FILL]) * 4096
        want[1000:1100], want[7:10], want[999:1000] = plain[300:400], plain[size - 3:], plain[40000:40001]
        assert buf.raw == bytes(want)


@pytest.mark.parametrize("name", ["checked", "unchecked", "chained", "reserved"])
def test_a_read_of_everything_is_the_whole_file_call(ctx, name):
    """bytes, status and unverified of read_device([0, size)) and of xz_decode_device, same context; the chain file in
    filter mode 0 (both refuse it) and in mode 1"""
    data, plain = getattr(X, name)()
    L = N.lib()
    with lzma_amd.XzFile(data) as f:
        for mode in (0, 1) if name == "chained" else (0,):
            ctx.set_filter_mode(mode)
            try:
                t = _filled(f.size)
                n, u = ctypes.c_uint64(), ctypes.c_size_t()
                wst = L.xlz_xz_decode_device(ctx._h, ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p), len(data), ctypes.c_void_p(t.data_ptr()),
                                             f.size, ctypes.byref(n), 1, ctypes.byref(u))
                whole = _bytes(t)[:n.value]
                st, got, copied, unverified = _device_read(ctx, f, [(0, f.size)])
            finally:
                ctx.set_filter_mode(0)
            assert (st, unverified) == (wst, u.value)
            if name == "chained" and mode == 0:
                assert st == N.ERR_UNSUPPORTED and copied == [0]
            else:
                assert st == N.OK and got[0] == whole == plain and copied == [f.size]
            assert unverified == (2 if name == "reserved" and st == N.OK else 0)
    if name == "reserved":
        with lzma_amd.XzFile(data) as f:
            assert f.read(ctx, 299, 2) == plain[299:301] and ctx.last_xz_unverified == 2
            assert f.read(ctx, 10, 20) == plain[10:30] and ctx.last_xz_unverified == 1
            assert f.read(ctx, 5300, 20) == plain[5300:5320] and ctx.last_xz_unverified == 0
            assert f.read(ctx, 10, 20, verify=False) == plain[10:30] and ctx.last_xz_unverified == 0


def test_ranges_of_every_file_against_the_judge(mode1):
    ctx = mode1
    for name in ("unchecked", "chained"):
        data, plain = getattr(X, name)()
        with lzma_amd.XzFile(data) as f:
            pairs = _pairs(f)[::7]
            st, got, copied, _ = _device_read(ctx, f, pairs)
            assert st == N.OK and got == [plain[o:o + n] for o, n in pairs], name


def test_filter_modes(ctx):
    data, plain = X.chained()
    with lzma_amd.XzFile(data) as f:
        assert f.steps == 3 and ctx.filter_mode() == 0
        b9, b10, b11 = (f.blocks[k]["uncomp_off"] for k in (9, 10, 11))
        inside_plain = (b10 + 5, 16000)             # block 10 alone: no filter
        touching = [(b10 - 1, 2), (b11, 1), (b10 + 16384, 2), (0, f.size)]
        assert f.cover([inside_plain]) == [10]
        assert f.read(ctx, *inside_plain) == plain[b10 + 5:b10 + 16005]
        assert f.read(ctx, 0, b9) == plain[:b9]      # everything in front of the first filtered block
        before = ctx.last_xz_read_stats()
        for off, n in touching:
            st, _, copied, _ = _device_read(ctx, f, [(off, n)])
            assert (st, copied) == (N.ERR_UNSUPPORTED, [0]), (off, n)
            assert ctx.last_xz_read_stats() == before  # (a refused call makes no statistics)
            with pytest.raises(LzmaError) as e:
                f.read(ctx, off, n)
            assert e.value.status == lzma_amd.ERR_UNSUPPORTED
        ctx.set_filter_mode(1)
        try:
            for off, n in [inside_plain] + touching + [(b9 + 3, 100), (b11 + 69000, 5000)]:
                assert f.read(ctx, off, n) == plain[off:off + n], (off, n)
            assert f.read(ctx, b9 + 100, 10) == plain[b9 + 100:b9 + 110]
            assert ctx.last_filter_stats()["device_steps"] + ctx.last_filter_stats()["host_steps"] == 2  # Delta and ARM of block 9
        finally:
            ctx.set_filter_mode(0)


def test_statistics_say_that_only_the_cover_is_decoded(ctx):
    data, plain = X.checked()
    with lzma_amd.XzFile(data) as f:
        k = 8
        b, nxt = f.blocks[k], f.blocks[k + 1]
        assert f.read(ctx, b["uncomp_off"] + 10, 100) == plain[b["uncomp_off"] + 10:b["uncomp_off"] + 110]
        rs = ctx.last_xz_read_stats()
        assert rs == {"ranges": 1, "empty_ranges": 0, "blocks": 1, "comp_bytes": b["comp_len"], "decoded_bytes": b["uncomp_len"],
                      "copied_bytes": 100}
        assert ctx.last_check_stats()["device_ranges"] + ctx.last_check_stats()["host_ranges"] == 1
        assert ctx.last_check_stats()["device_bytes"] + ctx.last_check_stats()["host_bytes"] == b["uncomp_len"]  # the WHOLE block
        assert ctx.last_pack_stats()["bytes"] == 100
        f.read(ctx, nxt["uncomp_off"] - 1, 2)
        rs = ctx.last_xz_read_stats()
        assert (rs["blocks"], rs["comp_bytes"], rs["decoded_bytes"], rs["copied_bytes"]) == (
            2, b["comp_len"] + nxt["comp_len"], b["uncomp_len"] + nxt["uncomp_len"], 2)
        assert ctx.last_pack_stats()["items"] == 2
        f.read_ranges(ctx, [(b["uncomp_off"], 5), (b["uncomp_off"] + 900, 5), (b["uncomp_off"], 5), (f.size, 4)])
        rs = ctx.last_xz_read_stats()
        assert (rs["ranges"], rs["empty_ranges"], rs["blocks"], rs["comp_bytes"], rs["copied_bytes"]) == (4, 1, 1, b["comp_len"], 15)
        f.read(ctx, 5, 10, verify=False)
        assert ctx.last_check_stats()["device_ranges"] + ctx.last_check_stats()["host_ranges"] == 0
        f.read(ctx, f.size, 10)
        assert ctx.last_xz_read_stats() == {"ranges": 1, "empty_ranges": 1, "blocks": 0, "comp_bytes": 0, "decoded_bytes": 0, "copied_bytes": 0}
        assert ctx.last_pack_stats()["bytes"] == 0


def _flipped(data, at, bit=0x10):
    bad = bytearray(data)
    bad[at] ^= bit
    return bytes(bad)


@pytest.mark.parametrize("k", [10, 13], ids=["crc32_block", "sha256_block"])
def test_damage_is_seen_in_the_cover_only(ctx, k):
    data, plain = X.checked()
    with lzma_amd.XzFile(data) as f:
        b = f.blocks[k]
    lo = b["uncomp_off"]
    inside, outside = [(lo + 7, 1000), (lo + 2000, 10)], [(lo - 3000, 2999), (5, 20)]
    payload = _flipped(data, b["comp_off"] + b["comp_len"] // 2)
    with lzma_amd.XzFile(payload) as f:  # (the index and the headers are whole: the damage is not seen at open)
        assert k not in f.cover(outside)
        assert f.read_ranges(ctx, outside) == [plain[o:o + n] for o, n in outside]
        st, _, copied, _ = _device_read(ctx, f, inside + outside)
        assert st < 0 and copied == [0] * 4
        st, copied, _ = _raw_read(ctx, f, [(o, n, 0) for o, n in inside[:1]], ctypes.create_string_buffer(1000), 1000, form="xlz_xz_read")
        assert st < 0 and copied == [0]
    check = _flipped(data, b["check_off"] + (3 if k == 10 else 31), 0x01)
    with lzma_amd.XzFile(check) as f:
        assert f.read_ranges(ctx, outside) == [plain[o:o + n] for o, n in outside]
        st, _, copied, _ = _device_read(ctx, f, inside)
        assert (st, copied) == (N.ERR_RESULT, [0, 0])
        with pytest.raises(LzmaError) as e:
            f.read(ctx, *inside[0])
        assert e.value.status == lzma_amd.ERR_RESULT
        assert f.read_ranges(ctx, inside, verify=False) == [plain[o:o + n] for o, n in inside]
        st, got, copied, _ = _device_read(ctx, f, inside, verify=False)
        assert st == N.OK and got == [plain[o:o + n] for o, n in inside]


def test_tensor_form(ctx):
    torch = _torch()
    data, plain = X.checked()
    with lzma_amd.XzFile(data) as f:
        t = f.read_tensor(ctx, 4000, 100_000)
        assert isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.device == torch.device("cuda", 0) and t.shape == (100_000,)
        assert _bytes(t) == plain[4000:104_000]
        out = _filled(200_000)
        t = f.read_tensor(ctx, f.size - 70_001, 1 << 40, out=out)
        assert t.data_ptr() == out.data_ptr() and t.shape == (70_001,) and _bytes(t) == plain[-70_001:]
        assert _bytes(out)[70_001:] == bytes([FILL]) * (200_000 - 70_001)
        assert f.read_tensor(ctx, f.size, 10).numel() == 0
        with pytest.raises(LzmaError) as e:
            f.read_tensor(ctx, 0, 1000, out=torch.empty(999, dtype=torch.uint8, device="cuda"))
        assert e.value.status == lzma_amd.ERR_OUT_CAP
        with pytest.raises(ValueError):
            f.read_tensor(ctx, 0, 1000, out=torch.empty(1000, dtype=torch.int8, device="cuda"))


def test_argument_errors_on_a_live_context(ctx):
    """what the CPU tests show with a context that is none, on a real one: refused, nothing written, no statistics made"""
    data, plain = X.checked()
    with lzma_amd.XzFile(data) as f:
        f.read(ctx, 0, 10)
        before = ctx.last_xz_read_stats()
        t = _filled(256)
        for ranges in ([(0, 10, 0), (100, 10, 9)], [(0, 10, 250)], [(f.size - 4, 100, 0), (0, 10, 3)]):
            st, copied, _ = _raw_read(ctx, f, ranges, ctypes.c_void_p(t.data_ptr()), 256)
            assert st == N.ERR_BAD_ARG and copied == [0] * len(ranges)
        assert _bytes(t) == bytes([FILL]) * 256 and ctx.last_xz_read_stats() == before
        # a destination that is host memory
        host = ctypes.create_string_buffer(64)
        st, copied, _ = _raw_read(ctx, f, [(0, 10, 0)], host, 64)
        assert st == N.ERR_BAD_ARG and copied == [0] and host.raw == bytes(64)
        assert ctx.last_xz_read_stats() == before  # (refused before the statistics of the call are made)
