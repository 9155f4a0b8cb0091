"""CPU: byte ranges of an .xz file (include/xlz.h: xlz_xz_open / xlz_xz_cover / xlz_xz_read) as
far as no device is needed.  The handle: xlz_xz_open returns what xlz_xz_index_chains returns, on every .xz fixture, on
malformed and cut files; info and blocks are the index's; close, and close again.  The cover against a scan of every
(range, block) pair, on the fixed multi-stream file and on 2000 seeded random files.  The argument errors of a read, which
are settled before the context is used.  And the shared header (lzma_amd/csrc/xlz_xz_cover.h) in a g++ program of its
own -- cover and pack items against a byte-wise model --, plain and under the host sanitizers."""
import ctypes
import glob
import lzma
import os
import random
import subprocess
import sys

import pytest

import lzma_amd
from lzma_amd import _native as N
from lzma_amd import LzmaError, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import xz_chains  # noqa: E402
import xz_ranges_files as X  # noqa: E402


def _index_status(data):
    buf = ctypes.create_string_buffer(data, len(data)) if len(data) else ctypes.create_string_buffer(1)
    n, ns, total = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_uint64()
    return N.lib().xlz_xz_index_chains(ctypes.cast(buf, ctypes.c_void_p), len(data), None, 0, ctypes.byref(n), None, 0, ctypes.byref(ns),
                                       ctypes.byref(total))


def _open_status(data):
    buf = ctypes.create_string_buffer(data, len(data)) if len(data) else ctypes.create_string_buffer(1)
    h = ctypes.c_void_p()
    st = N.lib().xlz_xz_open(ctypes.cast(buf, ctypes.c_void_p), len(data), ctypes.byref(h))
    assert bool(h) == (st == N.OK)
    N.lib().xlz_xz_close(h)
    return st


def _inputs():
    """name -> bytes: the .xz fixtures, the malformed files tests/test_xz_container.py makes, truncations"""
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "**", "*.xz"), recursive=True)):  # (whichever there are)
        out[os.path.relpath(path, ROOT)] = open(path, "rb").read()
    f = X.checked()[0]
    out.update({"fixed": f, "unchecked": X.unchecked()[0], "chained": X.chained()[0]})
    out.update({"minus_1": f[:-1], "half": f[: len(f) // 2], "from_1": f[1:], "empty": b"", "zeros": bytes(64)})
    for cut in (4, 11, 12, 31, 32, 100, len(f) - 4, len(f) - 12, len(f) - 13):
        out["cut_%d" % cut] = f[:cut]
    flip = bytearray(f)
    flip[-20] ^= 1
    out["flip_index"] = bytes(flip)
    flip = bytearray(f)
    flip[14] ^= 0x10  # the first block's header
    out["flip_block_header"] = bytes(flip)
    out["bcj"] = lzma.compress(b"\x90" * 5000, format=lzma.FORMAT_XZ, filters=[{"id": lzma.FILTER_X86}, {"id": lzma.FILTER_LZMA2, "preset": 1}])
    out["arm64"] = xz_chains.stream([(b"abc" * 100, [X.L2])], header_of={0: [(0x0A, b""), (0x21, bytes([xz_chains.DICT_BYTE]))]})
    out["no_blocks"] = lzma.compress(b"")
    out["padded"] = lzma.compress(b"x" * 10) + bytes(12)
    out["bad_padding"] = lzma.compress(b"x" * 10) + bytes(6)
    out.update(_wrapping_indexes())
    return out


def _wrapping_indexes():
    """an index whose record sizes wrap 64 bits (four records of 2^62 beside the real one), as tests/test_xz_container.py crafts it"""
    import struct
    import zlib
    good = lzma.compress(bytes(range(256)) * 20, format=lzma.FORMAT_XZ, check=lzma.CHECK_CRC32)
    ix = len(good) - 12 - (struct.unpack("<I", good[-8:-4])[0] + 1) * 4
    pos, vals = ix + 2, []
    for _ in range(2):
        v, sh = 0, 0
        while True:
            b = good[pos]
            pos += 1
            v |= (b & 0x7F) << sh
            sh += 7
            if not b & 0x80:
                break
        vals.append(v)
    out = {}
    for order in ("huge_first", "huge_last"):
        recs = [(1 << 62, 1)] * 4
        recs = recs + [tuple(vals)] if order == "huge_first" else [tuple(vals)] + recs
        body = b"\x00" + xz_chains.vli(len(recs)) + b"".join(xz_chains.vli(a) + xz_chains.vli(b) for a, b in recs)
        body += bytes(-len(body) % 4)
        index = body + struct.pack("<I", zlib.crc32(body))
        backward = struct.pack("<I", len(index) // 4 - 1)
        flags = good[-4:-2]
        out["wrap_" + order] = good[:ix] + index + struct.pack("<I", zlib.crc32(backward + flags)) + backward + flags + b"YZ"
    return out


def test_open_on_every_structural_bit_flip():
    """single-bit flips in the stream header, the block header, the block padding, the index and the footer of one file per
    check type (the flips of tests/test_xz_container.py): open says what the index says, whatever that is"""
    p = bytes((i * 7 + i // 13) % 251 for i in range(3001))
    refused = 0
    for chk in (lzma.CHECK_NONE, lzma.CHECK_CRC32, lzma.CHECK_CRC64, lzma.CHECK_SHA256):
        x = lzma.compress(p, format=lzma.FORMAT_XZ, check=chk, preset=0)
        n = len(x)
        b0 = lzma_amd.xz_index(x)[0][0]
        index_len = (int.from_bytes(x[n - 8:n - 4], "little") + 1) * 4
        for i in list(range(0, b0["comp_off"])) + list(range(b0["comp_off"] + b0["comp_len"], b0["check_off"])) + list(range(n - 12 - index_len, n)):
            for bit in range(8):
                y = bytearray(x)
                y[i] ^= 1 << bit
                st = _index_status(bytes(y))
                assert _open_status(bytes(y)) == st, (chk, i, bit)
                refused += st != N.OK
    assert refused > 1000


def test_data_is_borrowed_not_copied(tmp_path):
    """bytes, bytearray, memoryview and a read-only mmap: the same index from each, and the buffer stays exported until close()"""
    import mmap
    data = X.checked()[0]
    want = lzma_amd.xz_index_chains(data)[0]
    arr = bytearray(data)
    path = tmp_path / "f.xz"
    path.write_bytes(data)
    with open(path, "rb") as fh, mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ) as mm:
        for src in (data, arr, memoryview(data), memoryview(arr)[:], mm):
            with lzma_amd.XzFile(src) as f:
                assert f.blocks == want and f.cover([(0, f.size)]) == list(range(14))
        f = lzma_amd.XzFile(arr)
        with pytest.raises(BufferError):
            arr.append(0)  # (exported: the handle reads these very bytes)
        f.close()
        arr.append(0)
        f = lzma_amd.XzFile(mm)
        with pytest.raises(BufferError):
            mm.close()
        f.close()
    with pytest.raises(TypeError):
        lzma_amd.XzFile(12345)


def test_open_returns_what_the_index_returns():
    seen = set()
    for name, data in _inputs().items():
        st = _index_status(data)
        assert _open_status(data) == st, name
        seen.add(st)
    assert {N.OK, N.ERR_RESULT, N.ERR_UNEXPECTED_EOF, N.ERR_UNSUPPORTED} <= seen  # (the inputs reach every status of the parse)


def test_info_and_blocks_are_the_index():
    for name, data in _inputs().items():
        if _index_status(data) != N.OK:
            with pytest.raises(LzmaError) as e:
                lzma_amd.XzFile(data)
            assert e.value.status == _index_status(data), name
            continue
        blocks, steps, total = lzma_amd.xz_index_chains(data)
        with lzma_amd.XzFile(data) as f:
            assert (f.size, f.blocks, f.steps) == (total, blocks, len(steps)), name
            # the table in pieces: XLZ_ERR_OUT_CAP says there is more, what fits is filled in
            if len(blocks) > 1:
                part = (N.XzBlock * 1)()
                assert N.lib().xlz_xz_file_blocks(f._h, part, 1) == N.ERR_OUT_CAP
                assert part[0].comp_off == blocks[0]["comp_off"] and part[0].uncomp_len == blocks[0]["uncomp_len"]
    f = lzma_amd.XzFile(X.chained()[0])
    assert f.steps == 3 and len(f.blocks) == 14 and f.size == len(X.chained()[1])


def test_open_close_and_null_arguments():
    L = N.lib()
    data = X.checked()[0]
    f = lzma_amd.XzFile(data)
    f.close()
    f.close()
    with pytest.raises(LzmaError) as e:
        f.cover([(0, 1)])
    assert e.value.status == lzma_amd.ERR_CLOSED
    with lzma_amd.XzFile(data) as g:
        assert g.cover([(0, 1)]) == [0]
    assert not g._h
    L.xlz_xz_close(None)
    h = ctypes.c_void_p()
    assert L.xlz_xz_open(ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p), len(data), None) == N.ERR_BAD_ARG
    assert L.xlz_xz_open(None, 0, ctypes.byref(h)) == N.ERR_BAD_ARG and not h
    assert L.xlz_xz_file_info(None, None, None, None) == N.ERR_BAD_ARG
    assert L.xlz_xz_file_blocks(None, None, 0) == N.ERR_BAD_ARG
    with lzma_amd.XzFile(data) as g:
        n = ctypes.c_size_t(77)
        one = (N.XzRange * 1)((0, 1, 0))
        assert L.xlz_xz_file_info(g._h, None, None, None) == N.OK
        assert L.xlz_xz_file_blocks(g._h, None, 1) == N.ERR_BAD_ARG
        assert L.xlz_xz_cover(None, one, 1, None, 0, ctypes.byref(n)) == N.ERR_BAD_ARG
        assert L.xlz_xz_cover(g._h, None, 1, None, 0, ctypes.byref(n)) == N.ERR_BAD_ARG
        assert L.xlz_xz_cover(g._h, one, 1, None, 0, None) == N.ERR_BAD_ARG
        assert L.xlz_xz_cover(g._h, one, 1, None, 1, ctypes.byref(n)) == N.ERR_BAD_ARG
        assert L.xlz_xz_cover(g._h, None, 0, None, 0, ctypes.byref(n)) == N.OK and n.value == 0
        # the count alone, then too little room
        whole = (N.XzRange * 1)((0, g.size, 0))
        assert L.xlz_xz_cover(g._h, whole, 1, None, 0, ctypes.byref(n)) == N.OK and n.value == 14
        few = (ctypes.c_size_t * 3)()
        assert L.xlz_xz_cover(g._h, whole, 1, few, 3, ctypes.byref(n)) == N.ERR_OUT_CAP and n.value == 14 and list(few) == [0, 1, 2]
        # a read: no context, no file, no ranges, no destination
        out = ctypes.create_string_buffer(16)
        copied = (ctypes.c_uint64 * 1)(5)
        assert L.xlz_xz_read(None, g._h, one, 1, out, 16, copied, 1, None) == N.ERR_BAD_ARG and copied[0] == 0
        assert L.xlz_xz_read_device(None, g._h, one, 1, out, 16, copied, 1, None) == N.ERR_BAD_ARG
        assert L.xlz_ctx_last_xz_read_stats(None, None) == N.ERR_BAD_ARG
        assert out.raw == bytes(16)


def _extents(blocks):
    return [(b["uncomp_off"], b["uncomp_len"]) for b in blocks]


def test_cover_of_the_fixed_file():
    data, plain = X.checked()
    with lzma_amd.XzFile(data) as f:
        ext, size = _extents(f.blocks), f.size
        assert size == len(plain) == sum(X.SIZES_A + X.SIZES_B + X.SIZES_C)
        e = X.edges(f.blocks, size)
        for a in e:
            for b in e:
                if a <= b:
                    assert f.cover([(a, b - a)]) == X.brute_cover(ext, size, [(a, b - a)]), (a, b)
        big = 1 << 64
        cases = [[], [(0, 0)], [(size, 5)], [(size + 1, 5)], [(size - 1, big - size)], [(5, big - 1)], [(big - 1, big - 1)], [(0, size)],
                 [(17, 0), (size, 0)], [(32, 17), (32, 17)], [(70000, 3), (3, 3), (70000, 3)], [(0, 1), (size - 1, 1)],
                 [(ext[5][0], ext[5][1])], [(ext[5][0] - 1, 1)], [(ext[5][0] + ext[5][1], 1)], [(ext[5][0] + ext[5][1] - 1, 2)]]
        for ranges in cases:
            assert f.cover(ranges) == X.brute_cover(ext, size, ranges), ranges
        assert f.cover([(0, size)]) == list(range(14)) and f.cover([(size, 5)]) == [] and f.cover([(32, 17), (32, 17)]) == [3]
        assert f.cover([(48, 2), (31, 1)]) == [2, 3, 4]


def test_cover_on_2000_random_files():
    """seeded (block sizes, ranges): empty blocks and ranges, ranges at, behind and across the end, off + len past 2^64,
    ranges that begin or end on a block boundary, duplicates, streams without blocks"""
    rnd = random.Random(314159)
    big = 1 << 64
    for case in range(2000):
        streams = []
        for _ in range(rnd.randrange(1, 4)):
            sizes = [0 if rnd.randrange(5) == 0 else rnd.randrange(1, 300) for _ in range(rnd.randrange(0, 6))]
            streams.append(xz_chains.stream([(bytes(n), [X.L2]) for n in sizes], check=lzma.CHECK_NONE) + bytes(4 * rnd.randrange(3)))
        with lzma_amd.XzFile(b"".join(streams)) as f:
            ext, size = _extents(f.blocks), f.size
            marks = [0, size, size + 1, big - 1] + [v + d for o, n in ext for v in (o, o + n) for d in (-1, 0, 1) if 0 <= v + d]
            ranges = []
            for _ in range(rnd.randrange(0, 7)):
                kind = rnd.randrange(6)
                off = rnd.choice(marks) if kind < 3 else rnd.randrange(size + 3)
                n = 0 if kind == 0 else big - 1 - rnd.randrange(3) if kind == 1 else max(rnd.choice(marks) - off, 0) % big if kind == 2 else rnd.randrange(size + 3)
                ranges.append((off, n))
                if ranges and rnd.randrange(4) == 0:
                    ranges.append(rnd.choice(ranges))
            assert f.cover(ranges) == X.brute_cover(ext, size, ranges), (case, ext, ranges)


def test_argument_errors_of_a_read_need_no_device():
    """overlapping destinations, a destination past out_cap: XLZ_ERR_BAD_ARG before the context is looked at (the one
    passed here is 64 KiB of zeros that no library call may touch), nothing written, every copied[i] 0"""
    L = N.lib()
    data, _ = X.checked()
    not_a_context = ctypes.create_string_buffer(1 << 16)
    with lzma_amd.XzFile(data) as f:
        size = f.size
        bad = [
            [(0, 10, 0), (100, 10, 9)],            # the last byte of one is the first of the other
            [(0, 10, 5), (0, 10, 5)],              # the same destination twice
            [(0, 100, 0), (7, 1, 50)],             # one inside the other
            [(size - 4, 100, 0), (0, 10, 3)],      # clipped to 4 bytes: [0, 4) and [3, 13)
            [(0, 10, 55)],                         # [55, 65) past a capacity of 64
            [(0, 65, 0)],
            [(0, 1, 64)],
            [(0, 2, (1 << 64) - 1)],               # dst_off + len wraps
            [(0, 0, 0), (5, 5, 1 << 63), (size, 9, 0)],
        ]
        for form in ("xlz_xz_read", "xlz_xz_read_device"):
            for ranges in bad:
                out = ctypes.create_string_buffer(b"\xA5" * 64, 64)
                copied = (ctypes.c_uint64 * len(ranges))(*([7] * len(ranges)))
                unverified = ctypes.c_size_t(9)
                st = getattr(L, form)(not_a_context, f._h, f._ranges(ranges), len(ranges), out, 64, copied, 1, ctypes.byref(unverified))
                assert st == N.ERR_BAD_ARG, (form, ranges)
                assert out.raw == b"\xA5" * 64 and list(copied) == [0] * len(ranges)
            # ranges that are clipped to nothing declare no byte: what is left overlaps, so the call is still refused
            st = getattr(L, form)(not_a_context, f._h, f._ranges([(size, 5, 0), (0, 4, 0), (1, 4, 3)]), 3, out, 64, None, 0, None)
            assert st == N.ERR_BAD_ARG
        assert not_a_context.raw == bytes(1 << 16)


def test_cover_header_is_host_code():
    assert "xlz_xz_cover.h" in build.HEADERS and "xlz_xz_cover.h" not in build.KERNEL_FILES


def _selftest(tmp_path, flags):
    exe = str(tmp_path / "xz_cover_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "lzma_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "xz_cover_selftest.cpp"), "-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_cover_and_pack_items_against_a_byte_model(tmp_path, flags):
    out = _selftest(tmp_path, flags)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")
