"""Test infrastructure of the byte-range tests (XzFile): the fixed multi-stream files, their judge and the brute-force
cover.  A plain module, not a conftest.  The files come from the writer in xz_chains.py; the judge is liblzma through
Python, stream by stream (lzma.decompress stops at stream padding), concatenated."""
import functools
import hashlib
import lzma
import random

import filter_ref
import xz_chains

L2 = {"id": lzma.FILTER_LZMA2}
# block sizes on the edges of the 16-byte lane, the 256-byte arena alignment and the 16 KiB pack tile
SIZES_A = (1, 15, 16, 17, 255, 256, 257)          # CRC64
SIZES_B = (4096, 16383, 16384, 16385, 70001)      # CRC32
SIZES_C = (33, 65536)                             # SHA-256
PADDING = bytes(8)                                # behind the first stream


RESERVED_CHECK = 2  # a check id the format reserves (a 4-byte field nobody can verify)


def _stream(blocks, check):
    """xz_chains.stream, which knows neither a SHA-256 check field nor a reserved one: its check_bytes is stood in for
    while it runs"""
    if check not in (lzma.CHECK_SHA256, RESERVED_CHECK):
        return xz_chains.stream(blocks, check=check)
    keep = xz_chains.check_bytes
    xz_chains.check_bytes = lambda check, data: hashlib.sha256(data).digest() if check == lzma.CHECK_SHA256 else b"\x01\x02\x03\x04"
    try:
        return xz_chains.stream(blocks, check=check)
    finally:
        xz_chains.check_bytes = keep


def _content(k, n):
    return filter_ref.text(n, seed=100 + k) if k % 2 == 0 else random.Random(1000 + k).randbytes(n)


def _build(checks, chains):
    """-> (file, decoded) of streams A, B, an empty stream, C; 8 bytes of stream padding behind A.  chains: {block index:
    [filters in front of LZMA2]}"""
    parts, plain, k = [], [], 0
    for sizes, check in zip((SIZES_A, SIZES_B, (), SIZES_C), checks):
        blocks = []
        for n in sizes:
            blocks.append((_content(k, n), list(chains.get(k, ())) + [L2]))
            k += 1
        s = _stream(blocks, check)
        assert lzma.decompress(s) == b"".join(b for b, _ in blocks)  # liblzma reads every stream back
        parts.append(s)
        plain.append(lzma.decompress(s))
    return parts[0] + PADDING + b"".join(parts[1:]), b"".join(plain)


@functools.lru_cache(maxsize=None)
def checked():
    return _build((lzma.CHECK_CRC64, lzma.CHECK_CRC32, lzma.CHECK_CRC32, lzma.CHECK_SHA256), {})


@functools.lru_cache(maxsize=None)
def unchecked():
    return _build((lzma.CHECK_NONE,) * 4, {})


# Delta(3) + ARM + LZMA2 on the 16384-byte block (index 9), x86 + LZMA2 on the 70001-byte block (index 11): both hold
# random bytes, in which either BCJ filter finds opcodes to convert
CHAIN_BLOCKS = {9: ({"id": lzma.FILTER_DELTA, "dist": 3}, {"id": lzma.FILTER_ARM}), 11: ({"id": lzma.FILTER_X86},)}


@functools.lru_cache(maxsize=None)
def chained():
    return _build((lzma.CHECK_CRC64, lzma.CHECK_CRC32, lzma.CHECK_CRC32, lzma.CHECK_SHA256), CHAIN_BLOCKS)


@functools.lru_cache(maxsize=None)
def reserved():
    """two blocks under a reserved check id, then one under CRC32 -> (file, decoded)"""
    a = [(_content(0, 300), [L2]), (_content(1, 5000), [L2])]
    b = [(_content(2, 777), [L2])]
    return _stream(a, RESERVED_CHECK) + _stream(b, lzma.CHECK_CRC32), b"".join(d for d, _ in a + b)


def brute_cover(extents, size, ranges):
    """the blocks [(off, len), ...] that share a byte with a range [(off, n), ...] clipped to `size`: every pair looked at"""
    hit = set()
    for off, n in ranges:
        lo, hi = min(off, size), min(off + n, size)
        for i, (b, m) in enumerate(extents):
            if max(lo, b) < min(hi, b + m):
                hit.add(i)
    return sorted(hit)


def edges(blocks, size):
    """every block start and end, and one byte to either side, inside [0, size]"""
    e = set()
    for b in blocks:
        for v in (b["uncomp_off"], b["uncomp_off"] + b["uncomp_len"]):
            e.update(x for x in (v - 1, v, v + 1) if 0 <= x <= size)
    return sorted(e)
