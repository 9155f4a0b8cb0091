"""Expected digests of the device checks' tests: CRC32 from zlib, CRC64 from liblzma.  Python has no CRC64; liblzma's is
taken from the .xz file it writes -- the check of a file's only block is the 8 bytes in front of the index, whose size the
footer's backward size gives.  A plain module, not a conftest."""
import lzma
import zlib

CRC32 = 1
CRC64 = 4


def crc64(data):
    """liblzma's CRC64 of `data` (a few MiB of incompressible bytes take about a second: preset 0)"""
    data = bytes(data)
    if not data:
        return 0   # (an empty file has no block)
    xz = lzma.compress(data, format=lzma.FORMAT_XZ, check=lzma.CHECK_CRC64, preset=0)
    index_size = (int.from_bytes(xz[-8:-4], "little") + 1) * 4
    end = len(xz) - 12 - index_size
    # one block only: liblzma's one-shot encoder writes one block per call
    assert xz[end] == 0 and xz[end + 1] == 1, "more than one block"
    return int.from_bytes(xz[end - 8: end], "little")


def crc32(data):
    return zlib.crc32(bytes(data)) & 0xFFFFFFFF


def digest(kind, data):
    return crc32(data) if kind == CRC32 else crc64(data)
