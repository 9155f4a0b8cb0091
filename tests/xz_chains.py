"""Test infrastructure: an .xz WRITER for files whose blocks carry filter chains, from "The .xz File Format" 1.0.4.  The
payload of a block is liblzma's -- lzma.compress(FORMAT_RAW, filters=[...]) --, everything around it (block header, check,
index, stream header and footer) is assembled here, so that a file can have several blocks with different chains and a
block header can say something liblzma would never write.  liblzma reads the well-formed ones back (tests check that)."""
import lzma
import struct
import zlib

import check_ref

BCJ = (lzma.FILTER_X86, lzma.FILTER_POWERPC, lzma.FILTER_IA64, lzma.FILTER_ARM, lzma.FILTER_ARMTHUMB, lzma.FILTER_SPARC)
LZMA2 = {"id": lzma.FILTER_LZMA2, "preset": 1, "dict_size": 1 << 20}
DICT_BYTE = 18  # 1 MiB


def vli(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def filter_flags(f):
    """one liblzma filter dict -> (id, property bytes) as a block header carries them"""
    if f["id"] == lzma.FILTER_LZMA2:
        return 0x21, bytes([DICT_BYTE])
    if f["id"] == lzma.FILTER_DELTA:
        return 0x03, bytes([f.get("dist", 1) - 1])
    so = f.get("start_offset", 0)
    return f["id"], struct.pack("<I", so) if so else b""


def block_header(flags_list):
    """[(filter id, property bytes), ...] -> a block header without the optional sizes"""
    body = bytes([len(flags_list) - 1])
    for fid, props in flags_list:
        body += vli(fid) + vli(len(props)) + props
    size = (1 + len(body) + 4 + 3) // 4 * 4
    hdr = bytes([size // 4 - 1]) + body
    hdr += bytes(size - 4 - len(hdr))
    return hdr + struct.pack("<I", zlib.crc32(hdr))


def check_bytes(check, data):
    if check == lzma.CHECK_CRC32:
        return struct.pack("<I", zlib.crc32(data))
    if check == lzma.CHECK_CRC64:
        return struct.pack("<Q", check_ref.crc64(data))
    assert check == lzma.CHECK_NONE
    return b""


def stream(blocks, check=lzma.CHECK_CRC64, header_of=None):
    """blocks: [(plaintext, [liblzma filter dicts, LZMA2 last])] -> one .xz stream.  header_of: {block index: [(id, props), ...]}
    replaces that block's header (the payload stays what the block's filters made)"""
    flags = bytes([0, check])
    out = b"\xfd7zXZ\x00" + flags + struct.pack("<I", zlib.crc32(flags))
    records = b""
    for k, (data, filters) in enumerate(blocks):
        payload = lzma.compress(data, format=lzma.FORMAT_RAW, filters=[dict(f, **LZMA2) if f["id"] == lzma.FILTER_LZMA2 else f for f in filters])
        hdr = block_header((header_of or {}).get(k) or [filter_flags(f) for f in filters])
        chk = check_bytes(check, data)
        out += hdr + payload + bytes(-len(payload) % 4) + chk
        records += vli(len(hdr) + len(payload) + len(chk)) + vli(len(data))
    index = b"\x00" + vli(len(blocks)) + records
    index += bytes(-len(index) % 4)
    index += struct.pack("<I", zlib.crc32(index))
    foot = struct.pack("<I", len(index) // 4 - 1) + flags
    return out + index + struct.pack("<I", zlib.crc32(foot)) + foot + b"YZ"


def decoder_steps(blocks):
    """what xz_index_chains must report for stream(blocks): [(block index, filter id, parameter)] in decoder order"""
    out = []
    for k, (_, filters) in enumerate(blocks):
        for f in reversed(filters[:-1]):
            out.append((k, f["id"], f.get("dist", 1) if f["id"] == lzma.FILTER_DELTA else f.get("start_offset", 0)))
    return out
