"""Test infrastructure of the many-file tests (xz_decode_many): the small .xz files they share, the damaged ones, and the
single-file calls that judge status, out_len and unverified.  A plain module, not a conftest.  The judge for bytes is
liblzma through Python (lzma.decompress, stream by stream where a file has several)."""
import ctypes
import functools
import lzma
import struct
import zlib

import xz_chains
import xz_ranges_files as X

from lzma_amd import _native as N


def text(n, seed=0):
    """n bytes that compress: lines of words picked by a small generator"""
    words = [b"alpha", b"beta", b"gamma", b"delta", b"epsilon", b"zeta", b"eta", b"theta", b"iota", b"kappa", b"lambda", b"mu"]
    out, v = bytearray(), seed * 2654435761 + 12345
    while len(out) < n:
        v = (v * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        out += words[(v >> 33) % len(words)] + (b"\n" if (v >> 40) % 7 == 0 else b" ")
    return bytes(out[:n])


@functools.lru_cache(maxsize=None)
def good():
    """name -> (file, decoded): the seven files of the equality test but the chains file (X.chained(), filter mode 1)"""
    one = b"Z"
    mid = text(16385, 1)
    none = text(3000, 2)
    return {
        "crc64_1_byte": (lzma.compress(one, format=lzma.FORMAT_XZ, check=lzma.CHECK_CRC64), one),
        "crc32_16385": (lzma.compress(mid, format=lzma.FORMAT_XZ, check=lzma.CHECK_CRC32), mid),
        "checked": X.checked(),          # 14 blocks over CRC64 / CRC32 / SHA-256 streams, an empty stream, padding
        "check_none": (lzma.compress(none, format=lzma.FORMAT_XZ, check=lzma.CHECK_NONE), none),
        "reserved": X.reserved(),        # two blocks under a reserved check id, one under CRC32
        "empty": (lzma.compress(b""), b""),
    }


def first_block(data):
    import lzma_amd
    return lzma_amd.xz_index(data)[0][0]


@functools.lru_cache(maxsize=None)
def bad():
    """name -> file: a payload byte flipped so that the block decodes to its size but fails its CRC (a literal inside an
    uncompressed LZMA2 chunk); an LZMA2 chunk header with properties that no decoder accepts (the block's own status: XLZ_ERR_PROPS); a file cut short"""
    plain = bytes(range(256)) * 8
    # one block of ONE stored LZMA2 chunk, made by hand: control 0x01, size - 1, the bytes, then the end marker 0x00
    stored = b"\x01" + struct.pack(">H", len(plain) - 1) + plain + b"\x00"
    flags = bytes([0, lzma.CHECK_CRC32])
    hdr = xz_chains.block_header([(0x21, bytes([xz_chains.DICT_BYTE]))])
    chk = struct.pack("<I", zlib.crc32(plain))
    body = hdr + stored + bytes(-len(stored) % 4) + chk
    index = b"\x00" + xz_chains.vli(1) + xz_chains.vli(len(hdr) + len(stored) + len(chk)) + xz_chains.vli(len(plain))
    index += bytes(-len(index) % 4)
    index += struct.pack("<I", zlib.crc32(index))
    foot = struct.pack("<I", len(index) // 4 - 1) + flags
    whole = b"\xfd7zXZ\x00" + flags + struct.pack("<I", zlib.crc32(flags)) + body + index + struct.pack("<I", zlib.crc32(foot)) + foot + b"YZ"
    assert lzma.decompress(whole) == plain  # (liblzma reads it back)
    b0 = first_block(whole)
    crc = bytearray(whole)
    crc[b0["comp_off"] + 3 + 1000] ^= 0x40            # a stored byte: the block still decodes to 2048 bytes
    chunk = bytearray(whole)
    chunk[b0["comp_off"]] = 0xE0                      # an LZMA chunk that resets everything and brings new properties ...
    chunk[b0["comp_off"] + 5] = 0xFF                  # ... which no decoder accepts (lc / lp / pb byte of 225 and more)
    checked = X.checked()[0]
    return {"bad_crc": bytes(crc), "bad_chunk": bytes(chunk), "cut": checked[:len(checked) - 40]}


@functools.lru_cache(maxsize=None)
def announces(size):
    """a well-formed one-block file whose index announces `size` decoded bytes (its block holds 5120)"""
    ok = lzma.compress(bytes(range(256)) * 20, format=lzma.FORMAT_XZ, check=lzma.CHECK_CRC32)
    ix = len(ok) - 12 - (struct.unpack("<I", ok[-8:-4])[0] + 1) * 4
    pos, unpadded, sh = ix + 2, 0, 0
    while True:
        b = ok[pos]
        pos += 1
        unpadded |= (b & 0x7F) << sh
        sh += 7
        if not b & 0x80:
            break
    body = b"\x00" + xz_chains.vli(1) + xz_chains.vli(unpadded) + xz_chains.vli(size)
    body += bytes(-len(body) % 4)
    index = body + struct.pack("<I", zlib.crc32(body))
    backward = struct.pack("<I", len(index) // 4 - 1)
    flags = ok[-4:-2]
    return ok[:ix] + index + struct.pack("<I", zlib.crc32(backward + flags)) + backward + flags + b"YZ"


def index_status(data, chains):
    """what xlz_xz_index (chains false) / xlz_xz_index_chains returns -> (status, total)"""
    buf = ctypes.create_string_buffer(data, len(data)) if len(data) else ctypes.create_string_buffer(1)
    n, ns, total = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_uint64()
    p = ctypes.cast(buf, ctypes.c_void_p)
    if chains:
        st = N.lib().xlz_xz_index_chains(p, len(data), None, 0, ctypes.byref(n), None, 0, ctypes.byref(ns), ctypes.byref(total))
    else:
        st = N.lib().xlz_xz_index(p, len(data), None, 0, ctypes.byref(n), ctypes.byref(total))
    return st, total.value


def single(ctx, data, cap, device=False, verify=True):
    """the single-file front-end alone on `ctx`, into a buffer of `cap` bytes -> (status, out_len, unverified, bytes)"""
    n, u = ctypes.c_uint64(99), ctypes.c_size_t(99)
    src = ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p)
    if device:
        import torch
        t = torch.zeros(max(cap, 1), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        st = N.lib().xlz_xz_decode_device(ctx._h, src, len(data), ctypes.c_void_p(t.data_ptr()), cap, ctypes.byref(n), 1 if verify else 0,
                                          ctypes.byref(u))
        got = t.cpu().numpy().tobytes()
    else:
        out = ctypes.create_string_buffer(max(cap, 1))
        st = N.lib().xlz_xz_decode(ctx._h, src, len(data), out, cap, ctypes.byref(n), 1 if verify else 0, ctypes.byref(u))
        got = out.raw
    if st != N.OK:
        return st, 0, 0, None  # (what the single call leaves in *out_len and *unverified on a failure is not part of the comparison)
    return st, n.value, u.value, got[:n.value]
