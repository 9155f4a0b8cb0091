"""Test infrastructure: .7z archives whose folders are coder CHAINS -- Delta / BCJ filters behind one LZMA or LZMA2 coder --
built from 7-Zip's published format description on top of tests/sevenzip_craft.py's number() and archive layout.  The
payloads come from liblzma: lzma.compress(FORMAT_RAW, filters=[filter ..., LZMA1 | LZMA2]).

Every coder has one input (its packed side) and one output (its unpacked side); a bind pair (in, out) says that a coder's
input is another coder's output.  A chain [f1, f2, LZMA] (the encoder's order, liblzma's `filters` list) is decoded LZMA
first, then f2, then f1.  Two layouts of the same line: lzma_first=False lists the coders f1, f2, LZMA with the bind pairs
in 0 <- out 1, in 1 <- out 2 (the packed stream is in 2, the folder's output out 0); lzma_first=True lists them LZMA, f2, f1
with in 1 <- out 0, in 2 <- out 1 (packed stream in 0, output out 2) -- the order libarchive's reader expects."""
import lzma
import struct
import zlib

from sevenzip_craft import (K_CODERS_UNPACK_SIZE, K_CRC, K_END, K_FILES, K_FOLDER, K_HEADER, K_MAIN_STREAMS, K_NAMES,
                            K_NUM_UNPACK_STREAM, K_PACK_INFO, K_SIZE, K_SUBSTREAMS, K_UNPACK_INFO, number)

METHOD = {lzma.FILTER_DELTA: b"\x03", lzma.FILTER_X86: b"\x03\x03\x01\x03", lzma.FILTER_POWERPC: b"\x03\x03\x02\x05",
          lzma.FILTER_IA64: b"\x03\x03\x04\x01", lzma.FILTER_ARM: b"\x03\x03\x05\x01", lzma.FILTER_ARMTHUMB: b"\x03\x03\x07\x01",
          lzma.FILTER_SPARC: b"\x03\x03\x08\x05"}


def filter_coder(f):
    """one filter of liblzma's `filters` list -> its 7z coder record (Delta: one property byte, distance - 1)"""
    m = METHOD[f["id"]]
    if f["id"] == lzma.FILTER_DELTA:
        return bytes([0x20 | len(m)]) + m + number(1) + bytes([f.get("dist", 1) - 1])
    assert not f.get("start_offset"), ".7z has no start offset"
    return bytes([len(m)]) + m


def chain_folder(data, filters, lzma2=False, dict_size=1 << 16, binds=None, lzma_first=False, listed=None):
    """-> (("raw", folder record), packed bytes, number of coders).  filters: liblzma filter dicts in the encoder's order,
    WITHOUT the LZMA coder.  binds overrides the bind pairs, listed the filters the record names (the payload stays what
    `filters` made): for folders the parser must refuse."""
    if lzma2:
        dict_byte = 10
        last = {"id": lzma.FILTER_LZMA2, "dict_size": (2 | (dict_byte & 1)) << (dict_byte // 2 + 11), "preset": 1}
        last_rec = bytes([0x21]) + b"\x21" + number(1) + bytes([dict_byte])
    else:
        last = {"id": lzma.FILTER_LZMA1, "dict_size": dict_size, "lc": 3, "lp": 0, "pb": 2, "preset": 1}
        last_rec = bytes([0x23]) + b"\x03\x01\x01" + number(5) + bytes([(2 * 5 + 0) * 9 + 3]) + struct.pack("<I", dict_size)
    packed = lzma.compress(data, format=lzma.FORMAT_RAW, filters=list(filters) + [last])
    filters = listed if listed is not None else filters
    n = len(filters) + 1
    if lzma_first:
        rec = number(n) + last_rec + b"".join(filter_coder(f) for f in reversed(filters))
        default = [(k + 1, k) for k in range(n - 1)]
    else:
        rec = number(n) + b"".join(filter_coder(f) for f in filters) + last_rec
        default = [(k, k + 1) for k in range(n - 1)]
    for i, o in (binds if binds is not None else default):
        rec += number(i) + number(o)
    return ("raw", rec), packed, n


def archive(folders, folder_crc=True, names=None, sizes_override=None):
    """folders: [(rec, packed, n_coders, [file bytes, ...])] -> the bytes of a .7z file with a plain header.  names: give
    every file a name (a FilesInfo an extractor accepts).  sizes_override: {folder index: [size per output stream]}"""
    packed = b"".join(p for _, p, _, _ in folders)
    si = bytes([K_PACK_INFO]) + number(0) + number(len(folders)) + bytes([K_SIZE])
    si += b"".join(number(len(p)) for _, p, _, _ in folders) + bytes([K_END])
    si += bytes([K_UNPACK_INFO, K_FOLDER]) + number(len(folders)) + b"\x00"
    for rec, _, _, _ in folders:
        si += rec[1] if isinstance(rec, tuple) else number(1) + rec
    si += bytes([K_CODERS_UNPACK_SIZE])
    for k, (_, _, nc, files) in enumerate(folders):
        total = sum(len(f) for f in files)
        for v in (sizes_override or {}).get(k, [total] * nc):
            si += number(v)
    if folder_crc:
        si += bytes([K_CRC, 1]) + b"".join(struct.pack("<I", zlib.crc32(b"".join(f))) for _, _, _, f in folders)
    si += bytes([K_END])
    si += bytes([K_SUBSTREAMS, K_NUM_UNPACK_STREAM]) + b"".join(number(len(f)) for _, _, _, f in folders)
    sizes = b"".join(number(len(x)) for _, _, _, f in folders for x in f[:-1])
    if sizes:
        si += bytes([K_SIZE]) + sizes
    need = [x for _, _, _, f in folders if not (len(f) == 1 and folder_crc) for x in f]
    if need:
        si += bytes([K_CRC, 1]) + b"".join(struct.pack("<I", zlib.crc32(x)) for x in need)
    si += bytes([K_END]) + bytes([K_END])
    header = bytes([K_HEADER, K_MAIN_STREAMS]) + si
    nfiles = sum(len(f) for _, _, _, f in folders)
    if names is not None:
        assert len(names) == nfiles
        blob = b"\x00" + b"".join(n.encode("utf-16-le") + b"\0\0" for n in names)
        header += bytes([K_FILES]) + number(nfiles) + bytes([K_NAMES]) + number(len(blob)) + blob + bytes([K_END])
    else:
        header += bytes([K_FILES]) + number(nfiles) + bytes([0x19]) + number(3) + b"\0\0\0" + bytes([K_END])
    header += bytes([K_END])
    start = struct.pack("<QQI", len(packed), len(header), zlib.crc32(header))
    return b"7z\xbc\xaf\x27\x1c" + bytes([0, 4]) + struct.pack("<I", zlib.crc32(start)) + start + packed + header
