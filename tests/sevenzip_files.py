"""Test infrastructure: .7z archives WITH a FilesInfo section -- names, empty files, directories, anti items, modification
times, attributes -- built from 7-Zip's published format description on top of tests/sevenzip_craft.py's number() and the
folder dicts of tests/sevenzip_bcj2.py (plain_folder / bcj2_folder).  A plain module, not a conftest.

An entry is a dict: name (str; may hold lone surrogates), kind ("file": the next substream is its bytes; "empty": an empty
file; "dir"; "anti": an anti item), mtime (a raw FILETIME or None), attr (Windows attributes or None)."""
import lzma
import struct
import zlib

from sevenzip_craft import (K_CODERS_UNPACK_SIZE, K_CRC, K_ENCODED_HEADER, K_END, K_FILES, K_FOLDER, K_HEADER, K_MAIN_STREAMS,
                            K_NUM_UNPACK_STREAM, K_PACK_INFO, K_SIZE, K_SUBSTREAMS, K_UNPACK_INFO, lzma_folder, number)

K_EMPTY_STREAM, K_EMPTY_FILE, K_ANTI, K_NAMES, K_MTIME, K_ATTRIBUTES, K_DUMMY = 0x0E, 0x0F, 0x10, 0x11, 0x14, 0x15, 0x19
EPOCH = 116444736000000000  # 1970-01-01 as a FILETIME


def filetime(unix_seconds):
    return EPOCH + int(unix_seconds * 10_000_000)


def entry(name, kind="file", mtime=None, attr=None):
    return {"name": name, "kind": kind, "mtime": mtime, "attr": attr}


def bits(flags):
    """a bit vector, MSB first"""
    out = bytearray((len(flags) + 7) // 8)
    for i, f in enumerate(flags):
        if f:
            out[i // 8] |= 0x80 >> (i % 8)
    return bytes(out)


def prop(kind, data):
    return bytes([kind]) + number(len(data)) + data


def utf16(name):
    return name.encode("utf-16-le", "surrogatepass")


def as_utf8(name):
    """what the library hands out for `name`: UTF-8, an unpaired surrogate as U+FFFD"""
    return utf16(name).decode("utf-16-le", "replace")


def values(kind, vals, width):
    """kMTime / kWinAttributes: AllDefined, else a bit vector; External 0; the defined values"""
    defined = [v is not None for v in vals]
    data = b"\x01" if all(defined) else b"\x00" + bits(defined)
    data += b"\x00" + b"".join(v.to_bytes(width, "little") for v in vals if v is not None)
    return prop(kind, data)


def files_info(entries, names=True, dummy=True):
    """the FilesInfo section of `entries`, id byte and end mark included"""
    out = bytes([K_FILES]) + number(len(entries))
    empty = [e["kind"] != "file" for e in entries]
    if any(empty):
        out += prop(K_EMPTY_STREAM, bits(empty))
        ef = [e["kind"] in ("empty", "anti") for e in entries if e["kind"] != "file"]
        if any(ef):
            out += prop(K_EMPTY_FILE, bits(ef))
        anti = [e["kind"] == "anti" for e in entries if e["kind"] != "file"]
        if any(anti):
            out += prop(K_ANTI, bits(anti))
    if dummy:
        out += prop(K_DUMMY, b"\0\0\0")
    if names:
        out += prop(K_NAMES, b"\x00" + b"".join(utf16(e["name"]) + b"\0\0" for e in entries))
    if any(e["mtime"] is not None for e in entries):
        out += values(K_MTIME, [e["mtime"] for e in entries], 8)
    if any(e["attr"] is not None for e in entries):
        out += values(K_ATTRIBUTES, [e["attr"] for e in entries], 4)
    return out + bytes([K_END])


def streams_info(folders, crc_override=None, no_crc=()):
    """folders: dicts of sevenzip_bcj2.plain_folder / bcj2_folder.  Every file carries its own CRC (no folder CRCs) but the
    files whose index over all folders is in no_crc; crc_override: {file index: the CRC32 to write instead}"""
    si = bytes([K_PACK_INFO]) + number(0) + number(sum(len(f["packs"]) for f in folders)) + bytes([K_SIZE])
    si += b"".join(number(len(p)) for f in folders for p in f["packs"]) + bytes([K_END])
    si += bytes([K_UNPACK_INFO, K_FOLDER]) + number(len(folders)) + b"\x00"
    si += b"".join(f["rec"] for f in folders)
    si += bytes([K_CODERS_UNPACK_SIZE]) + b"".join(number(v) for f in folders for v in f["sizes"]) + bytes([K_END])
    si += bytes([K_SUBSTREAMS, K_NUM_UNPACK_STREAM]) + b"".join(number(len(f["files"])) for f in folders)
    sizes = b"".join(number(len(x)) for f in folders for x in f["files"][:-1])
    if sizes:
        si += bytes([K_SIZE]) + sizes
    files = [x for f in folders for x in f["files"]]
    if files:
        defined = [k not in no_crc for k in range(len(files))]
        si += bytes([K_CRC]) + (b"\x01" if all(defined) else b"\x00" + bits(defined))
        si += b"".join(struct.pack("<I", (crc_override or {}).get(k, zlib.crc32(x))) for k, x in enumerate(files) if defined[k])
    return si + bytes([K_END]) + bytes([K_END])


def archive(folders, entries=None, files=None, encoded_header=False, crc_override=None, no_crc=()):
    """-> the bytes of a .7z file.  entries: the FilesInfo of files_info(entries); files: the section's bytes as given (for
    sections a parser must refuse); neither: no FilesInfo.  encoded_header: the header is LZMA-compressed."""
    packed = b"".join(p for f in folders for p in f["packs"])
    header = bytes([K_HEADER])
    if folders:
        header += bytes([K_MAIN_STREAMS]) + streams_info(folders, crc_override, no_crc)
    if files is not None:
        header += files
    elif entries is not None:
        header += files_info(entries)
    header += bytes([K_END])
    body, next_header = packed, header
    if encoded_header:
        rec, hpacked = lzma_folder(header, dict_size=1 << 16)
        enc = bytes([K_ENCODED_HEADER, K_PACK_INFO]) + number(len(packed)) + number(1) + bytes([K_SIZE]) + number(len(hpacked)) + bytes([K_END])
        enc += bytes([K_UNPACK_INFO, K_FOLDER]) + number(1) + b"\x00" + number(1) + rec + bytes([K_CODERS_UNPACK_SIZE]) + \
            number(len(header)) + bytes([K_CRC, 1]) + struct.pack("<I", zlib.crc32(header)) + bytes([K_END]) + bytes([K_END])
        body, next_header = packed + hpacked, enc
    start = struct.pack("<QQI", len(body), len(next_header), zlib.crc32(next_header))
    return b"7z\xbc\xaf\x27\x1c" + bytes([0, 4]) + struct.pack("<I", zlib.crc32(start)) + start + body + next_header


def lzma2_units_folder(parts, dict_byte=10):
    """an LZMA2 folder whose payload is one unit per part: every part compressed on its own (liblzma starts a stream with a
    dictionary reset and new properties; a part liblzma stores starts with a stored chunk that resets the dictionary), the
    streams joined without their end marks -> (coder record, packed bytes)"""
    ds = (2 | (dict_byte & 1)) << (dict_byte // 2 + 11)
    filt = [{"id": lzma.FILTER_LZMA2, "dict_size": ds, "preset": 1}]
    packed = b""
    for part in parts:
        one = lzma.compress(part, format=lzma.FORMAT_RAW, filters=filt)
        assert one[-1] == 0
        packed += one[:-1]
    return bytes([0x21]) + b"\x21" + number(1) + bytes([dict_byte]), packed + b"\x00"
