"""Test infrastructure: .7z archives with BCJ2 folders (method 03 03 01 1B), built from 7-Zip's published format description
on top of tests/sevenzip_craft.py's number().  The four streams come from tests/bcj2_ref.py's encoder, the LZMA / LZMA2
payloads from liblzma.  A plain module, not a conftest.

Input and output streams of a folder are numbered through its coders in header order; a bind pair (in, out) says that an
input is another coder's output; the packed-stream index list names, for every packed stream of the folder in file order,
the input it feeds.  BCJ2 has four inputs -- 0 main, 1 call, 2 jump, 3 the range coder's bytes -- and one output.

  form 4, layout "libarchive": coders jump-LZMA, call-LZMA, main-LZMA, BCJ2; bind pairs (5,0) (4,1) (3,2); index list
      2, 6, 1, 0; packed data in file order main, rc, call, jump; unpack sizes jump, call, main, final -- the layout cmake's
      bundled libarchive extracts.
  form 4, layout "7zip": coders BCJ2, main, call, jump; bind pairs (0,1) (1,2) (2,3); index list 4, 5, 6, 3; file order
      main, call, jump, rc; sizes final, main, call, jump -- the order 7-Zip itself lists them in.
  form 2: coders main-LZMA, BCJ2; bind pair (1,0); index list 0, 2, 3, 4; file order main, call, jump, rc (call and jump
      raw); sizes main, final -- the two-coder form of older 7-Zip."""
import lzma
import struct
import zlib

import bcj2_ref
from sevenzip_craft import (K_CODERS_UNPACK_SIZE, K_CRC, K_END, K_FILES, K_FOLDER, K_HEADER, K_MAIN_STREAMS, K_NAMES,
                            K_NUM_UNPACK_STREAM, K_PACK_INFO, K_SIZE, K_SUBSTREAMS, K_UNPACK_INFO, number)

BCJ2_CODER = bytes([0x14]) + b"\x03\x03\x01\x1b" + number(4) + number(1)
DICT_BYTE = 12  # LZMA2: 256 KiB


def sub_coder(data, lzma2, dict_size=1 << 18):
    """-> (coder record, packed bytes) of one LZMA / LZMA2 coder over `data`"""
    if lzma2:
        ds = (2 | (DICT_BYTE & 1)) << (DICT_BYTE // 2 + 11)
        packed = lzma.compress(data, format=lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA2, "dict_size": ds, "preset": 1}])
        return bytes([0x21]) + b"\x21" + number(1) + bytes([DICT_BYTE]), packed
    filt = [{"id": lzma.FILTER_LZMA1, "dict_size": dict_size, "lc": 3, "lp": 0, "pb": 2, "preset": 1}]
    packed = lzma.compress(data, format=lzma.FORMAT_RAW, filters=filt)
    return bytes([0x23]) + b"\x03\x01\x01" + number(5) + bytes([0x5D]) + struct.pack("<I", dict_size), packed


def bcj2_folder(files, form=4, lzma2=False, layout="libarchive", binds=None, index=None, sizes=None, bcj2_coder=BCJ2_CODER,
                main_coder=None, convert=None, streams=None):
    """-> a folder dict for archive().  files: the folder's files (a solid folder when more than one).  binds, index, sizes,
    bcj2_coder, main_coder (a coder record in place of the main stream's LZMA coder) override what the form says: for the
    folders a parser must refuse.  streams: (main, call, jump, rc) in place of the encoder's."""
    data = b"".join(files)
    main, call, jump, rc = streams if streams is not None else bcj2_ref.encode(data, convert)
    mrec, mpk = sub_coder(main, lzma2)
    if main_coder is not None:
        mrec = main_coder
    if form == 4:
        crec, cpk = sub_coder(call, lzma2)
        jrec, jpk = sub_coder(jump, lzma2)
        if layout == "libarchive":
            coders = jrec + crec + mrec + bcj2_coder
            d_binds, d_index, packs = [(5, 0), (4, 1), (3, 2)], [2, 6, 1, 0], [mpk, rc, cpk, jpk]
            d_sizes = [len(jump), len(call), len(main), len(data)]
        else:
            coders = bcj2_coder + mrec + crec + jrec
            d_binds, d_index, packs = [(0, 1), (1, 2), (2, 3)], [4, 5, 6, 3], [mpk, cpk, jpk, rc]
            d_sizes = [len(data), len(main), len(call), len(jump)]
        n = 4
    else:
        coders = mrec + bcj2_coder
        d_binds, d_index, packs, d_sizes, n = [(1, 0)], [0, 2, 3, 4], [mpk, call, jump, rc], [len(main), len(data)], 2
    rec = number(n) + coders
    for i, o in (binds if binds is not None else d_binds):
        rec += number(i) + number(o)
    for i in (index if index is not None else d_index):
        rec += number(i)
    return {"rec": rec, "packs": packs, "sizes": list(sizes if sizes is not None else d_sizes), "files": list(files),
            "streams": (main, call, jump, rc)}


def plain_folder(rec, packed, files, n_coders=1):
    """a folder of tests/sevenzip_craft.py (one coder record) or tests/sevenzip_chains.py (("raw", record)) for archive()"""
    total = sum(len(f) for f in files)
    return {"rec": rec[1] if isinstance(rec, tuple) else number(1) + rec, "packs": [packed], "sizes": [total] * n_coders, "files": list(files)}


def archive(folders, folder_crc=True, names=None, crc_override=None, folder_crc_override=None):
    """folders: dicts of bcj2_folder / plain_folder -> the bytes of a .7z file with a plain header.  names: give every file a
    name (a FilesInfo an extractor accepts).  crc_override: {file index: CRC32 to write instead of the right one} (files
    whose CRC the header lists: all but the single file of a folder with a folder CRC), folder_crc_override: {folder index:
    ...}"""
    packed = b"".join(p for f in folders for p in f["packs"])
    si = bytes([K_PACK_INFO]) + number(0) + number(sum(len(f["packs"]) for f in folders)) + bytes([K_SIZE])
    si += b"".join(number(len(p)) for f in folders for p in f["packs"]) + bytes([K_END])
    si += bytes([K_UNPACK_INFO, K_FOLDER]) + number(len(folders)) + b"\x00"
    si += b"".join(f["rec"] for f in folders)
    si += bytes([K_CODERS_UNPACK_SIZE]) + b"".join(number(v) for f in folders for v in f["sizes"])
    if folder_crc:
        si += bytes([K_CRC, 1]) + b"".join(struct.pack("<I", (folder_crc_override or {}).get(k, zlib.crc32(b"".join(f["files"]))))
                                             for k, f in enumerate(folders))
    si += bytes([K_END])
    si += bytes([K_SUBSTREAMS, K_NUM_UNPACK_STREAM]) + b"".join(number(len(f["files"])) for f in folders)
    sizes = b"".join(number(len(x)) for f in folders for x in f["files"][:-1])
    if sizes:
        si += bytes([K_SIZE]) + sizes
    crcs, at = [], 0
    for f in folders:
        for x in f["files"]:
            if not (len(f["files"]) == 1 and folder_crc):
                crcs.append((crc_override or {}).get(at, zlib.crc32(x)))
            at += 1
    if crcs:
        si += bytes([K_CRC, 1]) + b"".join(struct.pack("<I", c) for c in crcs)
    si += bytes([K_END]) + bytes([K_END])
    header = bytes([K_HEADER, K_MAIN_STREAMS]) + si
    nfiles = sum(len(f["files"]) for f in folders)
    if names is not None:
        assert len(names) == nfiles
        blob = b"\x00" + b"".join(n.encode("utf-16-le") + b"\0\0" for n in names)
        header += bytes([K_FILES]) + number(nfiles) + bytes([K_NAMES]) + number(len(blob)) + blob + bytes([K_END])
    else:
        header += bytes([K_FILES]) + number(nfiles) + bytes([0x19]) + number(3) + b"\0\0\0" + bytes([K_END])
    header += bytes([K_END])
    start = struct.pack("<QQI", len(packed), len(header), zlib.crc32(header))
    return b"7z\xbc\xaf\x27\x1c" + bytes([0, 4]) + struct.pack("<I", zlib.crc32(start)) + start + packed + header
