"""Archives for the .zip front-end's tests (test_zip_cpu.py, test_gpu_zip.py), written three ways: by Python's zipfile
(the independent writer for method 14, ZIP64 and data descriptors), by hand from PKWARE's APPNOTE (what zipfile never
writes: method 14 without an end marker, local extras that differ from the central ones, and every defect), and once by
Info-ZIP (tests/golden/infozip.zip, recipe: tests/golden/make_infozip_zip.py).  Entry sizes are small on purpose: the
edges of the 16-byte lane, of the 256-byte arena alignment and of the 16 KiB pack tile, and one entry of 70 001 bytes."""
import functools
import io
import lzma
import os
import struct
import sys
import zipfile
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import corpus  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = [0, 1, 15, 16, 17, 255, 256, 257, 16383, 16384, 16385, 70001]
DATE = (2024, 2, 29, 13, 37, 42)


def text(seed, n):
    return corpus.plain_text(seed, n) if n else b""


def noise(seed, n):
    return corpus.plain_random(seed, n) if n else b""


# ---------------------------------------------------------------- with zipfile ----
def _info(name, method, date=DATE):
    zi = zipfile.ZipInfo(name, date_time=date)
    zi.compress_type = method
    zi.external_attr = 0o644 << 16
    return zi


@functools.lru_cache(maxsize=None)
def mixed():
    """every size as an LZMA entry (text) and as a stored entry (noise), a directory, a deflate entry, a non-ASCII name"""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w") as z:
        z.writestr(_info("dir/", zipfile.ZIP_STORED), b"")
        for k, n in enumerate(SIZES):
            z.writestr(_info("dir/lzma_%d.txt" % n, zipfile.ZIP_LZMA), text(100 + k, n))
            z.writestr(_info("s%d.bin" % n, zipfile.ZIP_STORED), noise(200 + k, n))
        z.writestr(_info("deflated.txt", zipfile.ZIP_DEFLATED), text(7, 3000))
        z.writestr(_info("grüß/世界.txt", zipfile.ZIP_LZMA, (1999, 12, 31, 23, 59, 58)), text(8, 999))
        z.comment = b"a comment"
    return buf.getvalue()


class _Unseekable(io.RawIOBase):
    def __init__(self):
        self.buf = bytearray()

    def writable(self):
        return True

    def write(self, b):
        self.buf += b
        return len(b)


@functools.lru_cache(maxsize=None)
def descriptors():
    """through an unseekable writer: every entry carries a data descriptor, its local header holds zeros"""
    w = _Unseekable()
    with zipfile.ZipFile(w, "w") as z:
        for k, n in enumerate([1, 17, 4097, 16385]):
            with z.open(_info("d_lzma_%d" % n, zipfile.ZIP_LZMA), "w") as f:
                f.write(text(300 + k, n))
            with z.open(_info("d_stored_%d" % n, zipfile.ZIP_STORED), "w") as f:
                f.write(noise(310 + k, n))
    return bytes(w.buf)


@functools.lru_cache(maxsize=None)
def forced_zip64():
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w") as z:
        for k, n in enumerate([0, 5, 300, 16385]):
            for method, nm in ((zipfile.ZIP_LZMA, "z64_lzma_%d"), (zipfile.ZIP_STORED, "z64_stored_%d")):
                with z.open(_info(nm % n, method), "w", force_zip64=True) as f:
                    f.write(text(320 + k, n))
    return buf.getvalue()


# ---------------------------------------------------------------- by hand ----
def lzma_payload(data, marker=True, prop_size=5, props=None, preset=6):
    """a method-14 payload: version, property size, lc/lp/pb, dictionary size, the raw stream -- with an end marker
    (liblzma's .lzma stream behind its 13-byte header) or without one (corpus.alone_known_size_no_eos)"""
    if marker:
        alone = lzma.compress(data, format=lzma.FORMAT_ALONE, filters=corpus.lzma1_filters(preset=preset))
    else:
        alone = corpus.alone_known_size_no_eos(data)
        assert alone is not None, "needs a plaintext that liblzma packs into one LZMA2 chunk"
    head = bytes([alone[0] if props is None else props]) + alone[1:5]
    return struct.pack("<BBH", 9, 20, prop_size) + head + alone[13:]


class Hand:
    """one archive written record by record; every field can be overridden per entry"""

    def __init__(self, prepend=b""):
        self.body = bytearray(prepend)
        self.start = len(prepend)  # offsets are declared from here
        self.central = []
        self.plain = []  # per entry: its bytes, or None where nobody can know them

    def add(self, name, payload, size, crc, method, flags=0, local_extra=b"", central_extra=b"", comp_size=None, header_off=None,
            plain=None, date=DATE, attr=0o644 << 16, zip64=False, local_sig=b"PK\x03\x04"):
        name = name.encode() if isinstance(name, str) else name
        t = date[3] << 11 | date[4] << 5 | date[5] // 2
        d = (date[0] - 1980) << 9 | date[1] << 5 | date[2]
        comp = len(payload) if comp_size is None else comp_size
        off = len(self.body) - self.start if header_off is None else header_off
        lsize, lcomp = (0xFFFFFFFF, 0xFFFFFFFF) if zip64 else (size, comp)
        if zip64:
            local_extra = struct.pack("<HHQQ", 1, 16, size, comp) + local_extra
            central_extra = struct.pack("<HHQQQ", 1, 24, size, comp, off) + central_extra
        self.body += local_sig + struct.pack("<HHHHHIIIHH", 63, flags, method, t, d, crc, lcomp, lsize, len(name), len(local_extra))
        self.body += name + local_extra + payload
        coff = 0xFFFFFFFF if zip64 else off
        self.central.append(b"PK\x01\x02" + struct.pack("<HHHHHHIIIHHHHHII", 63, 63, flags, method, t, d, crc, lcomp, lsize, len(name),
                                                      len(central_extra), 0, 0, 0, attr, coff) + name + central_extra)
        self.plain.append(plain)
        return len(self.central) - 1

    def lzma(self, name, data, marker=True, **kw):
        kw.setdefault("size", len(data))
        kw.setdefault("crc", zlib.crc32(data))
        return self.add(name, kw.pop("payload", None) or lzma_payload(data, marker), method=14, flags=kw.pop("flags", 0) | (2 if marker else 0),
                        plain=data, **kw)

    def stored(self, name, data, **kw):
        kw.setdefault("size", len(data))
        kw.setdefault("crc", zlib.crc32(data))
        return self.add(name, data, method=0, plain=data, **kw)

    def finish(self, comment=b"", trailing=b"", zip64=False, ones=False, disk=0, cd_disk=0, n_here=None, n_all=None, locator_disks=1):
        cd = b"".join(self.central)
        cd_off = len(self.body) - self.start
        n = len(self.central)
        n_here = n if n_here is None else n_here
        n_all = n if n_all is None else n_all
        out = bytes(self.body) + cd
        if zip64:
            at = len(out) - self.start
            out += b"PK\x06\x06" + struct.pack("<QHHIIQQQQ", 44, 45, 45, disk, cd_disk, n_here, n_all, len(cd), cd_off)
            out += b"PK\x06\x07" + struct.pack("<IQI", 0, at, locator_disks)
        if ones:  # (the 32-bit end record of a ZIP64 archive may say nothing at all)
            out += b"PK\x05\x06" + struct.pack("<HHHHIIH", 0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF, 0xFFFFFFFF, 0xFFFFFFFF, len(comment))
        else:
            out += b"PK\x05\x06" + struct.pack("<HHHHIIH", 0 if zip64 else disk, 0 if zip64 else cd_disk, min(n_here, 0xFFFF),
                                             min(n_all, 0xFFFF), min(len(cd), 0xFFFFFFFF), min(cd_off, 0xFFFFFFFF), len(comment))
        return out + comment + trailing


@functools.lru_cache(maxsize=None)
def residues(n=300):
    """about 300 small entries, LZMA with and without end marker and stored, whose name and extra lengths walk the payloads
    over every offset modulo 16; the local extra field is NOT the central one -> (archive, plaintexts)"""
    h = Hand()
    sizes = [1, 2, 15, 16, 17, 31, 33, 100, 255, 256, 257, 300, 1000]
    for i in range(n):
        data = text(1000 + i, sizes[i % len(sizes)])
        name = "r%03d" % i + "x" * (i % 7)
        le = struct.pack("<HH", 0x7075 + 0, i % 5) + b"\0" * (i % 5)  # (an unknown field, another length than the central one)
        ce = struct.pack("<HH", 0x5455, 0) if i % 2 else b""
        if i % 3 == 0 or (i % 3 == 1 and len(data) < 100):  # (liblzma packs no shorter text into a compressed LZMA2 chunk)
            h.lzma(name, data, marker=True, local_extra=le, central_extra=ce)
        elif i % 3 == 1:
            h.lzma(name, data, marker=False, local_extra=le, central_extra=ce)
        else:
            h.stored(name, noise(2000 + i, len(data)), local_extra=le, central_extra=ce)
    return h.finish(), list(h.plain)


def both_markers():
    """the same plaintexts as LZMA entries with the end marker and without -> (archive, plaintexts per pair)"""
    h = Hand()
    plains = [bytes([65 + n % 3]) * n for n in SIZES if 1 < n < 255] + [text(400 + k, n) for k, n in enumerate(SIZES) if n >= 255]
    for k, p in enumerate(plains):
        h.lzma("m%d" % k, p, marker=True)
        h.lzma("n%d" % k, p, marker=False)
    return h.finish(), plains


@functools.lru_cache(maxsize=None)
def damaged():
    """good entries with one defect each between them -> (archive, {name: (index, kind)}, plaintexts or None)"""
    h = Hand()
    what = {}

    def good(tag):
        k = len(h.central)
        h.lzma("good_%s_a" % tag, text(500 + k, 700 + k))
        h.stored("good_%s_b" % tag, noise(500 + k, 40 + k))

    def note(name, idx, kind):
        what[name] = (idx, kind)
        h.plain[idx] = None

    p = text(600, 5000)
    good("0")
    note("flipped", h.lzma("flipped", p), "stream_or_crc")
    good("1")
    note("wrong_crc", h.lzma("wrong_crc", p, crc=zlib.crc32(p) ^ 1), "crc")
    note("wrong_crc_stored", h.stored("wrong_crc_stored", noise(601, 333), crc=5), "crc")
    good("2")
    note("cut", h.lzma("cut", p, comp_size=len(lzma_payload(p)) - 40), "stream_or_crc")
    good("3")
    note("marker_size_small", h.lzma("marker_size_small", p, size=len(p) - 1), "result")
    note("marker_size_large", h.lzma("marker_size_large", p, size=len(p) + 1), "result")
    good("4")
    note("no_marker_size_large", h.lzma("no_marker_size_large", p, marker=False, size=len(p) + 1), "stream_or_crc")
    good("5")
    c = zlib.compressobj(9, zlib.DEFLATED, -15)
    note("deflate", h.add("deflate", c.compress(p) + c.flush(), len(p), zlib.crc32(p), 8), "unsupported")
    note("xz_in_zip", h.add("xz_in_zip", lzma.compress(p), len(p), zlib.crc32(p), 95), "unsupported")
    note("encrypted", h.lzma("encrypted", p, flags=1), "unsupported")
    note("stored_sizes_differ", h.stored("stored_sizes_differ", noise(602, 50), size=49), "unsupported")
    good("6")
    note("prop_size_4", h.lzma("prop_size_4", p, payload=lzma_payload(p, prop_size=4)), "bad")
    note("props_225", h.lzma("props_225", p, payload=lzma_payload(p, props=225)), "bad")
    note("short_lzma", h.lzma("short_lzma", p, comp_size=8), "bad")
    note("offset_out", h.stored("offset_out", b"abc", header_off=1 << 30), "bad")
    note("no_local_sig", h.stored("no_local_sig", b"abcd", local_sig=b"PK\x03\x05"), "bad")
    note("data_out", h.stored("data_out", b"abcde", size=1 << 24, comp_size=1 << 24), "bad")
    good("7")
    arc = bytearray(h.finish())
    # the flipped byte: in the middle of the entry's raw stream
    with zipfile.ZipFile(io.BytesIO(bytes(arc))) as z:
        zi = z.infolist()[what["flipped"][0]]
    at = zi.header_offset + 30 + len(zi.filename) + 9 + (zi.compress_size - 9) // 2
    arc[at] ^= 0x40
    return bytes(arc), what, list(h.plain)


def many_stored(n, lo=1, hi=1, zip64=None):
    """n stored entries of lo .. hi bytes (more than 65 535 entries need the ZIP64 end record) -> (archive, plaintexts)"""
    h = Hand()
    blob = noise(700, n + hi)
    for i in range(n):
        size = lo + (i * 7919) % (hi - lo + 1)
        h.stored("%x" % i, blob[i:i + size])
    return h.finish(zip64=n > 0xFFFF if zip64 is None else zip64), list(h.plain)


def small():
    """three entries by hand, the base of the end-record variants"""
    h = Hand()
    h.lzma("a", text(800, 100))
    h.stored("b", noise(801, 33))
    h.lzma("c", text(802, 257), marker=False)
    return h


def end_variants():
    """{name: archive}: what open must accept"""
    out = {
        "comment_65535": small().finish(comment=b"c" * 65535),
        "trailing": small().finish(comment=b"xy", trailing=b"\0" * 517),
        "zip64_ones": small().finish(zip64=True, ones=True),
        "zip64_entries": None,
    }
    h = Hand(b"#!stub\n" + b"\x90" * 993)
    h.lzma("a", text(800, 100))
    h.stored("b", noise(801, 33), zip64=True)
    out["prepended_1000"] = h.finish()
    h = Hand(b"S" * 1000)
    h.lzma("a", text(800, 100), zip64=True)
    h.stored("b", noise(801, 33))
    out["prepended_1000_zip64"] = h.finish(zip64=True)
    h = small()
    h.stored("z", noise(803, 77), zip64=True)
    out["zip64_entries"] = h.finish()
    return out


def end_defects():
    """{name: (archive, status name)}: what open must refuse, and with what"""
    good = small().finish()
    cd = good.index(b"PK\x01\x02")
    eocd = good.rindex(b"PK\x05\x06")
    bad_sig = bytearray(good)
    bad_sig[cd + 2] = 7
    second = good.index(b"PK\x01\x02", cd + 4)
    bad_sig2 = bytearray(good)
    bad_sig2[second + 3] = 9
    return {
        "multi_disk": (small().finish(disk=1), "ERR_UNSUPPORTED"),
        "multi_disk_cd": (small().finish(cd_disk=2), "ERR_UNSUPPORTED"),
        "counts_differ": (small().finish(n_here=2), "ERR_UNSUPPORTED"),
        "multi_disk_zip64": (small().finish(zip64=True, disk=3), "ERR_UNSUPPORTED"),
        "locator_two_disks": (small().finish(zip64=True, locator_disks=2), "ERR_UNSUPPORTED"),
        "empty_file": (b"", "ERR_UNEXPECTED_EOF"),
        "short_file": (good[-21:], "ERR_UNEXPECTED_EOF"),
        "cut_front": (good[eocd - 10:], "ERR_UNEXPECTED_EOF"),       # the directory is longer than what lies in front
        "no_end_record": (good[:eocd] + b"\0" * 22, "ERR_RESULT"),
        "bad_first_signature": (bytes(bad_sig), "ERR_RESULT"),
        "bad_second_signature": (bytes(bad_sig2), "ERR_RESULT"),
        "count_too_small": (small().finish(n_here=2, n_all=2), "ERR_RESULT"),
        "count_too_large": (small().finish(n_here=4, n_all=4), "ERR_RESULT"),
        "record_leaves_directory": (good[:eocd - 1] + good[eocd:eocd + 12] + struct.pack("<II", eocd - cd - 1, cd) + good[eocd + 20:],
                                    "ERR_UNEXPECTED_EOF"),
        "locator_without_record": (good[:eocd] + b"PK\x06\x07" + struct.pack("<IQI", 0, 5, 1) + good[eocd:], "ERR_RESULT"),
    }


def infozip():
    return open(os.path.join(GOLDEN, "infozip.zip"), "rb").read()
