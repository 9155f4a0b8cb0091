"""The .tar archives of the tar tests (tests/test_tar_walk_cpu.py, tests/test_gpu_tar.py) and their judge, Python's tarfile.
Everything is made in memory and is deterministic; nothing here needs a device."""
import functools
import io
import os
import tarfile

MTIME = 1_700_000_000
LONG = "a" * 118 + "é" + "/" + "b" * 60  # 120 + 60 bytes: ustar splits it into prefix and name


def judge(image):
    """what tarfile reports: [(name, linkname, size, type, mode, uid, gid, int(mtime), offset, offset_data)]"""
    with tarfile.open(fileobj=io.BytesIO(image), mode="r:") as t:
        return [(m.name, m.linkname, m.size, m.type, m.mode, m.uid, m.gid, int(m.mtime), m.offset, m.offset_data) for m in t.getmembers()]


def rows(entries):
    """the same tuples of a list of lzma_amd.TarEntry"""
    return [(e.name, e.linkname, e.size, e.type, e.mode, e.uid, e.gid, int(e.mtime), e.hdr_off, e.data_off) for e in entries]


def serial_flag(block):
    """the serial classifier, in Python"""
    if block == bytes(512):
        return 2
    body = block[:148] + b" " * 8 + block[156:]
    u, s = sum(body), sum(b - 256 if b >= 128 else b for b in body)
    f = block[148:156].lstrip(b" ")
    digits = f[:len(f) - len(f.lstrip(b"01234567"))]
    if not 1 <= len(digits) <= 7 or f[len(digits):].strip(b" \0"):
        return 0
    return 1 if int(digits, 8) in (u, s) else 0


def _info(name, type=tarfile.REGTYPE, size=0, linkname="", mode=0o644):
    ti = tarfile.TarInfo(name)
    ti.type, ti.size, ti.linkname, ti.mode, ti.mtime, ti.uid, ti.gid, ti.uname, ti.gname = type, size, linkname, mode, MTIME, 1000, 100, "user", "grp"
    return ti


def _write(fmt, add, **kw):
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w", format=fmt, **kw) as t:
        add(t)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def inner():
    """the tar that is stored as a member: three small files"""
    def add(t):
        for i in range(3):
            body = bytes([65 + i]) * (100 + 300 * i)
            t.addfile(_info("inner/%d.txt" % i, size=len(body)), io.BytesIO(body))
    return _write(tarfile.USTAR_FORMAT, add)


def _standard(t):
    t.addfile(_info("empty.txt"))
    t.addfile(_info("dir", type=tarfile.DIRTYPE, mode=0o755))
    t.addfile(_info("dir/f513.bin", size=513), io.BytesIO(bytes(range(256)) * 2 + b"!"))
    t.addfile(_info(LONG, size=7), io.BytesIO(b"longnam"))
    t.addfile(_info("dir/sym", type=tarfile.SYMTYPE, linkname="t" * 90))
    t.addfile(_info("dir/hard", type=tarfile.LNKTYPE, linkname="dir/f513.bin"))
    t.addfile(_info("c8.bin", size=512), io.BytesIO(b"\xc8" * 512))
    t.addfile(_info("inner.tar", size=len(inner())), io.BytesIO(inner()))
    t.addfile(_info("last.txt", size=3), io.BytesIO(b"end"))


@functools.lru_cache(maxsize=None)
def standard(fmt):
    """fmt: 'ustar', 'gnu' or 'pax' -> the image"""
    return _write({"ustar": tarfile.USTAR_FORMAT, "gnu": tarfile.GNU_FORMAT, "pax": tarfile.PAX_FORMAT}[fmt], _standard)


@functools.lru_cache(maxsize=None)
def gnu_long():
    """a 300-byte name and a 300-byte link target: 'L' and 'K' in front of one member"""
    def add(t):
        t.addfile(_info("first", size=5), io.BytesIO(b"first"))
        t.addfile(_info("n" * 300, type=tarfile.SYMTYPE, linkname="k" * 300))
        t.addfile(_info("d" * 150 + "/", type=tarfile.DIRTYPE, mode=0o755))
        t.addfile(_info("x" * 299 + "é", size=600), io.BytesIO(b"z" * 600))
    return _write(tarfile.GNU_FORMAT, add)


def header(name=b"", size=0, type=b"0", linkname=b"", mode=0o644, uid=1000, gid=100, mtime=MTIME, size_field=None, prefix=b"", magic=b"ustar\x0000"):
    """one hand-built 512-byte header with a right checksum"""
    h = bytearray(512)
    h[0:len(name)] = name
    h[100:108], h[108:116], h[116:124] = b"%07o\0" % mode, b"%07o\0" % uid, b"%07o\0" % gid
    h[124:136] = size_field if size_field is not None else b"%011o\0" % size
    h[136:148] = b"%011o\0" % mtime
    h[156:157] = type
    h[157:157 + len(linkname)] = linkname
    h[257:257 + len(magic)] = magic
    h[345:345 + len(prefix)] = prefix
    h[148:156] = b" " * 8
    h[148:156] = b"%06o\0 " % sum(h)
    return bytes(h)


def padded(data):
    return data + bytes(-len(data) % 512)


def member(name, body=b"", **kw):
    return header(name, size=len(body), **kw) + padded(body)


def pax_records(pairs):
    out = b""
    for k, v in pairs:
        body = b" " + k + b"=" + v + b"\n"
        n = len(body) + 1
        while len(b"%d" % n) + len(body) != n:
            n = len(b"%d" % n) + len(body)
        out += b"%d" % n + body
    return out


END = bytes(1024)


@functools.lru_cache(maxsize=None)
def pax_global_size():
    """a global header (comment, gid), then a member whose 'x' header moves its size from 0 to 700 and names it, then a plain one"""
    g = pax_records([(b"comment", b"made by hand"), (b"gid", b"4242")])
    x = pax_records([(b"path", b"renamed/by/pax/"), (b"size", b"700"), (b"mtime", b"1600000000.25"), (b"uid", b"70000"), (b"atime", b"1.5")])
    return (member(b"g-header", g, type=b"g") + member(b"x-header", x, type=b"x") + header(b"short", size=0) + padded(b"s" * 700) +
            member(b"plain", b"p" * 10) + END)


@functools.lru_cache(maxsize=None)
def crafted():
    """hand-built headers: a base-256 size, a '\\0' type with a trailing slash (and a size field that counts nothing), types
    '3'-'6' with a non-zero size field and no data, an unknown type letter with data, a '\\0' type file, a ustar prefix"""
    out = member(b"big256", b"B" * 1000, size_field=b"\x80" + (1000).to_bytes(11, "big"))
    out += header(b"olddir/", size=512, type=b"\0")
    for t in b"3456":
        out += header(b"node%c" % t, size=4096, type=bytes([t]))
    out += member(b"unknown", b"U" * 600, type=b"Z")
    out += member(b"oldfile", b"O" * 20, type=b"\0", magic=b"")
    out += member(b"leaf", b"L" * 5, prefix=b"some/prefix")
    out += member(b"dirs///", type=b"5")
    return out + END


@functools.lru_cache(maxsize=None)
def libarchive(fmt):
    """'gnutar' or 'pax' by libarchive through `cmake -E tar`: a second writer (tests/golden/make_libarchive_tar.py)"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "libarchive_%s.tar" % fmt), "rb") as f:
        return f.read()


def everything():
    """{name: image} of every well-formed archive above"""
    out = {"ustar": standard("ustar"), "gnu": standard("gnu"), "pax": standard("pax"), "gnu_long": gnu_long(), "pax_global_size": pax_global_size(),
           "crafted": crafted(), "empty": END}
    for fmt in ("gnutar", "pax"):
        out["libarchive_" + fmt] = libarchive(fmt)
    return out


def damaged():
    """{name: (image, end_status name, number of members listed)}: archives that do not end cleanly"""
    g = standard("gnu")
    members = judge(g)
    third = members[2]
    flipped = bytearray(g)
    flipped[third[8] + 20] ^= 0x01  # a byte of the third header's name field
    f513 = members[2]
    sparse = member(b"ok", b"1") + member(b"sparse", b"S" * 100, type=b"S") + END
    bad_pax = member(b"ok", b"1") + member(b"x", b"13 path=abc\n", type=b"x") + member(b"f", b"2") + END
    huge = member(b"ok", b"1") + header(b"huge", size_field=b"\x80\0\0\0" + (1 << 63).to_bytes(8, "big")) + END
    meta2m = member(b"ok", b"1") + member(b"././@LongLink", b"n" * (2 << 20), type=b"L") + member(b"f", b"2") + END
    return {
        "cut_in_header": (g[:third[8] + 100], "ERR_UNEXPECTED_EOF", 2),
        "cut_in_data": (g[:f513[9] + 200], "ERR_UNEXPECTED_EOF", 2),
        "cut_behind_member": (g[:f513[9] + 1024], "OK", 3),
        "flipped_third_header": (bytes(flipped), "ERR_RESULT", 2),
        "sparse": (sparse, "ERR_UNSUPPORTED", 1),
        "bad_pax_length": (bad_pax, "ERR_RESULT", 1),
        "size_2_63": (huge, "ERR_UNEXPECTED_EOF", 1),
        "meta_2mib": (meta2m, "ERR_RESULT", 1),
    }
