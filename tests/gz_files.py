"""gzip, BGZF and zlib test files, built at test time with Python's zlib / struct (no golden files, a seeded RNG, named
cases), and the judges the gz tests compare with: gzip.decompress, zlib.decompressobj.

Two classes of cases differ from Python's gzip ON PURPOSE (SPECIAL below): a wrong FHCRC with verify on, and reserved FLG
bits -- Python ignores both, the library refuses them.  A case whose only defect is a wrong check value (check_only) is
judged by its undamaged twin when verify is off: the judges always verify."""
import gzip
import random
import struct
import zlib
from collections import namedtuple

OK, ERR_RESULT, ERR_UNEXPECTED_EOF, ERR_OUT_CAP, ERR_UNSUPPORTED = 0, -1, -5, -6, -9
AUTO, GZIP, ZLIB = 0, 1, 2
FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT = 1, 2, 4, 8, 16

# the two classes where the library's rule is not Python's, and the status the issue sets for each (verify on)
SPECIAL = {"wrong_fhcrc": ERR_RESULT, "reserved_flg": ERR_UNSUPPORTED}

Case = namedtuple("Case", "name data cap special check_only clean")


def case(name, data, cap, special=None, check_only=False, clean=None):
    assert special is None or special in SPECIAL
    return Case(name, bytes(data), cap, special, check_only, clean)


def payload(seed, n):
    """n bytes that deflate finds something in: runs of a small alphabet, repeats of earlier pieces, some noise"""
    r = random.Random("gz-payload-%s" % (seed,))
    out = bytearray()
    while len(out) < n:
        k = r.randrange(4)
        if k == 0:
            out += r.randbytes(r.randrange(1, 40))
        elif k == 1:
            out += bytes(r.choices(b"acgtn \n", k=r.randrange(1, 200)))
        elif k == 2 and out:
            at = r.randrange(len(out))
            out += out[at:at + r.randrange(3, 300)]
        else:
            out += bytes([r.randrange(256)]) * r.randrange(1, 70)
    return bytes(out[:n])


def raw_deflate(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def header(flg=0, extra=b"", name=b"", comment=b"", mtime=0, hcrc=None, cm=8):
    """a member header; extra / name / comment are written iff their FLG bit is set; hcrc: the FHCRC value (None: the right
    one)"""
    h = bytearray(struct.pack("<BBBBIBB", 0x1F, 0x8B, cm, flg, mtime, 0, 255))
    if flg & FEXTRA:
        h += struct.pack("<H", len(extra)) + extra
    if flg & FNAME:
        h += name + b"\0"
    if flg & FCOMMENT:
        h += comment + b"\0"
    if flg & FHCRC:
        h += struct.pack("<H", (zlib.crc32(bytes(h)) & 0xFFFF) if hcrc is None else hcrc)
    return bytes(h)


def trailer(data, crc_xor=0, isize_add=0):
    return struct.pack("<II", zlib.crc32(data) ^ crc_xor, (len(data) + isize_add) & 0xFFFFFFFF)


def member(data, level=6, **kw):
    return header(**kw) + raw_deflate(data, level) + trailer(data)


def subfield(si, data):
    return si + struct.pack("<H", len(data)) + data


def bgzf_block(data, level=6, more_extra=b"", bc_first=True, crc_xor=0, isize_add=0, body_pad=b"", bsize_add=0):
    body = raw_deflate(data, level) + body_pad
    xlen = 6 + len(more_extra)
    total = 12 + xlen + len(body) + 8
    bc = subfield(b"BC", struct.pack("<H", total - 1 + bsize_add))
    extra = bc + more_extra if bc_first else more_extra + bc
    return header(FEXTRA, extra=extra) + body + trailer(data, crc_xor, isize_add)


BGZF_EOF = bgzf_block(b"")
assert BGZF_EOF == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")  # the SAM specification's EOF marker


def zlib_stream(data, level=6, adler_xor=0):
    z = zlib.compress(data, level)
    return z[:-4] + struct.pack(">I", zlib.adler32(data) ^ adler_xor)


# ---------------------------------------------------------------- the judges ----
def judge_gzip(data):
    """-> (ok, bytes, in_consumed)"""
    try:
        out = gzip.decompress(data)
    except (OSError, EOFError, zlib.error):
        return False, None, 0
    return True, out, len(data)


def judge_zlib(data):
    d = zlib.decompressobj()
    try:
        out = d.decompress(data)
    except zlib.error:
        return False, None, 0
    if not d.eof:
        return False, None, 0
    return True, out, len(data) - len(d.unused_data)


def is_zlib(c):
    return c.name.startswith("zlib")


def judge(c, verify=True):
    """what the library must say of case c: ("status", status) for the SPECIAL classes, else ("judge", ok, bytes,
    in_consumed)"""
    if c.special == "reserved_flg" or (c.special == "wrong_fhcrc" and verify):
        return ("status", SPECIAL[c.special])
    data = c.clean if (c.check_only and not verify) else c.data
    return ("judge",) + (judge_zlib(data) if is_zlib(c) else judge_gzip(data))


def check(c, got, verify=True):
    """got: (bytes or None, status, in_consumed, ...) of case c, against judge(c)"""
    out, status, used = got[:3]
    want = judge(c, verify)
    if want[0] == "status":
        assert status == want[1] and out is None and used == 0, (c.name, got[1:])
        return
    _, ok, data, consumed = want
    assert (status == OK) == ok, (c.name, status, ok)
    if ok:
        assert out == data and used == consumed, (c.name, len(out), len(data), used, consumed)
    else:
        assert out is None and used == 0, c.name


# ---------------------------------------------------------------- the cases ----
def header_cases():
    """the header matrix of tests/test_gz_cpu.py: every case is one member over the same payload"""
    p = payload("hdr", 700)
    out = []
    for flg in range(32):
        out.append(case("flg_%02d" % flg, member(p, flg=flg, extra=subfield(b"ab", b"xyz"), name=b"file.txt", comment=b"a comment"), len(p)))
    out.append(case("fextra_len0", member(p, flg=FEXTRA, extra=b""), len(p)))
    few = [subfield(b"Ap", b"\1\2\3"), subfield(b"zz", b""), subfield(b"cp", b"\0" * 9)]
    bc = subfield(b"BC", b"\x34\x12")  # (a BSIZE that leads nowhere: the file is ordinary gzip)
    out.append(case("fextra_bc_first", member(p, flg=FEXTRA, extra=bc + b"".join(few)), len(p)))
    out.append(case("fextra_bc_last", member(p, flg=FEXTRA, extra=b"".join(few) + bc), len(p)))
    out.append(case("fextra_bc_absent", member(p, flg=FEXTRA, extra=b"".join(few)), len(p)))
    out.append(case("fextra_bc_wrong_length", member(p, flg=FEXTRA, extra=subfield(b"BC", b"\1\2\3") + few[0]), len(p)))
    out.append(case("fextra_subfield_leaves_xlen", member(p, flg=FEXTRA, extra=b"Ap\x40\x00ab"), len(p)))
    return out


def member_cases():
    """members of a file, BGZF, defects: shared by the CPU and the GPU test"""
    a, b, c = payload("m1", 3000), payload("m2", 1777), payload("m3", 4099)
    out = [case("one_member", member(a), len(a)),
           case("two_members", member(a) + member(b, level=1), len(a) + len(b)),
           case("three_members", member(a, level=9) + member(b, level=0) + member(c, flg=FNAME, name=b"c"), len(a) + len(b) + len(c)),
           case("empty_member", member(b""), 0),
           case("empty_member_between", member(a) + member(b"") + member(b), len(a) + len(b)),
           case("zero_padding_1", member(a) + b"\0", len(a)),
           case("zero_padding_7", member(a) + b"\0" * 7, len(a)),
           case("zeros_then_a_member", member(a) + b"\0" * 3 + member(b), len(a) + len(b)),
           case("junk_behind_member", member(a) + b"junk", len(a)),
           case("cut_second_member", member(a) + member(b)[:40], len(a) + len(b)),
           case("cut_second_header", member(a) + member(b)[:5], len(a) + len(b)),
           case("second_member_bad_data", member(a) + header() + b"\x07" + trailer(b""), len(a) + 10),
           case("wrong_fhcrc", header(FHCRC, hcrc=0x1234) + raw_deflate(a) + trailer(a), len(a), special="wrong_fhcrc"),
           case("wrong_fhcrc_second_member", member(b) + header(FHCRC | FNAME, name=b"n", hcrc=1) + raw_deflate(a) + trailer(a), len(a) + len(b),
                special="wrong_fhcrc"),
           case("reserved_flg_bit5", member(a, flg=0x20), len(a), special="reserved_flg"),
           case("reserved_flg_bit7", member(a, flg=0x80 | FNAME, name=b"x"), len(a), special="reserved_flg"),
           case("method_7", member(a, cm=7), len(a)),
           case("wrong_magic", b"\x1f\x8c" + member(a)[2:], len(a))]
    clean = member(a)
    out += [case("flipped_crc", clean[:-8] + bytes([clean[-8] ^ 1]) + clean[-7:], len(a), check_only=True, clean=clean),
            case("flipped_crc_first_of_two", clean[:-8] + bytes([clean[-8] ^ 0x80]) + clean[-7:] + member(b), len(a) + len(b), check_only=True,
                 clean=clean + member(b)),
            case("flipped_isize", clean[:-4] + bytes([clean[-4] ^ 1]) + clean[-3:], len(a))]
    # BGZF
    blocks = [payload("b%d" % k, n) for k, n in enumerate((1500, 1, 4000, 65280, 333))]
    sound = b"".join(bgzf_block(x, level=(6, 1, 9, 6, 0)[k]) for k, x in enumerate(blocks))
    total = sum(len(x) for x in blocks)
    out += [case("bgzf_5_blocks_eof", sound + BGZF_EOF, total),
            case("bgzf_no_eof", sound, total),
            case("bgzf_eof_then_zeros", sound + BGZF_EOF + b"\0" * 5, total),
            case("bgzf_bc_last_of_three", bgzf_block(blocks[0], more_extra=subfield(b"xy", b"12") + subfield(b"q\0", b""), bc_first=False) + BGZF_EOF, 1500),
            # (three blocks: as ordinary gzip it is a file of three members, the most any file here has)
            case("bgzf_chain_overshoots_by_one", bgzf_block(blocks[0]) + bgzf_block(blocks[1], level=1) + bgzf_block(blocks[4], level=0, bsize_add=1),
                 1500 + 1 + 333),
            case("bgzf_isize_plus_1", bgzf_block(blocks[0]) + bgzf_block(blocks[2], isize_add=1) + BGZF_EOF, 5501),
            case("bgzf_isize_minus_1", bgzf_block(blocks[0]) + bgzf_block(blocks[2], isize_add=-1) + BGZF_EOF, 5500),
            case("bgzf_body_ends_one_early", bgzf_block(blocks[0]) + bgzf_block(blocks[2], body_pad=b"\0") + BGZF_EOF, 5500),
            case("bgzf_flipped_crc", bgzf_block(blocks[0]) + bgzf_block(blocks[2], crc_xor=4) + BGZF_EOF, 5500, check_only=True,
                 clean=bgzf_block(blocks[0]) + bgzf_block(blocks[2]) + BGZF_EOF),
            case("bgzf_bad_data_in_block", bgzf_block(blocks[0]) + header(FEXTRA, extra=subfield(b"BC", struct.pack("<H", 26))) + b"\x07" + trailer(b"")
                 + BGZF_EOF, 1500)]
    # zlib
    z = zlib_stream(a)
    out += [case("zlib_one", z, len(a)),
            case("zlib_level0", zlib_stream(b, 0), len(b)),
            case("zlib_empty", zlib_stream(b""), 0),
            case("zlib_input_behind_trailer", z + b"more bytes", len(a)),
            case("zlib_flipped_adler", zlib_stream(a, adler_xor=1 << 20), len(a), check_only=True, clean=z),
            case("zlib_cut_trailer", z[:-2], len(a)),
            case("zlib_cut_body", z[:len(z) // 2], len(a)),
            case("zlib_fdict", bytes([0x78, 0xBB]) + z[2:], len(a)),
            case("zlib_bad_header_check", bytes([0x78, 0x9D]) + z[2:], len(a))]
    names = [x.name for x in out]
    assert len(set(names)) == len(names)
    return out


def bulk_cases():
    """the GPU test's crowd: 64 small .gz files, 64 zlib streams, one BGZF file of 200 small blocks and three of 65 280
    bytes, one ordinary file of three members"""
    r = random.Random("gz-bulk")
    out = []
    for k in range(64):
        p = payload("gzs%d" % k, r.randrange(1024, 8193))
        out.append(case("small_gz_%02d" % k, member(p, level=(0, 1, 6, 9)[k % 4], flg=FNAME if k % 3 == 0 else 0, name=b"f%d" % k), len(p)))
    for k in range(64):
        p = payload("zs%d" % k, r.randrange(1024, 8193))
        out.append(case("zlib_small_%02d" % k, zlib_stream(p, (0, 1, 6, 9)[k % 4]), len(p)))
    blocks = [payload("bb%d" % k, r.randrange(1024, 4097)) for k in range(200)] + [payload("big%d" % k, 65280) for k in range(3)]
    r.shuffle(blocks)
    out.append(case("bgzf_203_blocks", b"".join(bgzf_block(x, level=(1, 6)[k % 2]) for k, x in enumerate(blocks)) + BGZF_EOF, sum(map(len, blocks))))
    three = [payload("t%d" % k, n) for k, n in enumerate((5000, 70000, 123))]
    out.append(case("ordinary_three_members", b"".join(member(x) for x in three), sum(map(len, three))))
    return out
