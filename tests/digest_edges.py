"""Crafted ranges for the device digest kernels (lzma_amd/csrc/xlz_check_dev.hip, xlz_sha256_dev.hip): ranges that sit ON
the seams of their work split -- the 16-byte lane chunk, the 1 KiB row and the four-row unrolled loop, the 128-byte base
line, the 128 KiB segment, the 256 threads of the fold and its Horner loop; for SHA-256 the start's byte shift times every
corner of the padding, the lanes of one wave, and a second launch.  The judges are zlib (CRC32), liblzma (CRC64, through
tests/check_ref.py) and hashlib (SHA-256) over the plain bytes; tests/test_digest_edges_cpu.py shows that every case sits
where its name says and runs the lane schemes on the CPU, tests/test_gpu_digest_edges.py runs the kernels.  A plain
module, not a conftest.

cases() -> [Case(name, stream, off, len, kind)]: stream = "grid" or "long" (stream(name) -> its bytes), off / len as a
caller passes them (a range behind its stream's end is the digest of nothing), kind = CRC32 / CRC64 / SHA.  A case's
family is the first two parts of its name.  probes(case) -> the geometry the name claims, from a restatement of
range_base / range_segments / seg_geom written from the comments of xlz_check_dev.h (not from the library):
  CRC:  "m" segments, "rows" and "pad" of the last one, "start_lane" / "end_lane": the lane whose chunk holds the range's
        first / last byte, "start_arm" / "end_arm": "vector" when that chunk lies wholly inside the range (one 16-byte load),
        "bytes" when it straddles the end (load_chunk's byte-wise arm), "fold_trips": the Horner trips the fold's threads make
  SHA:  "s" = off & 3, "n_full" blocks, "r" bytes behind them
Everything is seeded."""
import collections
import functools
import hashlib
import random
import zlib

import check_ref
from check_ref import CRC32, CRC64

SHA = 10
KINDS = (CRC32, CRC64)
TAG = {CRC32: "crc32", CRC64: "crc64", SHA: "sha"}

# restated from lzma_amd/csrc/xlz_check_dev.h and xlz_sha256_dev.h (tests/test_digest_edges_cpu.py holds them to the headers)
LANE, ROW, SEG, BASE, FOLD = 16, 1024, 128 << 10, 128, 256
ROUND = 131072                    # xlzsha::kRoundLanes = 64 lanes x 1024 SIMDs x 2 waves: the ranges of one SHA-256 launch
ARENA_ALIGN = 256                 # streams start at multiples of it in the output arena: offsets keep their value mod 128
PERIOD = 65521                    # the prime period of "long"

GRID_BYTES = 4 * SEG + 4096
LONG_BYTES = (2 * FOLD + 3) * SEG + 4096
STREAMS = ("grid", "long")        # in this order in the batch

Case = collections.namedtuple("Case", "name stream off len kind")


@functools.lru_cache(None)
def stream(name):
    if name == "grid":
        return random.Random(8101).randbytes(GRID_BYTES)
    block = random.Random(8102).randbytes(PERIOD)   # no two segments of "long" hold the same bytes: the period is prime
    return (block * (LONG_BYTES // PERIOD + 1))[:LONG_BYTES]


def raw_lzma2(data):
    """`data` as a raw LZMA2 stream of stored chunks, a dictionary reset every 1 MiB: independent units"""
    import lzma_craft
    parts = [lzma_craft.lzma2_stored(data[o:o + 65536], o % (1 << 20) == 0) for o in range(0, len(data), 65536)]
    return b"".join(parts) + b"\x00"


# ---- the geometry, restated --------------------------------------------------------------------------------------------
def range_base(off):
    return off - off % BASE


def range_segments(off, n):
    return -(-(off + n - range_base(off)) // SEG) if n else 0


def seg_geom(off, n, s):
    """(base, rows, pad) of segment s of the range"""
    base = range_base(off) + s * SEG
    rem = off + n - base
    if rem >= SEG:
        return base, SEG // ROW, 0
    rows = -(-rem // ROW)
    return base, rows, rows * ROW - rem


def clip(case):
    n = len(stream(case.stream))
    return min(case.off, n), min(case.off + case.len, n)


def probes(case):
    lo, hi = clip(case)
    n = hi - lo
    if case.kind == SHA:
        return {"s": lo & 3, "n_full": n >> 6, "r": n & 63}
    if not n:
        return {"m": 0}
    m = range_segments(lo, n)
    _, rows, pad = seg_geom(lo, n, m - 1)
    base = range_base(lo)
    first, last = lo - lo % LANE, (hi - 1) - (hi - 1) % LANE
    trips = sorted({(m - 2 - t) // FOLD + 1 if m >= 2 and t <= m - 2 else 0 for t in range(FOLD)})
    return {"m": m, "rows": rows, "pad": pad,
            "start_lane": (first - base) % ROW // LANE, "end_lane": (last - base) % ROW // LANE,
            "start_arm": "vector" if first >= lo and first + LANE <= hi else "bytes",
            "end_arm": "vector" if last >= lo and last + LANE <= hi else "bytes",
            "fold_trips": trips}


def family(case):
    return "/".join(case.name.split("/")[:2])


# ---- CRC ---------------------------------------------------------------------------------------------------------------------
def _crc(out, fam, what, strm, off, n):
    for kind in KINDS:
        out.append(Case("crc/%s/%s/%s" % (fam, TAG[kind], what), strm, off, n, kind))


ROW_ENDS = (0, 1, 15, 16, 17, ROW - 17, ROW - 16, ROW - 15, ROW - 1)   # (off + len - base) % ROW: pads 0, 1023 ... 17, 16, 15, 1
SELFTEST_LENS = (ROW - 17, ROW - 16, ROW - 1, ROW, ROW + 1, ROW + 16, 2 * ROW, 4 * ROW + 3, 5 * ROW, SEG - ROW, SEG - 129, SEG - 128,
                 SEG - 1, SEG, SEG + 1, SEG + 127, SEG + 128, 2 * SEG - 1, 2 * SEG, 2 * SEG + 1, 3 * SEG + 777)
FOLD_SEGS = (2, 3, FOLD + 1, FOLD + 2, FOLD + 3, 2 * FOLD + 1, 2 * FOLD + 2, 2 * FOLD + 3)
SEGMENT_STARTS = (256, 256 + 5, 256 + 127, 1024 + 112 + 9)
COPIES = 6                        # of each of the two longest fold ranges in crc/overlap


def _crc_cases(out):
    for lead in (256, 1024 + 112):           # (the second: the last chunk of a 128-byte line)
        for a in range(16):
            for n in range(301):
                _crc(out, "short", "off%d/len%d" % (lead + a, n), "grid", lead + a, n)
    for a in range(16):
        off = 1024 + 112 + a
        d = off - range_base(off)
        lens = set(SELFTEST_LENS)
        for rows in range(1, 10):
            for e in ROW_ENDS:
                total = rows * ROW if e == 0 else (rows - 1) * ROW + e   # = off + len - base
                if total - d >= 1:
                    lens.add(total - d)
        for n in sorted(lens):
            _crc(out, "rows", "off%d/len%d" % (off, n), "grid", off, n)
    for m in (1, 2, 3, 4):
        for off in SEGMENT_STARTS:
            d = off - range_base(off)
            # ends with its last segment; one byte into it (rows 1, pad 1023); one byte short of its end; somewhere inside
            for tag, total in (("full", m * SEG), ("one-byte", (m - 1) * SEG + 1), ("short", m * SEG - 1), ("inside", (m - 1) * SEG + 54321)):
                if total - d >= 1:
                    _crc(out, "segments", "m%d/off%d/%s" % (m, off, tag), "grid", off, total - d)
    _crc(out, "segments", "one-byte-at-127", "grid", 256 + 127, 1)
    for lane in range(8):                    # the start in every chunk of its 128-byte line, on the chunk's edge and inside it
        _crc(out, "segments", "start-lane%d/vector" % lane, "grid", 256 + LANE * lane, 2000)
        _crc(out, "segments", "start-lane%d/bytes" % lane, "grid", 256 + LANE * lane + 5, 2000)
    for lane in range(64):                   # the end inside every chunk of a row
        _crc(out, "segments", "end-lane%d" % lane, "grid", 1024 + 128, 2 * ROW + LANE * lane + 7)
    for rows in (1, 3, 128, 133, 4 * 128):   # from a 128-byte line to a row's end: no lane straddles anything
        _crc(out, "segments", "no-straddle/rows%d" % rows, "grid", 1024 + 128, rows * ROW)
    for m in FOLD_SEGS:
        for off in (0, 3):
            _crc(out, "fold", "m%d/off%d/one-byte" % (m, off), "long", off, (m - 1) * SEG + 1 - off)
            _crc(out, "fold", "m%d/off%d/full" % (m, off), "long", off, m * SEG - off)
    # identical, nested and overlapping ranges in descending offset order, ranges behind the output between them; every
    # second one has one segment.  The copies of the two longest fold ranges cost a judge nothing.
    k = 0

    def add(strm, off, n):
        nonlocal k
        _crc(out, "overlap", "%d" % k, strm, off, n)
        k += 1

    mmax = FOLD_SEGS[-1]
    add("long", LONG_BYTES + 1, 5)
    add("long", 1000, 1000)
    for c in range(COPIES):
        add("long", 3, mmax * SEG - 3)
        add("long", 3, 100 + c)
        if c % 2:
            add("long", LONG_BYTES + 7 * c, 1 << 40)
    for c in range(COPIES):
        add("long", 0, (mmax - 1) * SEG + 1)
        add("long", 0, 1 + c)
    for strm, off, n in (("grid", GRID_BYTES + 5, 10), ("grid", 400001, 100000), ("grid", GRID_BYTES, 1), ("grid", 300003, 200000),
                         ("grid", 300003, 1000), ("grid", 300003, 1000), ("grid", GRID_BYTES + 1, 0), ("grid", 250000, GRID_BYTES - 250000),
                         ("grid", 250000, 77), ("grid", 100, 500000), ("grid", 100, 130000), ("grid", 0, GRID_BYTES + 100), ("grid", 0, 1)):
        add(strm, off, n)


# ---- SHA-256 -------------------------------------------------------------------------------------------------------------------
SHA_BLOCKS = (1, 2, 3, 37, 1000)
SHA_TAILS = (0, 1, 54, 55, 56, 57, 62, 63)
WAVE_SETS = (64, 65, 1, 63)       # ranges the DEVICE gets in a set
BALLAST = Case("sha/ballast", "long", 0, 8 << 20, SHA)   # a range for the host's threads, see wave_set


def _sha_cases(out):
    for s in range(64):
        for n in range(201):
            out.append(Case("sha/grid/off%d/len%d" % (512 + s, n), "grid", 512 + s, n, SHA))
    at = 4096
    for blocks in SHA_BLOCKS:
        for r in SHA_TAILS:
            for s in range(4):
                out.append(Case("sha/blocks/b%d/r%d/s%d" % (blocks, r, s), "grid", at + s, 64 * blocks + r, SHA))
                at += 68
    for n in WAVE_SETS:
        out.extend(wave_set(n))
    for k in range(ROUND + 65):
        out.append(Case("sha/rounds/%d" % k, "long", 67 * k, 1 + k % 191, SHA))


def wave_set(n):
    """The ranges of one digests call whose device part is ONE launch of n lanes: len = 64 k + (k * 37 % 64), every lane of
    a wave another block count.  k = 0 is a range of no bytes, which never reaches the device; so k runs from 0 to n, and n
    ranges are the device's.  (The plan leaves few short ranges to the host's threads: a call adds BALLAST, a range long
    enough that the host is busy with it for longer than the longest lane.)"""
    return [Case("sha/wave/%d/%d" % (n, k), "grid", 1000 + 131 * k, 64 * k + k * 37 % 64, SHA) for k in range(n + 1)]


@functools.lru_cache(None)
def _all():
    out = []
    _crc_cases(out)
    _sha_cases(out)
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def cases(fam=None):
    return [c for c in _all() if fam is None or family(c) == fam or family(c).split("/")[0] == fam]


# ---- one launch of every CRC case ------------------------------------------------------------------------------------------
def one_launch_order(seed=8200):
    """every CRC case for one checks call: everything but crc/overlap in seeded shuffled order, dealt so that in the table
    of either kind (a call's non-empty ranges of that kind, in call order) no two ranges of several segments are
    neighbours and the table begins and ends with a range of one segment; then crc/overlap as it is listed"""
    rnd = random.Random(seed)
    per_kind, empty = [], []
    for kind in KINDS:
        cs = [c for c in cases("crc") if c.kind == kind and family(c) != "crc/overlap"]
        rnd.shuffle(cs)
        empty += [c for c in cs if probes(c)["m"] == 0]
        one = [c for c in cs if probes(c)["m"] == 1]
        many = [c for c in cs if probes(c)["m"] > 1]
        assert len(one) > len(many) + 1
        seq, at = [], 0
        for j, c in enumerate(many):   # the j-th long range goes behind an even share of the short ones (at least one)
            upto = (j + 1) * (len(one) - 1) // len(many)
            seq += one[at:upto] + [c]
            at = upto
        per_kind.append(seq + one[at:])
    order, idx = [], [0, 0]
    while idx[0] < len(per_kind[0]) or idx[1] < len(per_kind[1]):   # the two kinds shuffled into each other
        left = [len(per_kind[k]) - idx[k] for k in (0, 1)]
        k = 0 if rnd.randrange(left[0] + left[1]) < left[0] else 1
        order.append(per_kind[k][idx[k]])
        idx[k] += 1
    for c in empty:
        order.insert(rnd.randrange(len(order) + 1), c)
    return order + cases("crc/overlap")


def table_of(order, kind):
    """the segment counts of a call's table of one kind"""
    return [probes(c)["m"] for c in order if c.kind == kind and probes(c)["m"]]


def changes(table):
    """how often a table goes from a range of one segment to one of several or back"""
    return sum((a == 1) != (b == 1) for a, b in zip(table, table[1:]))


# ---- the judges --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _crc64_table():
    tab = []
    for v in range(256):
        for _ in range(8):
            v = (v >> 1) ^ (0xC96C5795D7870F42 if v & 1 else 0)
        tab.append(v)
    return tab


def crc64_at(data, off, lens):
    """a byte-wise table CRC64 (the .xz one) of data[off : off + n] for every n of lens in one walk -> {n: crc}.
    tests/test_digest_edges_cpu.py holds it to liblzma's."""
    tab, want, out = _crc64_table(), set(lens), {}
    c, ones = 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF
    if 0 in want:
        out[0] = 0
    for n, b in enumerate(memoryview(data)[off:off + max(want, default=0)], 1):
        c = tab[(c ^ b) & 0xFF] ^ (c >> 8)
        if n in want:
            out[n] = c ^ ones
    return out


_expected = {}


def expected(cs):
    """the judges' digests of the cases, in order: an int for a CRC, 32 bytes for a SHA-256.  CRC64 over "grid" is the table's
    (one walk per start), over "long" liblzma's own: its bytes repeat, which liblzma's encoder passes quickly.  Kept."""
    todo = collections.defaultdict(set)
    for c in cs:
        lo, hi = clip(c)
        if c.kind == CRC64 and c.stream == "grid" and (c.stream, lo, hi, c.kind) not in _expected:
            todo[lo].add(hi - lo)
    for lo, lens in todo.items():
        for n, d in crc64_at(stream("grid"), lo, lens).items():
            _expected["grid", lo, lo + n, CRC64] = d
    out = []
    for c in cs:
        lo, hi = clip(c)
        key = (c.stream, lo, hi, c.kind)
        if key not in _expected:
            data = memoryview(stream(c.stream))[lo:hi]
            _expected[key] = (hashlib.sha256(data).digest() if c.kind == SHA else zlib.crc32(data) if c.kind == CRC32
                              else check_ref.crc64(data))
        out.append(_expected[key])
    return out


def as_range(case):
    """the case as Batch.checks / Batch.digests take it"""
    return (STREAMS.index(case.stream), case.off, case.len, case.kind)
