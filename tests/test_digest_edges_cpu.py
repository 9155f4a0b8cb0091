"""CPU: the crafted ranges of tests/digest_edges.py, without a GPU.  Every case goes through the g++ lane schemes as the
kernels compose them (tests/c/check_dev_selftest.cpp --list: seg_lane, lane_finish, seg_finish, fold_thread, range_finish;
tests/c/sha256_dev_selftest.cpp --list: lane_digest, digest_word) and must give what zlib, liblzma and hashlib give over
the plain bytes -- and every case BITES: from the module's restated geometry, the pads, row counts, straddling lanes, fold
trips and padding corners it is named for all occur.  The totals are asserted so that an edit cannot quietly thin the
cases.  The file takes about 45 s: 9 s for the table CRC64 over the 64 MiB stream, 11 s for the judges (liblzma's CRC64 over the
24 long ranges) beside the g++ programs, the rest for the probes of 167 000 cases."""
import collections
import os
import random
import re
import subprocess
import time

import pytest

import check_ref
import digest_edges as E
import lzma_amd
from digest_edges import CRC32, CRC64, SHA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lzma_amd", "csrc")
TAIL_PAD = 1024   # a batch's arena carries as much behind its last stream


def test_constants_are_the_headers():
    chk = open(os.path.join(CSRC, "xlz_check_dev.h")).read()
    sha = open(os.path.join(CSRC, "xlz_sha256_dev.h")).read()
    host = open(os.path.join(CSRC, "xlz_host.hip")).read()

    def const(src, name):
        return re.search(r"constexpr \w+ %s = ([^;]+);" % name, src).group(1).strip()

    assert (const(chk, "kLanes"), const(chk, "kLaneBytes"), const(chk, "kRowBytes")) == ("64", "16", "kLanes * kLaneBytes")
    assert (const(chk, "kSegRows"), const(chk, "kSegBytes")) == ("128", "kSegRows * kRowBytes")
    assert (const(chk, "kBaseAlign"), const(chk, "kFoldThreads")) == ("128", "256")
    assert (E.LANE, E.ROW, E.SEG, E.BASE, E.FOLD) == (16, 64 * 16, 128 * 64 * 16, 128, 256)
    assert (const(sha, "kLanes"), const(sha, "kSimds"), const(sha, "kWavesPerSimd")) == ("64", "1024", "2")
    assert const(sha, "kRoundLanes") == "kLanes * kSimds * kWavesPerSimd" and E.ROUND == 64 * 1024 * 2
    assert int(const(host, "kArenaAlign")) == E.ARENA_ALIGN and E.ARENA_ALIGN % E.BASE == 0
    assert (CRC32, CRC64, SHA) == (lzma_amd.CHECK_CRC32, lzma_amd.CHECK_CRC64, lzma_amd.CHECK_SHA256)


def test_streams():
    grid, long = E.stream("grid"), E.stream("long")
    assert len(grid) == 4 * E.SEG + 4096 and len(long) == (2 * E.FOLD + 3) * E.SEG + 4096
    assert long[:E.PERIOD] == long[E.PERIOD:2 * E.PERIOD] and long[-E.PERIOD:] == long[-2 * E.PERIOD:-E.PERIOD]
    assert all(E.PERIOD % p for p in range(2, 256)) and len(set(long[:E.PERIOD])) == 256
    segs = {long[o:o + 64] for o in range(0, len(long) - 64, E.SEG)}   # no two segments begin alike
    assert len(segs) == len(range(0, len(long) - 64, E.SEG))
    import lzma
    raw = E.raw_lzma2(grid)
    assert lzma.decompress(raw, format=lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA2, "dict_size": 1 << 16}]) == grid
    units = lzma_amd.lzma2_units(E.raw_lzma2(long[:(3 << 20) + 5]))
    assert sum(u["out_len"] for u in units) == (3 << 20) + 5 and max(u["out_len"] for u in units) <= 1 << 20 and len(units) >= 4


def test_table_crc64_is_liblzmas():
    """the byte-wise table CRC64 that judges the ranges of "grid": liblzma's on 24 buffers, the whole of "long" among them"""
    t0 = time.time()
    rnd = random.Random(8300)
    bufs = [rnd.randbytes(n) for n in (0, 1, 2, 7, 8, 9, 15, 16, 17, 255, 256, 257, 1023, 1024, 4097, 65521, 100_000, 300_001)]
    bufs += [b"\x00" * 1000, b"\xff" * 1001, b"123456789", E.stream("grid"), E.stream("long")[:E.SEG + 1], E.stream("long")]
    assert len(bufs) >= 20
    for b in bufs:
        assert E.crc64_at(b, 0, [len(b)])[len(b)] == check_ref.crc64(b), len(b)
    assert E.crc64_at(b"123456789", 0, [9])[9] == 0x995DC9BBDF1939FA
    # one walk, many lengths, a start that is not 0
    g = E.stream("grid")
    got = E.crc64_at(g, 1145, [0, 1, 300, 5000])
    assert got == {n: check_ref.crc64(g[1145:1145 + n]) for n in (0, 1, 300, 5000)}
    print("test_table_crc64_is_liblzmas: %.1f s" % (time.time() - t0))


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("digest_edges")
    exes = {}
    for name, extra in (("check_dev_selftest", []), ("sha256_dev_selftest", ["-pthread"])):
        exes[name] = str(d / name)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror"] + extra + ["-I", CSRC,
                               os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exes[name]])
    arenas = {}
    for s in E.STREAMS:
        arenas[s] = str(d / (s + ".bin"))
        with open(arenas[s], "wb") as f:
            f.write(E.stream(s) + b"\xa5" * TAIL_PAD)
    return d, exes, arenas


def _cpu_cases():
    """every case but the middle of sha/rounds: 4096 of its ranges, from both launches"""
    rounds = E.cases("sha/rounds")
    keep = set(c.name for c in rounds[:2048] + rounds[-2048:])
    return [c for c in E.cases() if E.family(c) != "sha/rounds" or c.name in keep]


def test_lane_schemes_equal_the_judges(programs):
    """one run of a g++ program per stream and kind, all at once; ranges that several cases share run once"""
    d, exes, arenas = programs
    t0 = time.time()
    cs = _cpu_cases()
    jobs = collections.OrderedDict()   # (stream, kind) -> {(lo, n): slot}
    for c in cs:
        lo, hi = E.clip(c)
        jobs.setdefault((c.stream, c.kind), collections.OrderedDict()).setdefault((lo, hi - lo), None)
    running = []
    for (s, kind), ranges in jobs.items():
        stem = str(d / ("%s_%d" % (s, kind)))
        with open(stem + ".txt", "w") as f:
            for lo, n in ranges:
                f.write("%d %d %d\n" % (kind, lo, n))
        exe = exes["sha256_dev_selftest" if kind == SHA else "check_dev_selftest"]
        running.append((s, kind, stem, subprocess.Popen([exe, "--list", stem + ".txt", arenas[s], stem + ".out"])))
    want = E.expected(cs)   # (the judges work while the programs run)
    t1 = time.time()
    got = {}
    for s, kind, stem, p in running:
        assert p.wait(timeout=600) == 0, (s, kind)
        size = 32 if kind == SHA else 8
        blob = open(stem + ".out", "rb").read()
        assert len(blob) == size * len(jobs[s, kind]), (s, kind)
        for k, key in enumerate(jobs[s, kind]):
            v = blob[size * k:size * (k + 1)]
            got[(s, kind) + key] = v if kind == SHA else int.from_bytes(v, "little")
    print("test_lane_schemes_equal_the_judges: %d cases, %d runs of the scheme, judges %.1f s, all %.1f s"
          % (len(cs), len(got), t1 - t0, time.time() - t0))
    for c, w in zip(cs, want):
        lo, hi = E.clip(c)
        g = got[c.stream, c.kind, lo, hi - lo]
        assert g == w, (c, E.probes(c), g, w)
    # a digest written to the wrong index shows: the ranges of sha/rounds all differ, but for some of those of one to three
    # bytes (there are only 256 messages of one byte)
    rounds = [d for c, d in zip(E.cases("sha/rounds"), E.expected(E.cases("sha/rounds"))) if c.len >= 4]
    assert len(set(rounds)) == len(rounds) >= (E.ROUND + 65) * 187 // 191


def test_every_case_bites():
    seen = collections.defaultdict(set)
    for c in E.cases("crc"):
        p = E.probes(c)
        lo, hi = E.clip(c)
        assert lo % E.BASE == c.off % E.BASE or hi == lo   # (what a stream's place in the arena keeps)
        if not p["m"]:
            assert hi == lo
            seen[c.kind, "empty"].add(E.family(c))
            continue
        assert 1 <= p["rows"] <= 128 and 0 <= p["pad"] < E.ROW and (p["m"] - 1) * E.SEG < hi - E.range_base(lo) <= p["m"] * E.SEG
        assert (hi - E.range_base(lo) - (p["m"] - 1) * E.SEG + p["pad"]) == p["rows"] * E.ROW
        fam = E.family(c)
        seen[c.kind, "pad"].add(p["pad"])
        seen[c.kind, "m"].add(p["m"])
        seen[c.kind, "rows%4", p["rows"] >= 4].add(p["rows"] % 4)
        seen[c.kind, "start"].add((p["start_arm"], p["start_lane"]))
        seen[c.kind, "end"].add((p["end_arm"], p["end_lane"]))
        seen[c.kind, "trips"].add(tuple(p["fold_trips"]))
        if fam == "crc/rows":
            seen[c.kind, "rows/rows"].add(p["rows"])
            seen[c.kind, "rows/end"].add((hi - E.range_base(lo)) % E.ROW)
        if fam == "crc/fold":
            seen[c.kind, "fold/m-2"].add(p["m"] - 2)
            seen[c.kind, "fold/last", p["m"], c.off].add((p["rows"], p["pad"]))
        if fam == "crc/segments":
            seen[c.kind, "segments"].add((p["m"], p["rows"], p["pad"]))
            if "no-straddle" in c.name:
                assert (p["start_arm"], p["end_arm"], p["pad"], lo % E.BASE) == ("vector", "vector", 0, 0), c
            if "one-byte-at-127" in c.name:
                assert (lo % E.BASE, hi - lo, p["start_lane"], p["start_arm"]) == (127, 1, 7, "bytes"), c
    for kind in E.KINDS:
        assert seen[kind, "pad"] >= {0, 1, 15, 16, 17, 1023}
        assert seen[kind, "rows%4", False] == {1, 2, 3} and seen[kind, "rows%4", True] == {0, 1, 2, 3}
        assert seen[kind, "rows/rows"] >= set(range(1, 10))
        assert seen[kind, "rows/end"] >= {0, 1, 15, 16, 17, E.ROW - 1}
        assert seen[kind, "m"] >= {1, 2, 3, 4, 5} | set(E.FOLD_SEGS)
        assert seen[kind, "fold/m-2"] == {0, 1, 255, 256, 257, 511, 512, 513}
        for m in E.FOLD_SEGS:   # a one-byte and a full last segment, at both starts
            for off in (0, 3):
                assert seen[kind, "fold/last", m, off] == {(1, 1023), (128, 0)}, (m, off)
        # the fold's threads: none busy, some, all; one trip, one and two, two, two and three
        assert seen[kind, "trips"] >= {(0,), (0, 1), (1,), (1, 2), (2,), (2, 3)}
        # both arms of load_chunk at both ends, the byte-wise one in every lane of a 128-byte line at the start and in
        # every lane of a row at the end
        for end in ("start", "end"):
            assert {arm for arm, _ in seen[kind, end]} == {"vector", "bytes"}
        assert {lane for arm, lane in seen[kind, "start"] if arm == "bytes"} >= set(range(8))
        assert {lane for arm, lane in seen[kind, "end"] if arm == "bytes"} == set(range(64))
        assert {lane for arm, lane in seen[kind, "start"] if arm == "vector"} >= set(range(8))
        for m in (1, 2, 3, 4):   # ends with its segment; one byte into the last one
            assert (m, 128, 0) in seen[kind, "segments"] and (m, 1, 1023) in seen[kind, "segments"] and (m, 128, 1) in seen[kind, "segments"]
        assert seen[kind, "empty"] == {"crc/short", "crc/overlap"}
    corners = set()
    for c in E.cases("sha"):
        p = E.probes(c)
        lo, hi = E.clip(c)
        assert (p["s"], 64 * p["n_full"] + p["r"]) == (c.off & 3, hi - lo) and hi - lo == c.len
        fam = E.family(c)
        corners.add((fam, p["s"], p["r"], min(p["n_full"], 2)))
        if fam == "sha/blocks":
            corners.add((fam, p["s"], p["r"], "b%d" % p["n_full"]))
    for s in range(4):
        for r in range(64):   # every shift times every tail, with no, one and more full blocks in front
            for nf in (0, 1, 2):
                assert ("sha/grid", s, r, nf) in corners, (s, r, nf)
        for r in E.SHA_TAILS:
            for b in E.SHA_BLOCKS:
                assert ("sha/blocks", s, r, "b%d" % b) in corners, (s, r, b)
    assert {0, 55, 56, 63} <= set(range(64)) and {54, 55, 56, 57, 62, 63, 0, 1} == set(E.SHA_TAILS)
    for n in E.WAVE_SETS:   # n ranges for the device, every one another number of blocks
        ws = E.wave_set(n)
        assert [c.len for c in ws][:2] == [0, 101] and len(ws) == n + 1 and all(c in E.cases("sha/wave") for c in ws)
        assert sorted(c.len // 64 for c in ws if c.len) == list(range(1, n + 1))
        assert max(c.off + c.len for c in ws) <= E.GRID_BYTES
    rounds = E.cases("sha/rounds")
    assert [(c.off, c.len) for c in rounds] == [(67 * k, 1 + k % 191) for k in range(E.ROUND + 65)]
    assert rounds[-1].off + rounds[-1].len <= E.LONG_BYTES


COUNTS = {"crc/short": 2 * 32 * 301, "crc/rows": 2 * 16 * (21 + 9 * 9 - 4), "crc/segments": 2 * 147, "crc/fold": 2 * 32, "crc/overlap": 2 * 42,
          "sha/grid": 64 * 201, "sha/blocks": 160, "sha/wave": 65 + 66 + 2 + 64, "sha/rounds": 131072 + 65}


def test_totals():
    cs = E.cases()
    count = collections.Counter(E.family(c) for c in cs)
    assert dict(count) == COUNTS, dict(count)
    assert len({c.name for c in cs}) == len(cs)
    for kind in E.KINDS:   # every CRC case under both kinds
        assert sum(c.kind == kind for c in cs) == sum(v for k, v in COUNTS.items() if k.startswith("crc/")) // 2
    big = collections.Counter()
    for c in E.cases("crc"):
        lo, hi = E.clip(c)
        if hi - lo >= 30 << 20:
            big[c.kind, lo, hi] += 1
    for kind in E.KINDS:   # what the judges pay for
        assert sum(1 for k in big if k[0] == kind) == 24 and sum(v for k, v in big.items() if k[0] == kind) == 24 + 2 * E.COPIES


def test_one_launch_order():
    """the checks call of the GPU test: every CRC case once; in either kind's table no two ranges of several segments are
    neighbours; enough segments that on 256 CUs every wave of either segment kernel's grid makes three trips and more"""
    order = E.one_launch_order()
    assert sorted(order) == sorted(E.cases("crc")) and order != E.cases("crc")
    assert order[-len(E.cases("crc/overlap")):] == E.cases("crc/overlap")
    for kind, per_cu in ((CRC32, 8), (CRC64, 4)):
        tab = E.table_of(order, kind)
        n_many = sum(m > 1 for m in tab)
        assert n_many >= 200 and tab[0] == tab[-1] == 1 and E.changes(tab) == 2 * n_many
        assert sum(tab) >= 3 * 4 * per_cu * 256, sum(tab)
        print("kind %d: %d ranges in the table, %d of several segments, %d segments" % (kind, len(tab), n_many, sum(tab)))
    offs = [(E.STREAMS.index(c.stream), c.off) for c in E.cases("crc/overlap") if c.kind == CRC32 and E.probes(c)["m"]]
    assert offs == sorted(offs, reverse=True) and len(set(offs)) < len(offs)


def test_sha_sets_are_the_devices(xlz_so):
    """the host-only plan: all of sha/rounds go to the device, and every wave set next to its ballast"""
    lens = [c.len for c in E.cases("sha/rounds")]
    assert lzma_amd.sha256_plan(lens) == [True] * (E.ROUND + 65)
    assert E.clip(E.BALLAST) == (0, E.BALLAST.len)
    for n in E.WAVE_SETS:
        lens = [c.len for c in E.wave_set(n) if c.len]
        assert len(lens) == n and lzma_amd.sha256_plan(lens + [E.BALLAST.len]) == [True] * n + [False]
        assert lzma_amd.sha256_plan(lens + [E.BALLAST.len] * 2) == [True] * n + [False] * 2
