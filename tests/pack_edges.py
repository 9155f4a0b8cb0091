"""Crafted tables for the pack kernel (lzma_amd/csrc/xlz_pack_dev.hip, its scheme in xlz_pack_dev.h): items that sit ON the
seams of its work split -- the 16 KiB tile of the DESTINATION, the head / 16-byte chunks / tail of the portion a tile holds
of an item, the four-chunks-per-lane loop of 256 lanes, the byte shift r = (source - destination) mod 16 -- tiles that hold
nothing, tiles that hold thousands of items, and, in rounds, more tiles than a launch has workgroups.  Tiles count from the
destination pointer rounded DOWN to 16: with a pointer that is `mis` modulo 16 a seam lies at dst_off = k * 16384 - mis.
tests/test_pack_edges_cpu.py shows that every named shape occurs and runs the tables through the g++ lane scheme;
tests/test_gpu_pack_edges.py runs them on the device.  A plain module, not a conftest.

plan(family, mis) -> (stream sizes, items as Batch.pack takes them [(stream, off, len, dst_off)], dst_cap, probe).  probe()
restates portion / head / chunks / tail from (src, dst, len) alone (portions()), asserts the shapes the family is named for
and returns what it counted.  The streams' bytes are plains(sizes): corpus.plain, a handful of 64 KiB to 200 KiB, read by
many items each.  Everything is seeded."""
import collections
import functools
import random

import numpy as np

import corpus

TILE, LANES = 16384, 256
FILL = 0xA5
MIS = (0, 5)
FAMILIES = ("seam", "chunks", "empty", "crowd")
SIZES = (65536, 70001, 100003, 131072, 204800)
SEAM_A, SEAM_B = (1, 15, 16, 17), (0, 1, 15, 16, 17)
CHUNK_COUNTS = (0, 1, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024)
ENDS = (0, 1, 15)
SHIFTS = (0, 1, 7, 8, 9, 15)
ROUND_KINDS = ("inside", "across-start", "across-end", "congruent", "r1", "r8", "r15")

Portion = collections.namedtuple("Portion", "item tile d0 d1 head chunks tail r")


@functools.lru_cache(None)
def plains(sizes=SIZES):
    return tuple(corpus.plain("M", 760 + i, n) for i, n in enumerate(sizes))


def expect_pack(items, plains, cap, ptr_mod):
    """what the pack must leave in a destination of `cap` bytes filled with FILL whose address is ptr_mod modulo 16
    -> (bytes, copied per item, statistics)"""
    want = np.full(cap, FILL, dtype=np.uint8)
    copied = []
    st = {"items": 0, "bytes": 0, "congruent_items": 0, "empty_items": 0}
    for k, off, length, dst in items:
        n = len(plains[k])
        lo, hi = min(off, n), min(off + length, n)
        copied.append(hi - lo)
        if hi == lo:
            st["empty_items"] += 1
            continue
        want[dst:dst + hi - lo] = np.frombuffer(plains[k], dtype=np.uint8)[lo:hi]
        st["items"] += 1
        st["bytes"] += hi - lo
        st["congruent_items"] += lo % 16 == (ptr_mod + dst) % 16
    return want.tobytes(), copied, st


def portions(items, mis):
    """tile_lane restated: per item and tile the portion [d0, d1) the tile holds of it, in the kernel's coordinates
    (dst = dst_off + mis; a stream's region starts at a multiple of 256, so src mod 16 = off mod 16)"""
    out = []
    for q, (_, off, length, dst_off) in enumerate(items):
        dst = dst_off + mis
        for tile in range(dst // TILE, (dst + length - 1) // TILE + 1):
            d0, d1 = max(dst, tile * TILE), min(dst + length, (tile + 1) * TILE)
            head = min(-d0 % 16, d1 - d0)
            chunks = (d1 - d0 - head) // 16
            out.append(Portion(q, tile, d0, d1, head, chunks, d1 - d0 - head - 16 * chunks, (off - dst) % 16))
    return out


def tiles_of(items, mis):
    """-> (first tile, tile count) of the launch: xlzpack::first_tile / tile_count restated"""
    lo = min(d + mis for _, _, _, d in items) // TILE
    return lo, max(d + mis + n - 1 for _, _, n, d in items) // TILE - lo + 1


class _Table:
    """items laid out in the kernel's coordinates; sources dealt from the streams in turn"""

    def __init__(self, mis, seed):
        self.mis, self.items, self.rnd, self.turn = mis, [], random.Random(seed), 0

    def add(self, kdst, length, r):
        """an item of `length` bytes at kernel offset kdst whose source is r further on modulo 16 than its destination"""
        s = self.turn % len(SIZES)
        self.turn += 1
        off = 16 * self.rnd.randrange(1, (SIZES[s] - length) // 16 - 1) + (kdst + r) % 16
        assert kdst >= self.mis and 0 < length and off + length <= SIZES[s] and (off - kdst) % 16 == r
        self.items.append((s, off, length, kdst - self.mis))

    def done(self, slack=64):
        cap = max(d + n for _, _, n, d in self.items) + slack
        ordered = sorted(self.items, key=lambda it: it[3])
        assert all(a[3] + a[2] <= b[3] for a, b in zip(ordered, ordered[1:]))
        self.rnd.shuffle(self.items)
        return cap


def _seam(mis):
    """per source residue 0..15, a in SEAM_A and b in SEAM_B an item [T - a, T + b) over a seam T of its own; b = 0 ends at the
    tile's last byte, and the next item starts exactly at T"""
    t, tile = _Table(mis, 9600), 1
    want = {}
    for a in SEAM_A:
        for b in SEAM_B:
            for s in range(16):
                T = tile * TILE
                t.add(T - a, a + b, (s - (T - a)) % 16)
                if b == 0:
                    t.add(T, 1 + (7 * s + a) % 40, (3 * s + 1) % 16)
                want[tile] = (a, b)
                tile += 2
    cap = t.done()

    def probe():
        by = collections.defaultdict(list)
        for p in portions(t.items, mis):
            by[p.tile].append(p)
        srcs = collections.defaultdict(set)
        for tile, (a, b) in want.items():
            (left,), right = by[tile - 1], by[tile]
            assert left.d1 == tile * TILE and left.d1 - left.d0 == a and len(right) == 1 and right[0].d0 == tile * TILE
            assert right[0].item == left.item if b else right[0].item != left.item
            assert b == 0 or right[0].d1 - right[0].d0 == b
            srcs[a, b].add(t.items[left.item][1] % 16)
        assert len(srcs) == 20 and all(v == set(range(16)) for v in srcs.values())
        return {"seams": len(want)}
    return SIZES, t.items, cap, probe


def chunk_shapes():
    """(chunks, head, tail) of every portion that fits a tile: 1024 chunks are a whole tile, 1023 leave room for a head or a
    tail; no bytes at all are no item"""
    out = []
    for c in CHUNK_COUNTS:
        for head in ENDS:
            for tail in ENDS:
                if (16 if head else 0) + 16 * c + tail <= TILE and head + 16 * c + tail > 0:
                    out.append((c, head, tail))
    return out


def _chunks(mis):
    t, tile = _Table(mis, 9700), 1
    shapes = chunk_shapes()
    for c, head, tail in shapes:
        for r in SHIFTS:
            n, base = head + 16 * c + tail, -head % 16          # a tile of its own, anywhere on the 16-byte grid that leaves room
            t.add(tile * TILE + base + 16 * ((37 * tile) % ((TILE - base - n) // 16 + 1)), n, r)
            tile += 1
    cap = t.done()

    def probe():
        ps = portions(t.items, mis)
        assert len(ps) == len(t.items) == len(shapes) * len(SHIFTS)      # every item inside one tile
        seen = collections.Counter((p.chunks, p.head, p.tail, p.r) for p in ps)
        assert set(seen) == {(c, h, tl, r) for c, h, tl in shapes for r in SHIFTS} and set(seen.values()) == {1}
        # the four-chunks-per-lane loop: lane l takes chunks l, l + 256, l + 512, l + 768 -- every trip count of lane 0 and
        # of lane 255, and a lane without a chunk
        trips = {(-(-c // LANES), max(0, -(-(c - 255) // LANES))) for c, _, _, _ in seen}
        assert trips == {(0, 0), (1, 0), (1, 1), (2, 1), (2, 2), (3, 2), (3, 3), (4, 3), (4, 4)}
        return {"shapes": len(shapes), "whole_tiles": sum(p.chunks == 1024 for p in ps)}
    return SIZES, t.items, cap, probe


def _empty(mis):
    t = _Table(mis, 9800)
    T = TILE
    t.add(2 * T - 1, 300, 3)                 # the first item starts at a tile's last byte
    t.add(3 * T + 500, 77, 0)
    t.add(6 * T + 9, 1000, 9)                # two whole tiles apart (tiles 4 and 5 hold nothing)
    t.add(12 * T + 100, 50, 15)              # five whole tiles apart (7 to 11)
    t.add(13 * T - 901, 900, 1)              # ends one byte in front of t0 = 13 T; the next item starts two tiles on
    t.add(15 * T, 16, 8)
    t.add(16 * T - 800, 800, 7)              # ends exactly at t0 = 16 T; the next item starts two tiles on
    t.add(18 * T + 1, 20, 0)
    t.add(20 * T + 5000, 3 * T + 1000, 8)    # one item over four tiles (20 to 23) that starts mid-tile
    cap = t.done()

    def probe():
        first, count = tiles_of(t.items, mis)
        assert (first, count) == (1, 23)
        by = collections.defaultdict(list)
        for p in portions(t.items, mis):
            by[p.tile].append(p)
        empty = [k for k in range(first, first + count) if not by[k]]
        assert empty == [4, 5, 7, 8, 9, 10, 11, 13, 14, 16, 17, 19]
        ends = {k: max(p.d1 for kk in by if kk < k for p in by[kk]) for k in empty}
        assert ends[13] == 13 * T - 1 and ends[16] == 16 * T and ends[4] < 4 * T     # tile_lane's `continue`: <= t0, with equality
        assert [p.d1 - p.d0 for p in by[1]] == [1] and by[1][0].head == 1 and by[2][0].item == by[1][0].item
        assert [len(by[k]) for k in (20, 21, 22, 23)] == [1, 1, 1, 1] and len({by[k][0].item for k in (20, 21, 22, 23)}) == 1
        assert by[20][0].d0 % T == 5000 and [by[k][0].chunks for k in (21, 22)] == [1024, 1024]
        return {"empty_tiles": len(empty)}
    return SIZES, t.items, cap, probe


def _crowd(mis):
    """a tile of 16 384 one-byte items from scattered sources, an empty tile, a tile of 1024 sixteen-byte items on the 16-byte
    grid, alternately congruent and not"""
    t = _Table(mis, 9900)
    for k in range(TILE):
        t.add(TILE + k, 1, t.rnd.randrange(16))
    for k in range(1024):
        t.add(3 * TILE + 16 * k, 16, 0 if k % 2 == 0 else 1 + (k // 2) % 15)
    cap = t.done()

    def probe():
        by = collections.defaultdict(list)
        for p in portions(t.items, mis):
            by[p.tile].append(p)
        assert sorted(by) == [1, 3] and len(by[1]) == TILE and len(by[3]) == 1024
        assert all(p.d1 - p.d0 == 1 and p.chunks == 0 for p in by[1]) and len({t.items[p.item][:2] for p in by[1]}) > TILE // 2
        assert all((p.head, p.chunks, p.tail) == (0, 1, 0) for p in by[3])
        rs = [p.r for p in sorted(by[3], key=lambda p: p.d0)]
        assert all(r == 0 for r in rs[0::2]) and set(rs[1::2]) == set(range(1, 16))
        return {"items": len(t.items)}
    return SIZES, t.items, cap, probe


_PLANS = {"seam": _seam, "chunks": _chunks, "empty": _empty, "crowd": _crowd}


def plan(family, mis):
    assert mis in range(16)
    return _PLANS[family](mis)


def rounds(n_tiles, mis):
    """a destination of n_tiles tiles, every tile with one item of 100 to 700 bytes whose kind cycles with period 7
    (ROUND_KINDS): inside the tile, across its first byte, across its last, congruent, or shifted by 1, 8 or 15.  7 is
    coprime to the grid's cap, so a workgroup that walks tiles g, g + cap, g + 2 cap, ... meets another kind in every trip
    -> as plan()"""
    t = _Table(mis, 9950)
    for tile in range(n_tiles):
        kind = ROUND_KINDS[tile % 7]
        if kind == "across-end" and tile == n_tiles - 1:
            kind = "inside"
        n = t.rnd.randrange(100, 701)
        if kind == "across-start":
            t.add(tile * TILE - t.rnd.randrange(1, n), n, t.rnd.randrange(16))
        elif kind == "across-end":
            t.add((tile + 1) * TILE - t.rnd.randrange(1, n), n, t.rnd.randrange(16))
        else:
            r = {"inside": 3, "congruent": 0, "r1": 1, "r8": 8, "r15": 15}[kind]
            t.add(tile * TILE + t.rnd.randrange(1000, TILE - 2000), n, r)
    cap = t.done(slack=0)
    cap = max(cap, n_tiles * TILE - mis)

    def probe():
        assert tiles_of(t.items, mis) == (0, n_tiles) and len(t.items) == n_tiles
        ps = portions(t.items, mis)
        per_tile = collections.Counter(p.tile for p in ps)
        assert set(per_tile) == set(range(n_tiles)) and set(per_tile.values()) <= {1, 2}
        split = sum(1 for q, k in collections.Counter(p.item for p in ps).items() if k == 2)
        assert split >= 2 * (n_tiles // 7) - 1
        assert {p.r for p in ps} >= {0, 1, 3, 8, 15} and all(100 <= n <= 700 for _, _, n, _ in t.items)
        return {"tiles": n_tiles, "items": len(t.items), "bytes": sum(n for _, _, n, _ in t.items), "split_items": split}
    return SIZES, t.items, cap, probe
