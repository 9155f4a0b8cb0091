"""The packet matrix of tests/test_packet_matrix_cpu.py and tests/test_gpu_packet_matrix.py: crafted streams that walk
the edges at which the decode kernels change code path -- every match length in every posState, every distance slot,
the (distance, length) pairs on both sides of the fast loop's own copies, every follower behind a pending copy, the
distances at the edge of the window, the output and size limits around kFastOutput and kFastCopyRoom.  A plain module
like tests/kernel_streams.py, not a conftest.

Everything is deterministic (fixed seeds) and written packet by packet with tests/lzma_craft.py.  A section returns a
list of Case: (name, job, crafted, log, emu).  job is (Stream, want) as in pipeline_streams; crafted is what the
crafter's own window model expects of a VALID stream (None otherwise); log is the section's coverage record, made
while emitting: one P per packet; emu says how tests/test_packet_matrix_cpu.py runs the stream through the emulated
fast loops (None: not at all).

Shape of an emulated stream: a short prefix (random literals, then long matches), the section's packets, a trailer of
40 random literals and the end marker, with 400 bytes of room behind the output -- the fast loop (32 bytes of input,
128 bytes of output room) and wave_copy<false> (336 bytes of room) see every packet of the section."""
import collections
import functools
import random

import pipeline_streams as ps  # (puts the repository root and tests/ on sys.path)
from pipeline_streams import alone_job, raw2_job

from lzma_craft import Encoder, Window, alone_header, lzma2_lzma_chunk, lzma2_stored, props_byte  # noqa: E402

P = collections.namedtuple("P", "tag kind len rep0 ps state fill")
Case = collections.namedtuple("Case", "name job crafted log emu")
Emu = collections.namedtuple("Emu", "payload props dict_size ends")   # ends: "trailer", "marker" (exit 2), "error" (exit 1)

ROOM = 400          # > kFastCopyRoom = 336: room behind the output of a stream whose every packet the fast loop sees
TRAILER = 40        # random literals in front of the end marker: more than kFastInput = 32 bytes of input
COMPACT_PROPS = [(3, 0, 2), (0, 2, 0), (1, 1, 1)]
FULL_PROPS = [(3, 0, 4), (0, 4, 4)]
HBM_LENGTH_PROPS = [(8, 1, 0), (5, 4, 2)]
HBM_PROPS = (8, 1, 2)
KINDS = ("match", "rep0", "rep1", "rep2", "rep3")


class Rec(Encoder):
    """lzma_craft.Encoder that writes down every packet in front of emitting it: P(tag, kind, length, rep0 of the copy,
    posState, state, bytes in the window).  `tag` is whatever the section set last (None: prefix, padding, trailer)."""

    def __init__(self, lc=3, lp=0, pb=2, dict_size=1 << 16, window=None):
        super().__init__(lc, lp, pb, dict_size, window)
        self.log = []
        self.tag = None

    def _note(self, kind, length, rep0):
        w = self.w
        self.log.append(P(self.tag, kind, length, rep0, w.pos & ((1 << self.pb) - 1), self.state, w.size if w.full else w.pos))

    def literal(self, byte):
        self._note("lit", 1, self.reps[0])
        super().literal(byte)

    def match(self, distance, length, copy=True):
        self._note("match", length, distance - 1)
        super().match(distance, length, copy)

    def end_marker(self):
        self._note("marker", 0, 0xFFFFFFFF)
        super().end_marker()

    def short_rep(self):
        self._note("srep", 1, self.reps[0])
        super().short_rep()

    def rep(self, idx, length):
        self._note("rep%d" % idx, length, self.reps[idx])
        super().rep(idx, length)

    def _copy(self, dist, length):   # window.CopyMatch with slices where neither end wraps (megabytes of long matches)
        w = self.w
        if dist <= w.pos and w.pos + length < w.size:
            src = w.buf[w.pos - dist:w.pos - dist + min(dist, length)]
            if dist < length:
                src = (src * (length // dist + 1))[:length]
            w.buf[w.pos:w.pos + length] = src
            w.pos += length
            w.total += src
        else:
            super()._copy(dist, length)


def fill_of(e):
    return e.w.size if e.w.full else e.w.pos


def grow(e, rnd, upto, lits=24):
    """the prefix: `lits` random literals, then long matches at varied distances with a literal behind each, until the
    window holds `upto` bytes at least"""
    for _ in range(lits if not e.log else 0):
        e.literal(rnd.randrange(256))
    while len(e.w.total) < upto:
        f = fill_of(e)
        e.match(rnd.randint(max(1, f // 2), f), min(273, max(2, upto - len(e.w.total))))
        e.literal(rnd.randrange(256))


def pad_to(e, rnd, n):
    """exactly n more bytes, in as few packets as it takes (long matches, a literal where one byte is left)"""
    while n > 0:
        if n == 1 or e.w.empty():
            e.literal(rnd.randrange(256))
            n -= 1
            continue
        k = min(273, n)
        f = fill_of(e)
        e.match(rnd.randint(max(1, f // 2), f), k)
        n -= k


def finish1(e, rnd, name, emu=True, known_size=False, room=ROOM):
    """trailer + end marker (or the size in the header) -> Case of an LZMA1 stream"""
    props, ds = (e.lc, e.lp, e.pb), e.w.size
    e.tag = None
    for _ in range(TRAILER):
        e.literal(rnd.randrange(256))
    want = bytes(e.w.total)
    if known_size:
        blob = alone_header(*props, ds, size=len(want)) + e.payload()
    else:
        e.end_marker()
        blob = alone_header(*props, ds) + e.payload()
    return Case(name, alone_job(blob, len(want) + room), want, tuple(e.log),
                Emu(blob[13:], props, ds, "trailer") if emu else None)


def tagged(cases, tag=None):
    """the packets of the sections proper (tag not None, or a chosen tag) of `cases`"""
    return [p for c in cases for p in c.log if (p.tag is not None if tag is None else p.tag == tag)]


# ------------------------------------------------------------------ 1. lengths ----
def _length_stream(props, kind, seed, thin):
    rnd = random.Random(seed)
    e = Rec(*props, dict_size=1 << 16)
    nps = 1 << props[2]
    grow(e, rnd, 400)
    for d in (5, 33, 130, 277):        # four distinct reps
        e.match(d, 3)
        e.literal(rnd.randrange(256))
    for length in range(2, 274):
        # the low and mid trees are per posState (lengths 2 .. 17); the high tree is shared: thin = one posState per length
        todo = set(range(nps)) if not thin or length < 18 else {e.w.pos & (nps - 1)}
        while todo:
            now = e.w.pos & (nps - 1)
            ps_ = min(todo, key=lambda t: (t - now) % nps)
            for _ in range((ps_ - now) % nps):
                e.literal(rnd.randrange(256))
            e.tag = "len"
            if kind == "match":
                e.match(1 + (length * 7 + ps_ * 3) % 300, length)
            else:
                e.rep(int(kind[3]), length)
            e.tag = None
            todo.discard(ps_)
    return finish1(e, rnd, "lengths %s %s%s" % (props, kind, " thin" if thin else ""))


@functools.lru_cache(maxsize=None)
def lengths(props_list=tuple(COMPACT_PROPS + FULL_PROPS), thin=False):
    """every length 2 .. 273 x every posState x {simple match, rep0 long, rep1 .. 3}: one stream per properties and kind.
    Coverage: {(props, kind, length, posState)} of the packets tagged "len"."""
    return tuple(_length_stream(props, kind, 1000 + 10 * i + k, thin)
                 for i, props in enumerate(props_list) for k, kind in enumerate(KINDS))


def lengths_coverage(cases):
    return {(c.emu.props, p.kind, p.len, p.ps) for c in cases for p in c.log if p.tag == "len"}


# ------------------------------------------------------------------ 2. slots ----
def slot_of(rep0):
    if rep0 < 4:
        return rep0
    n = rep0.bit_length()
    return ((n - 1) << 1) | ((rep0 >> (n - 2)) & 1)


def slot_targets(slot):
    """rep0 values of one pos slot: base, base + 1, middle, top; from slot 14 on the direct bits all zero, all one and
    alternating (both phases), each with align 0 and 15"""
    if slot < 4:
        return [slot]
    nbits = (slot >> 1) - 1
    base = (2 | (slot & 1)) << nbits
    out = {base, base + 1, base + (1 << (nbits - 1)), base + (1 << nbits) - 1}
    if slot >= 14:
        nd = nbits - 4
        ones = (1 << nd) - 1
        alt = int("01" * 16, 2) & ones
        for direct in (0, ones, alt, alt ^ ones):
            for align in (0, 15):
                out.add(base + (direct << 4) + align)
    return sorted(out)


def _slots_small(props, seed):
    """every distance 1 .. 128 x len_state 0 .. 3: exhaustive for the reverse trees of slots 4 .. 13"""
    rnd = random.Random(seed)
    e = Rec(*props, dict_size=1 << 16)
    grow(e, rnd, 300)
    for dist in range(1, 129):
        for length in (2, 3, 4, 5):
            e.tag = "small"
            e.match(dist, length)
            e.tag = None
        e.literal(rnd.randrange(256))
    return finish1(e, rnd, "slots: distances 1..128 x len_state %s" % (props,))


def _slots_big(props, seed, top_bits):
    """for every pos slot up to the one that holds 2^top_bits: slot_targets() as valid matches of one stream that is filled
    with 273-byte matches at varied distances"""
    rnd = random.Random(seed)
    e = Rec(*props, dict_size=1 << (top_bits + 1))
    targets = sorted({r for s in range(slot_of((1 << top_bits) - 1) + 1) for r in slot_targets(s)})
    grow(e, rnd, 64)
    for i, rep0 in enumerate(targets):
        while fill_of(e) <= rep0:
            f = fill_of(e)
            e.match(rnd.choice([1, 2, 3, 9, 64, 273, f // 3 + 1, f, rnd.randint(1, f)]), 273)
            if rnd.random() < 0.1:
                e.literal(rnd.randrange(256))
        e.tag = "big"
        e.match(rep0 + 1, 2 + i % 5)      # len_state 0 .. 3, and 3 again at length 6
        e.tag = None
        e.literal(rnd.randrange(256))
    return finish1(e, rnd, "slots: up to 2^%d %s" % (top_bits, props))


def _slots_invalid(slot):
    """a match of a pos slot beyond every window: the oracle says what happens"""
    rnd = random.Random(2200 + slot)
    e = Rec(3, 0, 2, dict_size=1 << 16)
    grow(e, rnd, 300)
    nbits = (slot >> 1) - 1
    rep0 = ((2 | (slot & 1)) << nbits) + (0x5A5A5A50 & ((1 << nbits) - 1))
    e.tag = "invalid"
    e.match(rep0 + 1, 2 + slot % 4, copy=False)
    want = bytes(e.w.total)
    blob = alone_header(3, 0, 2, 1 << 16) + e.payload() + bytes(8)
    return Case("slots: invalid slot %d" % slot, alone_job(blob, len(want) + ROOM), None, tuple(e.log),
                Emu(blob[13:], (3, 0, 2), 1 << 16, "error"))


# packet sequences behind the prefix (which ends in a literal at state 0) that lead to each of the twelve states
STATE_PATHS = {0: "L", 1: "MLL", 2: "RLL", 3: "SLL", 4: "ML", 5: "RL", 6: "SL", 7: "M", 8: "R", 9: "S", 10: "MM", 11: "MR"}


def _marker_behind(state, props, seed):
    rnd = random.Random(seed)
    e = Rec(*props, dict_size=1 << 16)
    grow(e, rnd, 200)
    for _ in range(8):
        e.literal(rnd.randrange(256))
    assert e.state == 0
    for c in STATE_PATHS[state]:
        if c == "L":
            e.literal(rnd.randrange(256))
        elif c == "M":
            e.match(rnd.randint(1, 200), 5)
        elif c == "R":
            e.rep(0, 4)
        else:
            e.short_rep()
    assert e.state == state
    want = bytes(e.w.total)
    e.tag = "marker"
    e.end_marker()
    blob = alone_header(*props, 1 << 16) + e.payload()
    return Case("slots: end marker behind state %d %s" % (state, props), alone_job(blob, len(want) + ROOM), want, tuple(e.log),
                Emu(blob[13:], props, 1 << 16, "marker"))


@functools.lru_cache(maxsize=None)
def slots(top_bits=21, props=(3, 0, 2)):
    """distances 1 .. 128 x len_state; every pos slot up to the one that holds 2^top_bits; every higher slot as an invalid
    match; the end marker behind every state"""
    out = [_slots_small(props, 2001), _slots_big(props, 2002, top_bits)]
    out += [_slots_invalid(s) for s in range(slot_of((1 << 21) - 1) + 1, 64)]
    out += [_marker_behind(s, props, 2100 + s) for s in range(12)]
    return tuple(out)


# ------------------------------------------------------------------ 3. copies ----
COPY_DISTS = tuple(range(1, 81)) + (127, 128, 129, 255, 256, 257, 272, 273, 274, 300)
FOLLOWERS = ("literal", "short rep", "rep0 long", "match inside")
PLACES = ("ends at the wrap", "ends 1 before", "ends 1 past", "ends len-1 past")


def copy_lens(dist):
    return sorted(n for n in {2, 3, dist - 1, dist, dist + 1, 62, 63, 64, 65, 127, 128, 129, 191, 192, 193, 272, 273} if 2 <= n <= 273)


def _follower(e, rnd, what, length):
    e.tag = "follow " + what
    if what == "literal":
        e.literal(rnd.randrange(256))       # state >= 7: a matched literal, consumes the copy's matchByte
    elif what == "short rep":
        e.short_rep()
    elif what == "rep0 long":
        e.rep(0, 2 + rnd.randrange(6))
    else:
        e.match((length + 1) // 2, 5)       # its source starts inside the copy just made
    e.tag = None


def _place(e, rnd, length, place):
    """pad so that the next copy of `length` bytes ends at / 1 before / 1 past / length - 1 past the wrap of the window"""
    past = {"ends at the wrap": 0, "ends 1 before": -1, "ends 1 past": 1, "ends len-1 past": length - 1}[place]
    start = (e.w.size + past - length) % e.w.size
    pad_to(e, rnd, (start - e.w.pos) % e.w.size)
    assert e.w.pos == start


def _copy_stream(props, dists, lens_of, dict_size, seed, followers=FOLLOWERS, place=False, rep_dists=None):
    rnd = random.Random(seed)
    e = Rec(*props, dict_size=dict_size)
    grow(e, rnd, max(320, max(dists) + 8))
    for dist in dists:
        for k, length in enumerate(lens_of(dist)):
            for j, what in enumerate(followers):
                if place and j == 0:
                    _place(e, rnd, length, PLACES[(dist + k) % 4])
                    e.tag = "placed " + PLACES[(dist + k) % 4]
                else:
                    e.tag = "copy match"
                e.match(dist, length)
                _follower(e, rnd, what, length)
                if rep_dists is not None and dist not in rep_dists:
                    continue
                e.tag = "copy rep"
                e.rep(0 if e.reps[0] == dist - 1 else 1, length)   # (behind a follower that was a match the pair's distance is rep1)
                _follower(e, rnd, what, length)
    return finish1(e, rnd, "copies %s dict %d dists %d..%d%s" % (props, dict_size, dists[0], dists[-1], "" if len(followers) > 1 else " own"))


def own_copy_lens(dist):
    """the lengths the fast loop copies itself at this distance (gen_fastpath.py: copy_test)"""
    return list(range(2, min(dist, 64)))


PER_STREAM = 8      # distances per stream


@functools.lru_cache(maxsize=None)
def copies(props=(3, 0, 2), dict_size=1 << 16, dists=COPY_DISTS, own_dists=tuple(range(3, 71)), own_rep_dists=None):
    """COPY_DISTS x copy_lens(), each pair as a simple match and as a rep, each followed in turn by a matched literal, a short
    rep, a rep0 long and a match whose source starts inside the copy; and every pair the fast loop copies itself
    (3 <= dist <= 70, 2 <= len < min(dist, 64)) followed by a literal.  Eight distances per stream.  With a 4096-byte
    dictionary the window wraps hundreds of times, and the first copy of every pair is placed at the wrap (PLACES in
    rotation).  own_rep_dists: the distances at which the loop's own pairs appear as a rep too (None: all)."""
    place = dict_size <= 4096
    out = [_copy_stream(props, dists[i:i + PER_STREAM], copy_lens, dict_size, 3000 + i, place=place)
           for i in range(0, len(dists), PER_STREAM)]
    out += [_copy_stream(props, own_dists[i:i + PER_STREAM], own_copy_lens, dict_size, 3500 + i, followers=("literal",), place=place,
                         rep_dists=own_rep_dists)
            for i in range(0, len(own_dists), PER_STREAM)]
    return tuple(out)


def copies_coverage(cases):
    """{(kind of copy, distance, length, follower)}"""
    out = set()
    for c in cases:
        log = c.log
        for i, p in enumerate(log):
            if p.tag and (p.tag.startswith("copy") or p.tag.startswith("placed")):
                assert log[i + 1].tag.startswith("follow ")
                out.add(("match" if p.kind == "match" else "rep", p.rep0 + 1, p.len, log[i + 1].tag[7:]))
    return out


def placed_coverage(cases):
    """{(place, length)} of the copies placed at the wrap"""
    return {(p.tag[7:], p.len) for c in cases for p in c.log if p.tag and p.tag.startswith("placed")}


# ------------------------------------------------------------------ 4. all pairs (wave_copy) ----
PRECISE_DISTS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 272, 273)


def _pairs_stream(dist):
    rnd = random.Random(4000 + dist)
    e = Rec(3, 0, 2, dict_size=1 << 16)
    grow(e, rnd, 300)
    for length in range(2, 274):
        e.tag = "pair"
        e.match(dist, length)
        e.tag = None
        e.literal(rnd.randrange(256))
    return finish1(e, rnd, "all pairs dist %d" % dist, emu=False)


def _last_packet_stream(dist, length):
    rnd = random.Random(4500 + dist)          # (the same prefix for every length of a distance)
    e = Rec(3, 0, 2, dict_size=1 << 16)
    grow(e, rnd, 280, lits=12)
    e.tag = "last"
    e.match(dist, length)
    want = bytes(e.w.total)
    blob = alone_header(3, 0, 2, 1 << 16, size=len(want)) + e.payload()
    return Case("last packet dist %d len %d" % (dist, length), alone_job(blob, len(want)), want, tuple(e.log), None)


@functools.lru_cache(maxsize=None)
def all_pairs():
    """every 1 <= dist <= 273 x 2 <= len <= 273, a literal behind each match: one stream per distance (wave_copy<false>)"""
    return tuple(_pairs_stream(d) for d in range(1, 274))


@functools.lru_cache(maxsize=None)
def last_packets():
    """PRECISE_DISTS x every length as the LAST packet of a stream of known size without room to spare (wave_copy<true>)"""
    return tuple(_last_packet_stream(d, n) for d in PRECISE_DISTS for n in range(2, 274))


# ------------------------------------------------------------------ 5. window fill ----
FILLS = (1, 2, 63, 64, 65, 4095)


def _fill_followers(e, rnd):
    e.tag = "behind"
    e.literal(rnd.randrange(256))
    e.rep(0, 7)
    e.short_rep()
    e.literal(rnd.randrange(256))
    e.tag = None


def _fill_case1(props, kind, fill, delta, seed, dict_size=1 << 16):
    """LZMA1: at `fill` bytes in the window a match (or a rep) with rep0 = fill + delta.  A rep's rep0 comes from an
    earlier match that was valid then, and that match copied two bytes at least: a rep reaches rep0 <= fill - 2 only."""
    rnd = random.Random(seed)
    e = Rec(*props, dict_size=dict_size)
    rep0 = fill + delta
    valid = rep0 <= min(fill, dict_size - 1)
    if kind == "match":
        pad_to(e, rnd, fill)
        e.tag = "edge match"
        e.match(rep0 + 1, 9, copy=valid)
    else:
        assert delta == -2 and fill >= 3
        pad_to(e, rnd, rep0)
        e.match(rep0 + 1, 2)                 # rep0 == fill at this moment: the reference's off-by-one
        assert fill_of(e) == fill
        e.tag = "edge rep"
        e.rep(0, 9)
    e.tag = None
    name = "window fill %s %s fill %d rep0 fill%+d dict %d" % (props, kind, fill, delta, dict_size)
    if valid:
        _fill_followers(e, rnd)
        return finish1(e, rnd, name)
    want = bytes(e.w.total)
    blob = alone_header(*props, dict_size) + e.payload() + bytes(8)
    return Case(name, alone_job(blob, len(want) + ROOM), None, tuple(e.log), Emu(blob[13:], props, dict_size, "error"))


def _full_case1(props, kind, dict_size, delta, seed):
    """LZMA1, the window full: dist = dictSize + delta, as a match or (delta <= 0) as a rep of an earlier match"""
    rnd = random.Random(seed)
    e = Rec(*props, dict_size=dict_size)
    grow(e, rnd, dict_size + 300)
    assert e.w.full
    valid = delta <= 0
    if kind == "rep":
        e.match(dict_size + delta, 3)
        e.literal(rnd.randrange(256))
        e.tag = "edge rep"
        e.rep(0, 70)
    else:
        e.tag = "edge match"
        e.match(dict_size + delta, 70, copy=valid)
    e.tag = None
    name = "window full %s %s dict %d dist dict%+d" % (props, kind, dict_size, delta)
    if valid:
        _fill_followers(e, rnd)
        return finish1(e, rnd, name)
    want = bytes(e.w.total)
    blob = alone_header(*props, dict_size) + e.payload() + bytes(8)
    return Case(name, alone_job(blob, len(want) + ROOM), None, tuple(e.log), Emu(blob[13:], props, dict_size, "error"))


FIRST_EPOCH = 70_001


def _epoch2_case(props, kind, fill, rep0, dict_size, seed):
    """LZMA2: a first dictionary epoch of 70 001 bytes that ends with a match of rep0, a stored chunk of `fill` bytes that
    resets the dictionary, and a chunk that resets nothing and begins with a match (or a rep: rep0 survives the reset) of
    rep0 -- wbase != 0, and whatever lies in front of the epoch is the first epoch's bytes (window.go:135-140)"""
    rnd = random.Random(seed)
    w = Window(dict_size)
    e = Rec(*props, dict_size=dict_size, window=w)
    grow(e, rnd, FIRST_EPOCH - 300)
    pad_to(e, rnd, FIRST_EPOCH - 5 - len(w.total))
    e.match(min(rep0 + 1, dict_size), 5)
    if e.reps[0] != rep0:                    # rep0 == dictSize cannot be written as a match
        assert kind == "match"
    assert len(w.total) == FIRST_EPOCH
    blob = lzma2_lzma_chunk(0xE0, FIRST_EPOCH, e.payload(), props_byte(*props))
    w.reset()
    data = bytes(rnd.randrange(256) for _ in range(fill))
    for b in data:
        w.put(b)
    blob += lzma2_stored(data, dict_reset=True)
    e.new_chunk()
    start = len(w.total)
    valid = kind == "rep" or rep0 <= min(fill, dict_size - 1)
    e.tag = "edge " + kind
    if kind == "match":
        e.match(rep0 + 1, 9, copy=valid)
    else:
        e.rep(0, 9)
    e.tag = None
    if valid:
        _fill_followers(e, rnd)
        for _ in range(TRAILER):
            e.literal(rnd.randrange(256))
    want = bytes(w.total)
    name = "epoch 2 %s %s fill %d rep0 %d dict %d" % (props, kind, fill, rep0, dict_size)
    # an invalid match: the chunk announces the bytes it would have made
    blob += lzma2_lzma_chunk(0x80, (len(want) - start) if valid else 9, e.payload() + (b"" if valid else bytes(8))) + b"\x00"
    return Case(name, raw2_job(blob, len(want) + ROOM, dict_size), want if valid else None, tuple(e.log), None)


@functools.lru_cache(maxsize=None)
def window_fill(props=(3, 0, 2)):
    """match and rep with rep0 in {fill - 2 .. fill + 1} while the window fills and dist in {dictSize - 1 .. dictSize + 1}
    once it is full, as LZMA1 and as the second dictionary epoch of an LZMA2 stream"""
    out, seed = [], 5000
    for fill in FILLS:
        for delta in (-2, -1, 0, 1):
            if fill + delta >= 0:
                seed += 1
                out.append(_fill_case1(props, "match", fill, delta, seed))
        if fill >= 3:
            seed += 1
            out.append(_fill_case1(props, "rep", fill, -2, seed))
    for ds in (4096, 4097):
        for delta in (-1, 0, 1):
            for kind in ("match", "rep") if delta <= 0 else ("match",):
                seed += 1
                out.append(_full_case1(props, kind, ds, delta, seed))
    for fill in FILLS:
        for delta in (-2, -1, 0, 1):
            for kind in ("match", "rep"):
                if fill + delta >= 0:
                    seed += 1
                    out.append(_epoch2_case(props, kind, fill, fill + delta, 1 << 16, seed))
    for ds in (4096, 4097):
        for delta in (-1, 0, 1):
            for kind in ("match", "rep") if delta <= 0 else ("match",):
                seed += 1
                out.append(_epoch2_case(props, kind, ds + 40, ds + delta - 1, ds, seed))
    return tuple(out)


def window_coverage(cases):
    """{(form, kind, fill, rep0 - fill)} of the packets tagged "edge ..." (fill: dictSize once the window is full)"""
    return {(c.name.split()[0], p.kind[:3] if p.kind != "match" else "match", p.fill, p.rep0 - p.fill)
            for c in cases for p in c.log if p.tag and p.tag.startswith("edge")}


# ------------------------------------------------------------------ 6. limits ----
TAILS = ("literals", "len 273 dist 1", "len 273 dist 300", "len 63 dist 64", "reps")
SWEEP = 340


def _tail(e, rnd, which):
    """about 400 bytes"""
    e.tag = "tail"
    start = len(e.w.total)
    if which == "literals":
        for _ in range(400):
            e.literal(rnd.randrange(97, 123))
    elif which in ("len 273 dist 1", "len 273 dist 300"):
        d = int(which.split()[-1])
        e.match(d, 273)
        e.literal(rnd.randrange(256))
        e.match(d, 126)
    elif which == "len 63 dist 64":
        while len(e.w.total) - start < 400:
            e.match(64, 63)
            e.literal(rnd.randrange(256))
    else:
        for d in (7, 40, 111, 290):
            e.match(d, 4)
        while len(e.w.total) - start < 400:
            e.rep(rnd.randrange(4), rnd.choice([2, 9, 30, 70]))
            e.short_rep()
            if rnd.random() < 0.3:
                e.literal(rnd.randrange(256))
    e.tag = None


def _tail_encoder(which, props, lead=b""):
    """prefix + tail; lead: bytes a stored chunk has put into the window in front"""
    rnd = random.Random(6000 + TAILS.index(which))
    w = Window(1 << 16)
    for b in lead:
        w.put(b)
    e = Rec(*props, dict_size=1 << 16, window=w)
    if lead:
        e.literal(rnd.randrange(256))
    grow(e, rnd, 320 + len(lead), lits=16)
    _tail(e, rnd, which)
    return e


@functools.lru_cache(maxsize=None)
def limit_tails(props=(3, 0, 2)):
    """the five tails unswept, with an end marker and ample room: what the emulated loops run"""
    out = []
    for which in TAILS:
        e = _tail_encoder(which, props)
        rnd = random.Random(6100)
        out.append(finish1(e, rnd, "limits: tail %s" % which))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def limits(props=(3, 0, 2)):
    """five tails of about 400 bytes behind a short prefix, S bytes in all: out_cap over [S - 340, S + 1] with an end marker
    and with a known size, the header's size over [S - 340, S + 2] with ample room, the uncompressed size of a single
    LZMA2 chunk over the same values, and the out_cap sweep again behind stored chunks of 1 .. 4 bytes (the payload at
    every alignment in its dword)"""
    out = []
    pbyte = props_byte(*props)
    for which in TAILS:
        e = _tail_encoder(which, props)
        want = bytes(e.w.total)
        S = len(want)
        log = tuple(e.log)
        known = e.payload()
        e = _tail_encoder(which, props)     # (payload() has flushed the range coder: the same packets again)
        e.end_marker()
        marked = e.payload()
        hdr = alone_header(*props, 1 << 16)
        for cap in range(S - SWEEP, S + 2):
            out.append(Case("limits: %s, end marker, room %d" % (which, cap), alone_job(hdr + marked, cap), None, log, None))
            out.append(Case("limits: %s, known size, room %d" % (which, cap),
                            alone_job(alone_header(*props, 1 << 16, size=S) + known, cap), None, log, None))
        for size in range(S - SWEEP, S + 3):
            out.append(Case("limits: %s, size %d of %d" % (which, size, S),
                            alone_job(alone_header(*props, 1 << 16, size=size) + known, S + ROOM), None, log, None))
            out.append(Case("limits: %s, chunk size %d of %d" % (which, size, S),
                            raw2_job(lzma2_lzma_chunk(0xE0, size, known, pbyte) + b"\x00", S + ROOM), None, log, None))
        for k in (1, 2, 3, 4):
            lead = bytes(range(65, 65 + k))
            e2 = _tail_encoder(which, props, lead)
            S2 = len(e2.w.total)
            blob = lzma2_stored(lead, dict_reset=True) + lzma2_lzma_chunk(0xC0, S2 - k, e2.payload(), pbyte) + b"\x00"
            for cap in range(S2 - SWEEP, S2 + 2):
                out.append(Case("limits: %s behind %d stored bytes, room %d" % (which, k, cap), raw2_job(blob, cap), None,
                                tuple(e2.log), None))
    return tuple(out)


# ------------------------------------------------------------------ 7. the HBM-model kernel ----
@functools.lru_cache(maxsize=None)
def hbm():
    """sections 1, 3 and 5 at properties with lc + lp > 8: every unit is decoded by xlz_decode_kernel_hbm_model"""
    return (lengths(tuple(HBM_LENGTH_PROPS)) + copies(HBM_PROPS) + copies(HBM_PROPS, 4096) + window_fill(HBM_PROPS))


def jobs(cases):
    return [c.job for c in cases]


def packets(cases):
    return sum(len(c.log) for c in cases)
