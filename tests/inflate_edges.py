"""The raw-deflate edge cases of the inflate tests, each named by the edge it sits on and by the class it must fall in
("family/what:class"), the judge -- Python's zlib --, and seeded mutations.  Used by tests/test_inflate_edges_cpu.py
(inflate_host, the g++ lane scheme) and tests/test_gpu_inflate_edges.py (the kernel)."""
import functools
import random
import zlib

import inflate_craft as C

OK, RESULT, EOF, OUT_CAP = "ok", "result", "eof", "out_cap"
FAMILIES = ("block", "len", "dist", "copy", "table", "input", "output", "grace")


def judge(data, cap):
    """-> (class, bytes or None, input bytes used or None): zlib.decompressobj(-15) with room for cap + 1 bytes; raises ->
    RESULT, more than cap bytes -> OUT_CAP, not at its end -> EOF, otherwise OK"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(bytes(data), cap + 1)
    except zlib.error:
        return RESULT, None, None
    if len(out) > cap:
        return OUT_CAP, None, None
    if not d.eof:
        return EOF, None, None
    return OK, out, len(data) - len(d.unused_data)


def _rand(n, seed, below=256):
    r = random.Random(seed)
    return bytes(r.randrange(below) for _ in range(n))


def _fixed(tokens, final=True, eob=True, fill=0):
    w = C.Bits()
    C.fixed(w, tokens, final=final, eob=eob)
    return w.bytes(fill)


# a small dynamic code: literals a - d, end of block and the shortest length, two bits each ... and four distance codes;
# its lengths are spelled with repeats, one of which runs across the seam between the two alphabets
def _seam_header():
    lit = [0] * 258
    for s in (97, 98, 254, 255, 256, 257):
        lit[s] = 3
    lit[97], lit[98] = 2, 2     # 2 / 4 + 4 / 8 = 1
    dist = [3, 3, 3, 3, 3, 3, 3, 3]
    # 0 .. 96 zero | 97, 98 = 2 | 99 .. 253 zero (155) | 254 .. 257 = 3 and the eight distance lengths = 3: twelve threes
    seq = [(18, 97 - 11), (2, 0), (2, 0), (18, 127), (18, 155 - 138 - 11), (3, 0), (16, 3), (16, 2)]
    cl = [0] * 19
    cl[18], cl[2], cl[3], cl[16] = 2, 2, 2, 2
    return lit, dist, cl, seq


def seam_block(tokens, final=True, eob=True):
    lit, dist, cl, seq = _seam_header()
    w = C.Bits()
    C.dynamic(w, tokens, lit, dist, final=final, eob=eob, cl_lens=cl, cl_seq=seq)
    return w.bytes()


def _dyn(tokens, lit, dist, **kw):
    w = C.Bits()
    C.dynamic(w, tokens, lit, dist, final=True, **kw)
    return w.bytes()


def _ladder(symbols, top):
    """lengths 1, 2, ..., top - 1, top, top over the symbols given (a complete set): {symbol: length}"""
    assert len(symbols) == top + 1
    return {s: min(i + 1, top) for i, s in enumerate(symbols)}


def _lens(n, assign):
    out = [0] * n
    for s, l in assign.items():
        out[s] = l
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, stream, out_cap, class, residue of the destination modulo 16)]"""
    out = []

    def add(name, data, cap, cls):
        out.append(("%s:%s" % (name, cls), bytes(data), cap, cls, 5 if len(out) % 2 else 0))

    # ---- block forms
    w = C.Bits()
    C.stored(w, b"", final=True)
    add("block/stored-empty", w.bytes(), 0, OK)
    w = C.Bits()
    C.stored(w, _rand(65535, 1), final=True)
    add("block/stored-65535", w.bytes(), 65535, OK)
    add("block/stored-65535-room-1-short", w.bytes(), 65534, OUT_CAP)
    add("block/stored-65535-cut", w.bytes()[:40000], 65535, EOF)
    for j in range(8):   # a fixed block of j nine-bit literals in front: the stored block's header begins at every bit offset
        w = C.Bits()
        C.fixed(w, [200] * j)
        at = w.bit_len % 8
        C.stored(w, _rand(100 + j, 2), final=True)
        add("block/stored-at-bit-%d" % at, w.bytes(), 100 + 2 * j, OK)
    assert {c[0] for c in out if "stored-at-bit" in c[0]} == {"block/stored-at-bit-%d:ok" % k for k in range(8)}
    w = C.Bits()
    C.stored(w, b"abc", final=True, nlength=0x1234)
    add("block/stored-nlen-mismatch", w.bytes(), 3, RESULT)
    w = C.Bits()
    C.fixed(w, list(_rand(30, 3, 128)))
    C.fixed(w, list(_rand(50, 4, 128)), final=True)
    add("block/boundary-inside-a-64-byte-store", w.bytes(), 80, OK)
    w = C.Bits()
    C.stored(w, _rand(37, 5))
    C.fixed(w, list(_rand(40, 6, 128)))
    C.stored(w, _rand(29, 7))
    C.fixed(w, [65, ("m", 20, 1)], final=True)
    add("block/stored-fixed-stored-fixed", w.bytes(), 37 + 40 + 29 + 21, OK)
    w = C.Bits()
    C.fixed(w, [])
    C.fixed(w, [66], final=True)
    add("block/empty-fixed-not-final", w.bytes(), 1, OK)
    add("block/final-only-end-of-block", _fixed([]), 0, OK)
    add("block/type-3", bytes([0x07]), 10, RESULT)
    add("block/type-3-not-final", bytes([0x06]), 10, RESULT)
    for j in range(8):
        w = C.Bits()
        C.fixed(w, [200] * j, final=True)
        spare = -w.bit_len % 8
        add("block/trailing-bits-%d" % spare, w.bytes(fill=1), j, OK)
    add("block/trailing-bytes", _fixed([65, 66]) + b"\xff\x07\x00junk", 2, OK)

    # ---- every length symbol, its fewest and its most extra bits
    for s in range(257, 286):
        base, xb = C.LEN_BASE[s - 257], C.LEN_EXTRA[s - 257]
        for length in sorted({base, base + (1 << xb) - 1}):
            add("len/symbol-%d-length-%d" % (s, length), _fixed([97, ("m", length, 1, s)]), 1 + length, OK)
    add("len/symbol-286", _fixed([97, ("lit", 286)]), 10, RESULT)
    add("len/symbol-287", _fixed([97, ("lit", 287)]), 10, RESULT)

    # ---- every distance symbol likewise, with exactly `distance` bytes produced, and with one byte fewer
    def far(distance, produced):
        w = C.Bits()
        C.stored(w, _rand(produced, distance))
        C.fixed(w, [("m", 3, distance)], final=True)
        return w.bytes()

    for s in range(30):
        base, xb = C.DIST_BASE[s], C.DIST_EXTRA[s]
        for distance in sorted({base, base + (1 << xb) - 1}):
            add("dist/symbol-%d-distance-%d-of-%d" % (s, distance, distance), far(distance, distance), distance + 3, OK)
    add("dist/32768-of-32767", far(32768, 32767), 32770, RESULT)
    add("dist/2-of-1", _fixed([97, ("m", 3, 2)]), 10, RESULT)
    add("dist/1-of-0", _fixed([("m", 3, 1)]), 10, RESULT)
    add("dist/symbol-30", _fixed([97, ("len", 257, 0), ("dist", 30, 0)]), 10, RESULT)
    add("dist/symbol-31", _fixed([97, ("len", 257, 0), ("dist", 31, 0)]), 10, RESULT)

    # ---- copies
    head = list(range(33, 33 + 70))
    for distance in (1, 2, 3, 63, 64, 65):
        for length in (3, 63, 64, 65, 258):
            add("copy/distance-%d-length-%d" % (distance, length), _fixed(head + [("m", length, distance)]), 70 + length, OK)
    add("copy/reads-pending-literals", _fixed([97, 98, 99, ("m", 5, 3), 100, ("m", 4, 2)]), 13, OK)
    add("copy/chain-of-short-matches", _fixed([97, 98] + [("m", 3, 2), 99, ("m", 4, 1)] * 40), 2 + 8 * 40, OK)
    w = C.Bits()
    C.fixed(w, list(_rand(20, 8, 128)))
    C.fixed(w, [("m", 30, 20), 65], final=True)
    add("copy/across-a-block-boundary", w.bytes(), 51, OK)
    w = C.Bits()
    C.stored(w, _rand(300, 9))
    C.fixed(w, [("m", 258, 300), ("m", 100, 258)], final=True)
    add("copy/from-a-stored-block", w.bytes(), 658, OK)
    add("copy/ends-at-out-cap", _fixed(head + [("m", 100, 7)]), 170, OK)
    add("copy/ends-one-past-out-cap", _fixed(head + [("m", 100, 7)]), 169, OUT_CAP)

    # ---- tables
    lit15 = _ladder([97, 98, 99, 100, 101, 102, 103, 104, 105, 106, 107, 108, 109, 110, 256, 257], 15)
    add("table/codes-of-15-bits", _dyn([97, 110, 105, ("m", 3, 1), 98], _lens(258, lit15), C.FLAT_DIST), 7, OK)
    lit11 = _ladder([97, 98, 99, 100, 101, 102, 103, 104, 105, 256, 107, 257], 11)
    add("table/literal-codes-of-10-and-11-bits", _dyn([97, 105, 107, ("m", 3, 2), 107], _lens(258, lit11), C.FLAT_DIST), 7, OK)
    assert lit11[256] == 10 and lit11[107] == 11 == lit11[257] and lit11[105] == 9
    dist9 = _ladder([0, 1, 2, 3, 4, 5, 6, 8, 9, 7], 9)
    assert dist9[8] == 8 and dist9[9] == 9 == dist9[7]
    add("table/distance-codes-of-8-and-9-bits",
        _dyn(list(range(40, 80)) + [("m", 5, 17), ("m", 6, 25), ("m", 3, 13)], C.FLAT_LIT, _lens(10, dist9)), 54, OK)
    cl7 = _lens(19, {8: 1, 9: 2, 4: 3, 5: 4, 0: 5, 1: 6, 2: 7, 3: 7})
    add("table/code-length-codes-of-7-bits", _dyn([97, ("m", 9, 1)], C.FLAT_LIT, C.FLAT_DIST, cl_lens=cl7), 10, OK)
    one = _lens(257, {256: 1})
    add("table/one-literal-code-of-length-1", _dyn([], one, [0]), 0, OK)
    add("table/one-literal-code-its-other-pattern", _dyn([("bits", 1, 1)], one, [0], eob=False), 0, RESULT)
    two = _lens(258, {97: 2, 98: 2, 256: 2, 257: 2})
    add("table/one-distance-code-of-length-1", _dyn([97, ("m", 3, 1)], two, [1]), 4, OK)
    add("table/one-distance-code-its-other-pattern", _dyn([97, ("len", 257, 0), ("bits", 1, 1)], two, [1]), 4, RESULT)
    add("table/no-distance-code-literals-only", _dyn([97, 98, 97], two, [0]), 3, OK)
    add("table/no-distance-code-and-a-match", _dyn([97, ("len", 257, 0), ("bits", 0, 1)], two, [0]), 4, RESULT)
    add("table/literals-over-subscribed", _dyn([], _lens(258, {97: 1, 98: 1, 256: 1}), [1, 1], body=False), 4, RESULT)
    add("table/literals-incomplete", _dyn([], _lens(258, {97: 2, 256: 2}), [1, 1], body=False), 4, RESULT)
    add("table/distances-over-subscribed", _dyn([], two, [1, 1, 1], body=False), 4, RESULT)
    add("table/distances-incomplete", _dyn([], two, [2, 2, 2], body=False), 4, RESULT)
    add("table/code-lengths-over-subscribed", _dyn([], two, [1, 1], cl_lens=_lens(19, {0: 1, 1: 1, 2: 1}), cl_seq=[], body=False), 4, RESULT)
    add("table/code-lengths-incomplete", _dyn([], two, [1, 1], cl_lens=_lens(19, {0: 1}), cl_seq=[], body=False), 4, RESULT)
    add("table/code-lengths-without-any-code", _dyn([], two, [1, 1], cl_lens=[0] * 19, cl_seq=[(0, 0)] * 260, body=False) + bytes(4), 4, RESULT)
    add("table/code-lengths-without-any-code-cut", _dyn([], two, [1, 1], cl_lens=[0] * 19, cl_seq=[(0, 0)] * 100, body=False)[:8], 4, EOF)
    add("table/no-end-of-block-code", _dyn([], _lens(258, {97: 1, 98: 1}), [1, 1], body=False), 4, RESULT)
    for h in (30, 31):
        add("table/hlit-%d" % h, _dyn([], two, [1, 1], hlit=h, cl_seq=[], body=False), 4, RESULT)
        add("table/hdist-%d" % h, _dyn([], two, [1, 1], hdist=h, cl_seq=[], body=False), 4, RESULT)
    add("table/repeat-16-with-nothing-before", _dyn([], two, [1, 1], cl_seq=[(16, 0)], body=False) + bytes(2), 4, RESULT)
    add("table/repeat-16-cut-before-its-extra-bits", _dyn([], two, [1, 1], cl_seq=[], body=False)[:-1], 4, EOF)
    add("table/repeats-run-over-the-lengths", _dyn([], two, [1, 1], cl_seq=[(18, 127), (18, 127 - 138 + 122 - 1), (18, 0)], body=False) + bytes(2),
        4, RESULT)
    add("table/repeat-16-runs-over-the-lengths", _dyn([], two, [1, 1], cl_seq=[(18, 127), (18, 120 - 11), (1, 0), (16, 0)], body=False) + bytes(2),
        4, RESULT)
    add("table/repeat-across-the-seam", seam_block([97, 98, 98, ("m", 3, 2), 97]), 7, OK)

    # ---- input
    small = seam_block([97, 98, 98, ("m", 3, 2), 97, ("m", 3, 5), 98])
    assert judge(small, 11)[0] == OK and 12 <= len(small) <= 40
    for cut in range(len(small)):
        add("input/dynamic-block-cut-at-%d" % cut, small[:cut], 11, EOF)
    add("input/dynamic-block-whole", small, 11, OK)
    for n in (15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049):   # k eight-bit literals: k + 2 bytes
        data = _fixed(list(_rand(n - 2, n, 144)))
        assert len(data) == n
        add("input/stream-of-%d-bytes" % n, data, n - 2, OK)
        add("input/stream-of-%d-bytes-less-one" % n, data[:-1], n - 2, EOF)
    w = C.Bits()
    C.stored(w, _rand(1024 - 5 - 3, 10))
    C.fixed(w, [65, ("m", 3, 1)], final=True)       # the second block's header begins at the input window's seam
    add("input/block-header-at-the-window-seam", w.bytes(), 1024 - 8 + 4, OK)

    # ---- output
    for n in (0, 1, 63, 64, 65, 127, 128, 129):
        for res in (0, 5):
            data = _fixed(list(_rand(n, 100 + n, 144)))
            out.append(("output/%d-bytes-at-residue-%d:ok" % (n, res), data, n, OK, res))
        if n:
            add("output/%d-bytes-room-one-short" % n, _fixed(list(_rand(n, 100 + n, 144))), n - 1, OUT_CAP)
    w = C.Bits()
    C.stored(w, _rand(200, 11), final=True)
    for res in range(16):
        out.append(("output/stored-200-at-residue-%d:ok" % res, w.bytes(), 200, OK, res))
    add("output/stored-room-exact-then-literal", w.bytes()[:0] + _stored_then([65]), 200, OUT_CAP)

    # ---- the byte behind the room: the yardstick reads on until it has something to write
    add("grace/literal-then-end", _fixed([97]), 0, OUT_CAP)
    add("grace/two-literals", _fixed([97, 98]), 0, OUT_CAP)
    add("grace/literal-then-symbol-286", _fixed([97, ("lit", 286)]), 0, RESULT)
    add("grace/literal-then-match-too-far", _fixed([97, ("m", 3, 2)]), 0, OUT_CAP)
    add("grace/literal-then-match-too-far-with-room", _fixed([97, ("m", 3, 2)]), 1, RESULT)
    w = C.Bits()
    C.fixed(w, [97])
    w.put(7, 3)
    add("grace/literal-then-block-type-3", w.bytes(), 0, RESULT)
    w = C.Bits()
    C.fixed(w, [97])
    C.stored(w, b"", final=True)
    add("grace/literal-then-empty-stored", w.bytes(), 0, OUT_CAP)
    w = C.Bits()
    C.fixed(w, [97])
    C.stored(w, b"", final=True, nlength=1)
    add("grace/literal-then-stored-nlen-mismatch", w.bytes(), 0, RESULT)
    add("grace/literal-then-cut", _fixed([97, 98, 99])[:2], 0, OUT_CAP)
    add("grace/match-fills-room-plus-one", _fixed([97, ("m", 10, 1)]), 10, OUT_CAP)
    add("grace/match-fills-room-plus-one-then-286", _fixed([97, ("m", 10, 1), ("lit", 286)]), 10, RESULT)
    w = C.Bits()
    C.stored(w, _rand(11, 12))
    w.put(7, 3)
    add("grace/stored-fills-room-plus-one-then-type-3", w.bytes(), 10, RESULT)
    assert len({c[0] for c in out}) == len(out)
    return out


def _stored_then(tokens):
    w = C.Bits()
    C.stored(w, _rand(200, 11))
    C.fixed(w, tokens, final=True)
    return w.bytes()


def family(case):
    return case[0].split("/")[0]


def _deflate(data, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


@functools.lru_cache(maxsize=None)
def seeds():
    """[(stream, size)]: zlib-made and crafted good streams that the mutations start from"""
    r = random.Random(77)
    words = [b"alpha ", b"beta ", b"gamma ", b"delta ", b"epsilon\n", b"0123456789"]
    texts = [b"".join(r.choice(words) for _ in range(k)) for k in (3, 40, 300)] + [_rand(200, 5), _rand(900, 6, 4), b"z" * 700]
    out = []
    for t in texts:
        for level, strat in ((0, 0), (1, 0), (6, 0), (9, 0), (6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_RLE)):
            out.append((_deflate(t, level, strat), len(t)))
    for name, data, cap, cls, _ in cases():
        if cls == OK and len(data) <= 1200:
            out.append((data, cap))
    return out


def mutations(n, seed, pool=None):
    """n (stream, out_cap) pairs: byte flips, cuts, spliced headers and changed room, of seeds() -- or of `pool`, a list of
    (good stream, its size)"""
    r = random.Random(seed)
    pool = seeds() if pool is None else pool
    out = []
    while len(out) < n:
        data, size = pool[r.randrange(len(pool))]
        m = bytearray(data)
        kind = r.randrange(6)
        if kind == 0 and m:      # one bit, early (headers and tables) or anywhere
            m[r.randrange(min(len(m), 24)) if r.random() < 0.6 else r.randrange(len(m))] ^= 1 << r.randrange(8)
        elif kind == 1 and m:    # a byte
            m[r.randrange(len(m))] = r.randrange(256)
        elif kind == 2:          # a cut
            m = m[:r.randrange(len(m) + 1)]
        elif kind == 3:          # another stream's head on this one's tail
            other = pool[r.randrange(len(pool))][0]
            k = r.randrange(1, 12)
            m = bytearray(other[:k]) + m[min(k, len(m)):]
        elif kind == 4 and m:    # several bits
            for _ in range(r.randrange(2, 6)):
                m[r.randrange(len(m))] ^= 1 << r.randrange(8)
        cap = size if r.random() < 0.7 else max(0, size + r.choice((-2, -1, 1, 7)))
        out.append((bytes(m), cap))
    return out


def tiny_items(n, seed):
    """n streams of at most 200 bytes, good and damaged interleaved (for a launch in which every workgroup takes many):
    [(stream, out_cap)] drawn from a pool of a few dozen"""
    r = random.Random(seed)
    good = [(d, c) for _, d, c, cls, _ in cases() if cls == OK and len(d) <= 200 and c <= 400]
    bad = [(d, c) for _, d, c, cls, _ in cases() if cls != OK and len(d) <= 200 and c <= 400]
    r.shuffle(good), r.shuffle(bad)
    good, bad = good[:40], bad[:24]
    out = []
    for i in range(n):
        out.append(bad[(i // 3) % len(bad)] if i % 3 == 1 else good[(i + i // 7) % len(good)])
    return out
