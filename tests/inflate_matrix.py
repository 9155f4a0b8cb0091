"""The stream lists of the inflate matrix tests (tests/test_inflate_matrix_cpu.py: the judge, the token reader and the two
CPU twins; tests/test_gpu_inflate_matrix.py: the kernel, one launch per list).  Every list is [(stream, out_cap, residue of
the destination modulo 16)], seeded, and classed by nobody but the judge (inflate_edges.judge: Python's zlib).

    corpus()         zlib-made streams: six kinds of data x nine sizes x seven settings, each with exact room, room one
                     short, cut at two thirds, and with one byte flipped in the middle
    seam_sweep()     one crafted probe block pushed bit by bit across the seam of the kernel's 1024-byte input window, and
                     a stored block's LEN / NLEN pushed across it; each stream also cut to exactly 1024 bytes
    stored_matrix()  the stored copy: source offset modulo 16 x length x destination residue
    block_orders()   every order of three blocks of four kinds in one stream
    mutation_lists() inflate_edges.mutations of the small seeds, and of a pool of corpus streams of 2 to 40 KB
    pairs(grid)      eleven kinds of stream padded to three lengths, and empty inputs behind them, so that the launch rule
                     (items stable-sorted by in_len descending, workgroup g taking sorted positions g, g + grid, ...) runs a
                     chosen kind behind a chosen kind in the same LDS"""
import functools
import random
import zlib

import inflate_craft as C
import inflate_edges as E

WINDOW = 1024        # xlz_inflate_dev.h: kWindow
SEAM = 8 * WINDOW    # the first bit of the second window


# ---- 2. the zlib-made corpus
KINDS = ("text", "noise", "skewed", "below-4", "one-byte", "block-repeated")
SIZES = (1, 1023, 32767, 32768, 32769, 65535, 65536, 70000, 200000)
SETTINGS = ((0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY),
            (6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_RLE))
_WORDS = [w.encode() for w in ("the", "of", "wave", "lane", "block", "stored", "code", "length", "distance", "window", "literal", "a", "and",
                               "canonical", "Huffman", "table", "input", "output", "seam", "byte", "bit", "0123456789", "match", "copy",
                               "end", "header", "dynamic", "fixed", "repeat", "zero", "symbol", "extra")]


def data_of(kind, size, seed):
    r = random.Random("%s %d %d" % (kind, size, seed))
    if kind == "text":
        out = bytearray()
        while len(out) < size:
            out += r.choice(_WORDS) + (b"\n" if r.random() < 0.1 else b" ")
        return bytes(out[:size])
    if kind == "noise":
        return r.getrandbits(8 * size).to_bytes(size, "little")
    if kind == "skewed":
        return bytes(min(255, int(r.expovariate(0.08))) for _ in range(size))
    if kind == "below-4":
        return bytes(r.randrange(4) for _ in range(size))
    if kind == "one-byte":
        return bytes([0x41 + seed % 26]) * size
    if kind == "block-repeated":
        block = r.getrandbits(8 * 32500).to_bytes(32500, "little")
        return (block * (size // 32500 + 1))[:size]
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def corpus_streams():
    """[(name, stream, size)]: the good streams, as zlib wrote them"""
    out = []
    for kind in KINDS:
        for size in SIZES:
            data = data_of(kind, size, len(out))
            for level, strategy in SETTINGS:
                out.append(("%s/%d/level-%d-strategy-%d" % (kind, size, level, strategy), E._deflate(data, level, strategy), size))
    return out


@functools.lru_cache(maxsize=None)
def corpus():
    out = []
    for _, stream, size in corpus_streams():
        flipped = bytearray(stream)
        flipped[len(stream) // 2] ^= 0x10
        for data, cap in ((stream, size), (stream, size - 1), (stream[:2 * len(stream) // 3], size), (bytes(flipped), size)):
            out.append((data, max(cap, 0), len(out) % 16))
    return out


# ---- 3. the window-seam sweep
def rle_cl_seq(lengths):
    """the code lengths spelled with the repeat symbols wherever they fit: [(symbol, extra)]"""
    seq, i = [], 0
    while i < len(lengths):
        v, run = lengths[i], 1
        while i + run < len(lengths) and lengths[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                seq.append((18, k - 11))
                run -= k
            if run >= 3:
                seq.append((17, run - 3))
                run = 0
            seq += [(0, 0)] * run
        else:
            seq.append((v, 0))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                seq.append((16, k - 3))
                run -= k
            seq += [(v, 0)] * run
    return seq


def _probe_codes():
    # literal/length: 97 of one bit, 98 - 101 of four (a repeat 16), then one code each of 3 ... 14 bits and two of 15
    lit = {97: 1, 98: 4, 99: 4, 100: 4, 101: 4}
    for k, s in enumerate([102, 103, 284, 104, 105, 106, 107, 108, 109, 110, 111, 256, 112, 113]):
        lit[s] = min(3 + k, 15)
    lit_lens = E._lens(285, lit)
    dist_lens = E._lens(30, E._ladder([0, 1, 2, 3, 4, 5, 6, 7, 28, 29], 9))
    # the code-length code: all nineteen symbols, two to seven bits
    cl = {18: 2, 4: 3, 16: 3, 17: 4, 0: 4, 1: 4, 3: 4, 2: 5, 5: 5, 6: 5, 7: 5, 8: 5, 9: 6, 10: 6, 11: 6, 14: 6, 15: 6, 12: 7, 13: 7}
    cl_lens = E._lens(19, cl)
    assert C.kraft(lit_lens) == C.kraft(dist_lens) == C.kraft(cl_lens) == 1 << 15
    assert lit_lens[284] == 5 and lit_lens[112] == 15 == lit_lens[113] and dist_lens[28] == 9 == dist_lens[29]
    return lit_lens, dist_lens, cl_lens


PROBE_TOKENS = [98, 112, ("m", 258, 16385 + 5000, 284), 102, ("m", 227 + 9, 24577 + 7000, 284), 113, 97, ("m", 258, 32768 - 300, 284), 103]
# 33 791 bytes for the probe's distances to reach into: 251 random bytes and 130 matches of (258, 251), not one byte
# repeated -- with a period that is prime, a distance that is wrong by any power of two copies other bytes
FRONT = list(E._rand(251, 251)) + [("m", 258, 251)] * 130
FRONT_BYTES = 251 + 130 * 258


def _probe(w):
    lit_lens, dist_lens, cl_lens = _probe_codes()
    C.dynamic(w, PROBE_TOKENS, lit_lens, dist_lens, final=True, cl_lens=cl_lens, cl_seq=rle_cl_seq(lit_lens + dist_lens))


def seam_stream(L, j, seed=0):
    """-> (stream, out_cap, spans of the probe block): the front, a stored block of L random bytes, a fixed block of j
    nine-bit literals (10 + 9 j bits: the probe begins at every bit of a byte), the probe"""
    w = C.Bits()
    C.fixed(w, FRONT)
    C.stored(w, E._rand(L, 1000 * j + L + seed))
    C.fixed(w, [200] * j)
    first = len(w.spans)
    _probe(w)
    return w.bytes(), FRONT_BYTES + L + j + len(C.expand(PROBE_TOKENS, bytes(33000))), w.spans[first:]


@functools.lru_cache(maxsize=None)
def _probe_frame():
    """(bits in front of the probe at L = 0 and j = 0, bits of the probe)"""
    _, _, spans = seam_stream(0, 0)
    start = spans[0][1]
    return start, spans[-1][1] + spans[-1][2] - start


def seam_params():
    """(L, j) such that the seam falls on every bit of the probe, and a few bits in front of it and behind it"""
    start0, bits = _probe_frame()
    out = []
    for j in range(8):
        for L in range(0, WINDOW):
            start = start0 + 8 * L + 9 * j
            if start - 16 <= SEAM <= start + bits + 16:
                out.append((L, j))
    return out


def len_nlen_stream(at, j, seed=0):
    """-> (stream, out_cap, spans): a stored block, a fixed block of j nine-bit literals, and a final stored block of forty
    bytes whose LEN begins at byte `at`"""
    head = (13 + 9 * j + 7) // 8     # the fixed block and the three bits of the last block's header, in whole bytes
    w = C.Bits()
    C.stored(w, E._rand(at - 5 - head, at + j + seed))
    C.fixed(w, [200] * j)
    first = len(w.spans)
    C.stored(w, E._rand(40, 7 * at + j + seed), final=True)
    spans = w.spans[first:]
    assert [s for s in spans if s[0] == "stored-len-nlen"][0][1] == 8 * at
    return w.bytes(), at - 5 - head + j + 40, spans


def _seam_in(spans, kind, bits=None):
    """how the seam meets a field of this kind (and of this many bits): "inside", "begins" or None"""
    for k, at, n in spans:
        if k == kind and (bits is None or bits(n)):
            if at < SEAM < at + n:
                return "inside"
            if at == SEAM:
                return "begins"
    return None


# the field kinds of the sweep: name -> (span kind, a test of the field's width or None)
SEAM_KINDS = {
    "block header": ("block-header", None),
    "the 14-bit counts": ("counts", None),
    "a 3-bit code-length length": ("cl-length", None),
    "a code-length symbol": ("cl-symbol", lambda n: n >= 2),
    "a code-length symbol of 7 bits": ("cl-symbol", lambda n: n == 7),
    "the extra bits of 16": ("cl-extra-16", None),
    "the extra bits of 17": ("cl-extra-17", None),
    "the extra bits of 18": ("cl-extra-18", None),
    "short literal": ("literal", lambda n: 2 <= n <= 10),
    "15-bit literal": ("literal", lambda n: n == 15),
    "length symbol": ("length", None),
    "length extra": ("length-extra", lambda n: n == 5),
    "distance code": ("distance", lambda n: n == 9),
    "13-bit distance extra": ("distance-extra", lambda n: n == 13),
    "end of block": ("end-of-block", None),
    "LEN / NLEN": ("stored-len-nlen", None),
}


@functools.lru_cache(maxsize=None)
def seam_sweep_spans():
    """[(stream, out_cap, spans)] of the two sweeps, whole streams only"""
    out = [seam_stream(L, j) for L, j in seam_params()]
    out += [len_nlen_stream(at, j) for at in range(1020, 1029) for j in range(8)]
    return out


def seam_coverage():
    """{field kind: {"inside", "begins"} met}"""
    seen = {name: set() for name in SEAM_KINDS}
    for _, _, spans in seam_sweep_spans():
        for name, (kind, bits) in SEAM_KINDS.items():
            how = _seam_in(spans, kind, bits)
            if how:
                seen[name].add(how)
    return seen


@functools.lru_cache(maxsize=None)
def seam_sweep():
    out = []
    for stream, cap, _ in seam_sweep_spans():
        out.append((stream, cap, len(out) % 16))
        out.append((stream[:WINDOW], cap, len(out) % 16))
    return out


# ---- 4. the stored-copy matrix
STORED_K = tuple(range(16))
STORED_N = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1031)
STORED_BIG = ((0, 0), (5, 3), (10, 15), (15, 8))   # (k, residue) of the 65 535-byte blocks


def _two_stored(k, n):
    w = C.Bits()
    C.stored(w, E._rand(k, 50 + k))
    C.stored(w, E._rand(n, 100 * n + k), final=True)
    return w.bytes()


@functools.lru_cache(maxsize=None)
def stored_matrix():
    """a first stored block of k bytes puts the second one's bytes at input offset 10 + k; the second holds n bytes"""
    out = []
    for k in STORED_K:
        for n in STORED_N:
            stream = _two_stored(k, n)
            for res in range(16):
                out.append((stream, k + n, res))
                if (k + n + res) % 5 == 0 and k + n:     # a sample with room one short
                    out.append((stream, k + n - 1, res))
    for k, res in STORED_BIG:
        out.append((_two_stored(k, 65535), k + 65535, res))
    k, res = STORED_BIG[1]
    out.append((_two_stored(k, 65535), k + 65534, res))
    return out


# ---- every order of three blocks
def _block(w, kind, k, final):
    tokens = [65 + k, 97 + k, ("m", 4, 2), 48 + k] + ([("m", 5, 3 + k)] if k else [])
    if kind == "stored":
        C.stored(w, E._rand(3 + k, 70 + k), final=final)
        return 3 + k
    if kind == "fixed":
        C.fixed(w, tokens, final=final)
    elif kind == "dynamic-flat":
        C.dynamic(w, tokens, C.FLAT_LIT, C.FLAT_DIST, final=final)
    else:      # codes of two and three bits: what the fixed tables hold reads as other symbols
        lit = E._lens(260, {65 + k: 2, 97 + k: 2, 48 + k: 3, 256: 3, 258: 3, 259: 3})
        C.dynamic(w, tokens, lit, _small_dist(k), final=final)
    return len(C.expand(tokens, bytes(16)))


def _small_dist(k):
    """distance 2 (symbol 1) and distance 3 + k, one bit each"""
    out = [0] * (C.dist_symbol(3 + k)[0] + 1)
    out[1] = out[-1] = 1
    return out


BLOCK_KINDS = ("stored", "fixed", "dynamic-flat", "dynamic-small")


@functools.lru_cache(maxsize=None)
def block_orders():
    """all 64 orders of three blocks of four kinds in one stream (the fixed tables are built once per stream and must be
    built again behind a dynamic block), each with exact room and with room one short"""
    out = []
    for a in BLOCK_KINDS:
        for b in BLOCK_KINDS:
            for c in BLOCK_KINDS:
                w = C.Bits()
                n = _block(w, a, 0, False) + _block(w, b, 1, False) + _block(w, c, 2, True)
                out.append((w.bytes(), n, len(out) % 16))
                out.append((w.bytes(), n - 1, len(out) % 16))
    return out


# ---- 5. mutations
@functools.lru_cache(maxsize=None)
def big_pool():
    """[(stream, size)]: the corpus streams of 2 to 40 KB"""
    return [(stream, size) for _, stream, size in corpus_streams() if 2048 <= len(stream) <= 40 * 1024]


@functools.lru_cache(maxsize=None)
def mutation_lists():
    """(of the small seeds, of the big pool)"""
    small = [(d, c, (7 * k) % 16) for k, (d, c) in enumerate(E.mutations(6000, 31337))]
    big = [(d, c, (11 * k) % 16) for k, (d, c) in enumerate(E.mutations(2000, 4242, pool=big_pool()))]
    return small, big


# ---- 6. ordered pairs on one workgroup
def _case(name):
    return next((data, cap) for n, data, cap, _, _ in E.cases() if n == name)


def _big_dynamic():
    """all 286 literal/length and all 30 distance codes, 15-bit codes in both, and symbols decoded through them"""
    lit_lens = [8] * 232 + [9] * 47 + [10, 11, 12, 13, 14, 15, 15]
    lit_lens[97], lit_lens[285] = lit_lens[285], lit_lens[97]     # 'a' is a 15-bit code
    lit_lens[98], lit_lens[284] = lit_lens[284], lit_lens[98]     # 'b' too
    dist_lens = [15, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6] + [5] * 7 + [4] * 12
    assert len(lit_lens) == 286 and len(dist_lens) == 30 and C.kraft(lit_lens) == C.kraft(dist_lens) == 1 << 15
    tokens = [97, 98, 99, 97, ("m", 3, 1), ("m", 4, 2), 100, ("m", 5, 3), 98, ("m", 6, 9)]
    w = C.Bits()
    C.dynamic(w, tokens, lit_lens, dist_lens, final=True)
    return w.bytes(), len(C.expand(tokens))


def _long_good():
    tokens = list(E._rand(2200, 61, 144))
    return E._fixed(tokens), 2200


PAIR_KINDS = ("fixed", "dynamic-286-30-15-bit", "dynamic-one-literal-code", "stored", "code-lengths-over-subscribed",
              "repeats-run-over-the-lengths", "distances-over-subscribed", "eof-with-literals-pending", "out-cap-with-literals-pending",
              "long-good-stream", "code-lengths-without-any-code")
EMPTY = "empty-input"     # in_len 0 cannot be padded: it sorts behind everything else
PAIR_LENGTHS = (2400, 2320, 2240)


@functools.lru_cache(maxsize=None)
def _pair_item(kind, length):
    """(stream of exactly `length` bytes, out_cap): bytes behind the final block are ignored, and so is what follows a
    defect, so the others are padded behind; a stream that must END early is padded by a stored block in front"""
    pad = lambda data: data + E._rand(length - len(data), length + len(data))
    if kind == "fixed":
        return pad(E._fixed([97, 98, 99, ("m", 5, 3), 100])), 9
    if kind == "dynamic-286-30-15-bit":
        data, cap = _big_dynamic()
        return pad(data), cap
    if kind == "dynamic-one-literal-code":
        return pad(_case("table/one-literal-code-of-length-1:ok")[0]), 0
    if kind == "stored":
        w = C.Bits()
        C.stored(w, E._rand(50, 62), final=True)
        return pad(w.bytes()), 50
    if kind == "code-lengths-over-subscribed":
        return pad(_case("table/code-lengths-over-subscribed:result")[0]), 4
    if kind == "repeats-run-over-the-lengths":
        return pad(_case("table/repeats-run-over-the-lengths:result")[0]), 4
    if kind == "distances-over-subscribed":
        return pad(_case("table/distances-over-subscribed:result")[0]), 4
    if kind == "code-lengths-without-any-code":
        return pad(_case("table/code-lengths-without-any-code:result")[0]), 4
    if kind == "eof-with-literals-pending":
        body = E._fixed(list(range(65, 65 + 20)), final=True)[:12]
        w = C.Bits()
        C.stored(w, E._rand(length - 5 - len(body), 63))
        return w.bytes() + body, length - 5 - len(body) + 20
    if kind == "out-cap-with-literals-pending":
        return pad(E._fixed(list(range(65, 65 + 20)))), 10
    if kind == "long-good-stream":
        data, cap = _long_good()
        assert 2048 < len(data) <= length
        return pad(data), cap
    raise ValueError(kind)


def pair_kinds_at(grid):
    """the kind at every sorted position: three rounds of `grid` padded items -- position p of round one holds kind
    (p // 11) % 11 and of round two kind p % 11, so that the 121 ordered pairs of the eleven kinds lie in front of
    p = 121; round three repeats round one's kinds shifted by one -- and grid + 11 empty inputs behind them"""
    n = len(PAIR_KINDS)
    one = [PAIR_KINDS[(p // n) % n] for p in range(grid)]
    two = [PAIR_KINDS[p % n] for p in range(grid)]
    three = [PAIR_KINDS[((p // n) + 1) % n] for p in range(grid)]
    return one + two + three + [EMPTY] * (grid + n)


def pairs(grid):
    """the items in sorted order (the sort is stable and the lengths fall: the launch keeps this order)"""
    out = []
    for p, kind in enumerate(pair_kinds_at(grid)):
        data, cap = (b"", 3) if kind == EMPTY else _pair_item(kind, PAIR_LENGTHS[p // grid])
        out.append((data, cap, (3 * p) % 16))
    return out


def pairs_met(grid):
    """the ordered pairs (kind, kind behind it in the same LDS) of pairs(grid)"""
    kinds = pair_kinds_at(grid)
    return {(kinds[p], kinds[p + grid]) for p in range(len(kinds) - grid)}


def lds_order(items, grid):
    """the items in the order ONE Wave would meet them if it ran workgroup 0's, then workgroup 1's, ... (for the CPU twins,
    whose one Wave takes the list in order)"""
    return [items[p] for g in range(grid) for p in range(g, len(items), grid)]
