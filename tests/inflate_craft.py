"""A small deflate (RFC 1951) bit writer for tests: stored, fixed and dynamic blocks from token lists, with the code lengths
given explicitly.  zlib never emits a distance above 32 506, a 15-bit code on small inputs, a block type 3 or a broken
header; the edges of a decoder lie there.

Tokens of a fixed or dynamic block:
    65 / b"A"[0]             a literal
    ("m", length, distance)  a match: the usual symbols and extra bits
    ("m", length, distance, lensym)   ... with the length symbol chosen (258 is 285, or 284 with extra bits 31)
    ("lit", symbol)          any literal/length symbol by its code alone (256 in the middle, 286, 287)
    ("len", symbol, extra)   a length symbol and its extra bits, no distance behind it
    ("dist", symbol, extra)  a distance symbol and its extra bits (30, 31 in fixed blocks)
    ("bits", value, n)       n raw bits

Bits.spans lists every field the writers wrote as (kind, first bit, bits) -- fields of no bits left out --, so that a test
can say where in a field a given input bit lies.  The kinds: block-header (BFINAL and BTYPE), stored-pad, stored-len-nlen,
stored-data; counts (HLIT, HDIST and HCLEN together), cl-length, cl-symbol, cl-extra-16 / -17 / -18; literal, length,
length-extra, distance, distance-extra, end-of-block, bits.
"""

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]

FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
# complete sets over the whole alphabets, for dynamic blocks that only want SOME valid code
FLAT_LIT = [8] * 226 + [9] * 60          # 286 symbols: 226 / 256 + 60 / 512 = 1
FLAT_DIST = [4] * 2 + [5] * 28           # 30 symbols: 2 / 16 + 28 / 32 = 1
FLAT_CL = [4] * 13 + [5] * 6             # 19 symbols: 13 / 16 + 6 / 32 = 1


class Bits:
    """spans: [(kind, first bit, bits)] of every field written with a kind (fields of no bits are not listed)"""

    def __init__(self):
        self.acc, self.n, self.out, self.spans = 0, 0, bytearray(), []

    def put(self, value, n, kind=None):
        """n bits of value, least significant first (header fields, extra bits)"""
        assert 0 <= value < (1 << n) or n == 0
        if kind and n:
            self.spans.append((kind, self.bit_len, n))
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n, kind=None):
        """a Huffman code: most significant bit first"""
        self.put(int(format(code, "0%db" % n)[::-1], 2) if n else 0, n, kind)

    def align(self, kind=None):
        if self.n:
            self.put(0, 8 - self.n, kind)

    @property
    def bit_len(self):
        return 8 * len(self.out) + self.n

    def bytes(self, fill=0):
        """the stream; the last byte's spare bits are `fill` (0 or all ones)"""
        if not self.n:
            return bytes(self.out)
        last = self.acc | ((0xFF << self.n) & 0xFF if fill else 0)
        return bytes(self.out) + bytes([last])


def canonical(lengths):
    """{symbol: (code, length)} of the canonical code with these lengths (0: no code)"""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    codes = {}
    for s, l in enumerate(lengths):
        if l:
            codes[s] = (nxt[l], l)
            nxt[l] += 1
    return codes


def kraft(lengths):
    """the sum of 2 ** -length as a fraction of 1 << 15: 1 << 15 is a complete set, more is over-subscribed"""
    return sum(1 << (15 - l) for l in lengths if l)


def len_symbol(length):
    if length == 258:
        return 285, 0
    k = max(i for i in range(28) if LEN_BASE[i] <= length)
    return 257 + k, length - LEN_BASE[k]


def dist_symbol(distance):
    k = max(i for i in range(30) if DIST_BASE[i] <= distance)
    return k, distance - DIST_BASE[k]


def _lit_kind(symbol):
    return "literal" if symbol < 256 else "end-of-block" if symbol == 256 else "length"


def _emit(w, tokens, lit, dist):
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit[t], kind="literal")
        elif t[0] == "m":
            length, distance = t[1], t[2]
            if len(t) > 3:
                ls, lx = t[3], length - LEN_BASE[t[3] - 257]
            else:
                ls, lx = len_symbol(length)
            w.code(*lit[ls], kind="length")
            w.put(lx, LEN_EXTRA[ls - 257], "length-extra")
            ds, dx = dist_symbol(distance)
            w.code(*dist[ds], kind="distance")
            w.put(dx, DIST_EXTRA[ds], "distance-extra")
        elif t[0] == "lit":
            w.code(*lit[t[1]], kind=_lit_kind(t[1]))
        elif t[0] == "len":
            w.code(*lit[t[1]], kind="length")
            w.put(t[2], LEN_EXTRA[t[1] - 257], "length-extra")
        elif t[0] == "dist":
            w.code(*dist[t[1]], kind="distance")
            w.put(t[2], DIST_EXTRA[t[1]] if t[1] < 30 else 0, "distance-extra")
        elif t[0] == "bits":
            w.put(t[1], t[2], "bits")
        else:
            raise ValueError(t)


def stored(w, data, final=False, length=None, nlength=None):
    """a stored block; length / nlength override the two fields"""
    w.put(1 if final else 0, 3, "block-header")   # BFINAL, BTYPE 0
    w.align("stored-pad")
    n = len(data) if length is None else length
    w.put(n | ((n ^ 0xFFFF) if nlength is None else nlength) << 16, 32, "stored-len-nlen")
    at = w.bit_len
    for b in data:
        w.put(b, 8)
    if data:
        w.spans.append(("stored-data", at, 8 * len(data)))


def fixed(w, tokens, final=False, eob=True):
    w.put((1 if final else 0) | 1 << 1, 3, "block-header")
    _emit(w, tokens, canonical(FIXED_LIT), canonical(FIXED_DIST))
    if eob:
        w.code(*canonical(FIXED_LIT)[256], kind="end-of-block")


def plain_cl_seq(lengths):
    """the code lengths one by one, no repeat symbols"""
    return [(l, 0) for l in lengths]


def dynamic(w, tokens, lit_lens, dist_lens, final=False, eob=True, cl_lens=None, cl_seq=None, hlit=None, hdist=None, hclen=None,
            body=True):
    """a dynamic block.  lit_lens / dist_lens: the code lengths (257 ... 286 and 1 ... 30 of them, or what hlit / hdist
    force).  cl_lens: the nineteen lengths of the code-length code (default: a complete set over all of them); cl_seq: the
    (symbol, extra) pairs that spell the lengths (default: one by one); body=False: the header alone"""
    cl_lens = list(FLAT_CL if cl_lens is None else cl_lens)
    cl_seq = plain_cl_seq(list(lit_lens) + list(dist_lens)) if cl_seq is None else cl_seq
    w.put((1 if final else 0) | 2 << 1, 3, "block-header")
    at = w.bit_len
    w.put(len(lit_lens) - 257 if hlit is None else hlit, 5)
    w.put(len(dist_lens) - 1 if hdist is None else hdist, 5)
    order = [cl_lens[s] for s in CL_ORDER]
    n = 19
    while n > 4 and order[n - 1] == 0:
        n -= 1
    n = n if hclen is None else hclen + 4
    w.put(n - 4, 4)
    w.spans.append(("counts", at, 14))
    for l in order[:n]:
        w.put(l, 3, "cl-length")
    cl = canonical(cl_lens)
    for s, x in cl_seq:
        if s in cl:
            w.code(*cl[s], kind="cl-symbol")
        else:
            assert not cl, "symbol %d has no code" % s
            w.put(0, 1, "cl-symbol")  # (a code-length set without any code: a symbol is one bit)
        if s >= 16:
            w.put(x, {16: 2, 17: 3, 18: 7}[s], "cl-extra-%d" % s)
    if not body:
        return
    lit, dist = canonical(lit_lens), canonical(dist_lens)
    _emit(w, tokens, lit, dist)
    if eob:
        w.code(*lit[256], kind="end-of-block")


def expand(tokens, start=b""):
    """what the tokens decode to behind `start` (literals and matches only)"""
    out = bytearray(start)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[1]):
                out.append(out[-t[2]])
    return bytes(out[len(start):])
