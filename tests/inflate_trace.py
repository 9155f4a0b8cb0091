"""A deflate token reader in plain Python, written from RFC 1951: it walks a GOOD raw-deflate stream symbol by symbol and
reports what a decoder meets on the way.  Its only use is to state what the stream lists of tests/inflate_matrix.py cover
(tests/test_inflate_matrix_cpu.py); it decides nothing about right and wrong -- that is zlib's -- and produces no bytes,
only their count, which must be len(zlib's output).

trace(stream) -> dict:
    blocks          [stored, fixed, dynamic] blocks
    order           the block types in stream order (0 stored, 1 fixed, 2 dynamic)
    lit_max, dist_max, cl_max   the longest literal/length, distance and code-length code that was DECODED (dynamic blocks)
    lit_long        literal/length symbols decoded with a code above LIT_FAST bits  (the kernel's first-level table: 10)
    dist_long       distance symbols decoded with a code above DIST_FAST bits       (8)
    dist_far        the greatest distance
    len_258         the matches of 258 bytes
    produced        bytes produced
    used            input bytes used"""
LIT_FAST, DIST_FAST = 10, 8
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
              12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
_CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
_FAST = 10   # the reader's own first-level width, for both alphabets


def _table(lengths):
    """-> (fast, slow): fast[next _FAST bits of the stream] = (symbol, length) for codes of up to _FAST bits; slow[(length,
    code)] = symbol for the longer ones.  Canonical codes, sent most significant bit first"""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    fast, slow = [None] * (1 << _FAST), {}
    for s, l in enumerate(lengths):
        if not l:
            continue
        c = nxt[l]
        nxt[l] += 1
        if l <= _FAST:
            r = int(format(c, "0%db" % l)[::-1], 2)
            for e in range(r, 1 << _FAST, 1 << l):
                fast[e] = (s, l)
        else:
            slow[(l, c)] = s
    return fast, slow


_FIXED = None


def trace(data):
    global _FIXED
    data = bytes(data) + bytes(8)
    pos = 0      # in bits

    def bits(n):
        nonlocal pos
        v = (int.from_bytes(data[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << n) - 1)
        pos += n
        return v

    def symbol(table):
        """-> (symbol, length of its code)"""
        nonlocal pos
        fast, slow = table
        window = int.from_bytes(data[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)
        hit = fast[window & ((1 << _FAST) - 1)]
        if hit:
            pos += hit[1]
            return hit
        code = 0
        for l in range(1, 16):
            code = code << 1 | (window >> (l - 1) & 1)
            if l > _FAST and (l, code) in slow:
                pos += l
                return slow[(l, code)], l
        raise ValueError("no code at bit %d" % pos)

    t = {"blocks": [0, 0, 0], "order": [], "lit_max": 0, "dist_max": 0, "cl_max": 0, "lit_long": 0, "dist_long": 0, "dist_far": 0, "len_258": 0,
         "produced": 0, "used": 0}
    produced = 0
    last = 0
    while not last:
        last, kind = bits(1), bits(2)
        t["blocks"][kind] += 1          # (kind 3: an IndexError -- the reader is for good streams)
        t["order"].append(kind)
        if kind == 0:
            pos = (pos + 7) & ~7
            n, inv = bits(16), bits(16)
            assert n == inv ^ 0xFFFF
            pos += 8 * n
            produced += n
            continue
        if kind == 1:
            if _FIXED is None:
                _FIXED = _table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _table([5] * 32)
            lit, dist = _FIXED
        else:
            nlit, ndist, ncl = bits(5) + 257, bits(5) + 1, bits(4) + 4
            cl = [0] * 19
            for i in range(ncl):
                cl[_CL_ORDER[i]] = bits(3)
            clt = _table(cl)
            lens = []
            while len(lens) < nlit + ndist:
                s, l = symbol(clt)
                t["cl_max"] = max(t["cl_max"], l)
                if s < 16:
                    lens.append(s)
                elif s == 16:
                    lens += [lens[-1]] * (3 + bits(2))
                elif s == 17:
                    lens += [0] * (3 + bits(3))
                else:
                    lens += [0] * (11 + bits(7))
            assert len(lens) == nlit + ndist
            lit, dist = _table(lens[:nlit]), _table(lens[nlit:])
        dynamic = kind == 2
        lit_long = dist_long = lit_max = dist_max = 0
        while True:
            s, l = symbol(lit)
            if l > LIT_FAST:
                lit_long += 1
            if l > lit_max:
                lit_max = l
            if s < 256:
                produced += 1
                continue
            if s == 256:
                break
            n = _LEN_BASE[s - 257] + bits(_LEN_EXTRA[s - 257])
            ds, l = symbol(dist)
            if l > DIST_FAST:
                dist_long += 1
            if l > dist_max:
                dist_max = l
            distance = _DIST_BASE[ds] + bits(_DIST_EXTRA[ds])
            assert distance <= produced
            if distance > t["dist_far"]:
                t["dist_far"] = distance
            if n == 258:
                t["len_258"] += 1
            produced += n
        t["lit_long"] += lit_long
        t["dist_long"] += dist_long
        if dynamic:
            t["lit_max"], t["dist_max"] = max(t["lit_max"], lit_max), max(t["dist_max"], dist_max)
    t["produced"], t["used"] = produced, (pos + 7) >> 3
    return t
