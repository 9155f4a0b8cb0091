"""A small bzip2 WRITER for tests (test infrastructure, like tests/lzma_craft.py): a naive rotation sort on small inputs,
with the choices a test wants -- level, nGroups, selectors, code lengths up to 20, origPtr, how runs are split -- and the
defects a decoder must refuse.  Written from the format's public description (lzma_amd/csrc/xlz_bz2_dev.h has it).

    stream([block(data), ...], level=1) -> bytes

Every valid crafted file decompresses under Python's bz2 to the intended bytes and every defect is refused by it:
tests/test_bz2_cpu.py asserts both, so the case list bites by the yardstick alone."""
import heapq

BLOCK_MAGIC, END_MAGIC = 0x314159265359, 0x177245385090


def crc32_bzip2(data, crc=0):
    """bit by bit: polynomial 0x04C11DB7, not reflected"""
    r = crc ^ 0xFFFFFFFF
    for b in data:
        r ^= b << 24
        for _ in range(8):
            r = ((r << 1) ^ 0x04C11DB7) & 0xFFFFFFFF if r & 0x80000000 else (r << 1) & 0xFFFFFFFF
    return r ^ 0xFFFFFFFF


class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, nbits):
        assert 0 <= value < (1 << nbits) or nbits == 0
        self.v = (self.v << nbits) | value
        self.n += nbits

    def extend(self, other):
        self.put(other.v, other.n)

    def bytes(self):
        pad = -self.n % 8
        return ((self.v << pad).to_bytes((self.n + pad) // 8, "big")) if self.n else b""


def rle1(data, max_run=255):
    """the first-stage run-length code: four equal bytes, then a count of up to max_run - 4 further ones (max_run >= 4;
    255 is what encoders write, 4 splits every run into fours with a count of 0)"""
    out, i = bytearray(), 0
    while i < len(data):
        j = i
        while j < len(data) and data[j] == data[i] and j - i < max_run:
            j += 1
        n = j - i
        out += data[i:i + min(n, 4)]
        if n >= 4:
            out.append(n - 4)
        i = j
    return bytes(out)


def unrle1(pre):
    """what the run-length stage makes of `pre`"""
    out, run, last = bytearray(), 0, None
    for x in pre:
        if run == 4:
            out += bytes([last]) * x
            run = 0
        elif run and x == last:
            run += 1
            out.append(x)
        else:
            last, run = x, 1
            out.append(x)
    return bytes(out)


def bwt(s):
    n = len(s)
    rows = sorted(range(n), key=lambda i: s[i:] + s[:i])
    return bytes(s[(i - 1) % n] for i in rows), rows.index(0)


def unbwt(last, orig):
    """the bytes whose last column and origPtr these are (any orig below len(last) gives some)"""
    n = len(last)
    tt = sorted(range(n), key=lambda i: last[i])  # (stable: the counting sort)
    out, p = bytearray(), tt[orig]
    for _ in range(n):
        out.append(last[p])
        p = tt[p]
    return bytes(out)


def symbols(last):
    """the move-to-front / RUNA-RUNB symbols of a last column -> (symbols with the end symbol, the used bytes)"""
    used = sorted(set(last))
    mtf, syms, run = list(range(len(used))), [], 0

    def flush():
        nonlocal run
        while run:  # bijective base 2, least digit first
            syms.append((run - 1) & 1)
            run = (run - 1) >> 1

    for b in last:
        k = mtf.index(used.index(b))
        if k == 0:
            run += 1
            continue
        flush()
        syms.append(k + 1)
        mtf.insert(0, mtf.pop(k))
    flush()
    syms.append(len(used) + 1)
    return syms, used


def huffman_lengths(freq, limit=17):
    """code lengths of an optimal code (every symbol gets one), flat if it came out deeper than `limit`"""
    n = len(freq)
    heap = [(f + 1, i, (i,)) for i, f in enumerate(freq)]
    heapq.heapify(heap)
    lens = [0] * n
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for i in a[2] + b[2]:
            lens[i] += 1
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    if max(lens) > limit or n == 1:
        lens = [max(1, (n - 1).bit_length())] * n
    return lens


def deep_lengths(n, deep=(0, 1)):
    """a legal (incomplete) code with two symbols at length 20: the others flat, one bit above what they need"""
    flat = max(1, (n - 1).bit_length()) + 1
    return [20 if i in deep else flat for i in range(n)]


def canonical(lens):
    codes, code = {}, 0
    for l in range(1, 21):
        for s, x in enumerate(lens):
            if x == l:
                codes[s] = (code, l)
                code += 1
        code <<= 1
    return codes


def block(data, n_groups=2, deep=False, selectors=None, max_run=255, orig=None, defect=None, pre=None, column=None):
    """one block of `data` (not empty) -> Bits.  n_groups 2..6 tables, used in turn (selectors: a list of table numbers, one
    per 50 symbols, instead); deep: codes of length 20, other symbols deep in every table; orig: the origPtr field
    instead of the true one; pre: the bytes behind the run-length stage instead of rle1(data, max_run); column: (last column,
    origPtr) instead of a sort -- a successor vector made to order.
    defect: "orig" (origPtr = nblock), "groups1", "groups7", "selectors0", "len0", "len21", "empty_map", "crc", "random"."""
    if column is not None:  # (last column, origPtr) as given: data is then what they decode to, whatever was passed
        last, true_orig = column
        data = unrle1(unbwt(last, true_orig))
    else:
        pre = rle1(data, max_run) if pre is None else pre
        last, true_orig = bwt(pre)
    syms, used = symbols(last)
    alpha = len(used) + 2
    freq = [0] * alpha
    for s in syms:
        freq[s] += 1
    tables = []
    for t in range(n_groups):
        tables.append(deep_lengths(alpha, ((2 * t) % alpha, (2 * t + 1) % alpha)) if deep else huffman_lengths(freq))
    n_sel = (len(syms) + 49) // 50
    sel = list(selectors) if selectors is not None else [i % n_groups for i in range(n_sel)]
    assert len(sel) >= n_sel and all(0 <= s < n_groups for s in sel)
    w = Bits()
    w.put(BLOCK_MAGIC, 48)
    w.put(crc32_bzip2(data) ^ (0x5A5A5A5A if defect == "crc" else 0), 32)
    w.put(1 if defect == "random" else 0, 1)
    w.put(len(last) if defect == "orig" else true_orig if orig is None else orig, 24)
    if defect == "empty_map":
        w.put(0, 16)
    else:
        w.put(sum(0x8000 >> i for i in range(16) if any(b >> 4 == i for b in used)), 16)
        for i in range(16):
            if any(b >> 4 == i for b in used):
                w.put(sum(0x8000 >> j for j in range(16) if 16 * i + j in used), 16)
    w.put({"groups1": 1, "groups7": 7}.get(defect, n_groups), 3)
    w.put(0 if defect == "selectors0" else len(sel), 15)
    order = list(range(n_groups))
    for s in sel:
        k = order.index(s)
        w.put((1 << (k + 1)) - 2, k + 1)  # k ones and a zero
        order.insert(0, order.pop(k))
    for t, lens in enumerate(tables):
        curr = lens[0]
        w.put({"len0": 0, "len21": 21}.get(defect, curr) if t == 0 else curr, 5)
        for x in lens:
            while curr < x:
                w.put(0b10, 2)
                curr += 1
            while curr > x:
                w.put(0b11, 2)
                curr -= 1
            w.put(0, 1)
    codes = [canonical(lens) for lens in tables]
    for i, s in enumerate(syms):
        code, l = codes[sel[i // 50]][s]
        w.put(code, l)
    return w


def long_run_block(byte, run, n_groups=2):
    """a block that is ONE run of `run` copies of `byte` in its last column (the longest RUNA/RUNB number there is when run
    fills the block; a run past the block size when it does not fit): -> (Bits, the bytes it decodes to)"""
    pre = bytes([byte]) * run
    data, i = bytearray(), 0
    while i < run:  # what the run-length stage makes of them: four bytes, then a count that is the byte itself
        take = min(4, run - i)
        data += bytes([byte]) * take
        i += take
        if take == 4 and i < run:
            data += bytes([byte]) * byte
            i += 1
    syms, n = [], run
    while n:
        syms.append((n - 1) & 1)
        n = (n - 1) >> 1
    syms.append(2)
    w = Bits()
    w.put(BLOCK_MAGIC, 48)
    w.put(crc32_bzip2(bytes(data)), 32)
    w.put(0, 1)
    w.put(0, 24)
    w.put(0x8000 >> (byte >> 4), 16)
    w.put(0x8000 >> (byte & 15), 16)
    w.put(n_groups, 3)
    w.put(1, 15)
    w.put(0, 1)
    for _ in range(n_groups):
        w.put(2, 5)
        for _ in range(3):
            w.put(0, 1)
    for s in syms:
        w.put(s, 2)
    return w, bytes(data)


def stream(blocks, level=1, datas=None, defect=None):
    """"BZh" + level, the blocks (Bits, as block() makes them), the end magic and the combined CRC -> bytes.  The combined
    CRC is formed from the CRC fields of the blocks as they are written.  defect: "combined" (a wrong combined CRC)."""
    w = Bits()
    for c in b"BZh" + bytes([ord("0") + level]):
        w.put(c, 8)
    combined = 0
    for b in blocks:
        stored = (b.v >> (b.n - 80)) & 0xFFFFFFFF
        combined = (((combined << 1) | (combined >> 31)) & 0xFFFFFFFF) ^ stored
        w.extend(b)
    w.put(END_MAGIC, 48)
    w.put(combined ^ (1 if defect == "combined" else 0), 32)
    return w.bytes()
