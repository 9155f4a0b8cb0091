"""BCJ2 (7-Zip method 03 03 01 1B) in Python, written from the description: the encoder that makes the test streams and
the serial decoder they are judged by (which libarchive, through `cmake -E tar xf`, confirms: tests/test_bcj2_cpu.py).
A plain module, not a conftest.

  IsJ(prev, b) = (b & 0xFE) == 0xE8 or (prev == 0x0F and (b & 0xF0) == 0x80)
  range coder: LZMA's, 11-bit probabilities from 1024, move 5 bits, top 1 << 24; 258 probabilities: [prev] for E8, [256]
  for E9, [257] for 0F 8x.
The encoder converts a candidate when four bytes follow it and the operand's top byte is 00 or FF (a near branch);
otherwise it encodes bit 0.  It encodes no bit for a candidate that is the last byte."""
OK, ERR_RESULT = 0, -1
TOP = 1 << 24


def is_j(prev, b):
    return (b & 0xFE) == 0xE8 or (prev == 0x0F and (b & 0xF0) == 0x80)


def prob_index(prev, b):
    return prev if b == 0xE8 else 256 if b == 0xE9 else 257


class _RangeEncoder:
    def __init__(self):
        self.low, self.range, self.cache, self.cache_size, self.out = 0, 0xFFFFFFFF, 0, 1, bytearray()

    def _shift_low(self):
        if self.low < 0xFF000000 or self.low >= 1 << 32:
            carry = self.low >> 32
            c = self.cache
            while True:
                self.out.append((c + carry) & 0xFF)
                c = 0xFF
                self.cache_size -= 1
                if not self.cache_size:
                    break
            self.cache = (self.low >> 24) & 0xFF
        self.cache_size += 1
        self.low = (self.low & 0x00FFFFFF) << 8

    def bit(self, probs, i, bit):
        p = probs[i]
        bound = (self.range >> 11) * p
        if not bit:
            self.range = bound
            probs[i] = p + ((2048 - p) >> 5)
        else:
            self.low += bound
            self.range -= bound
            probs[i] = p - (p >> 5)
        while self.range < TOP:
            self.range = (self.range << 8) & 0xFFFFFFFF
            self._shift_low()

    def finish(self):
        for _ in range(5):
            self._shift_low()
        return bytes(self.out)


def encode(data, convert=None):
    """-> (main, call, jump, rc).  convert(i, rel): overrides the choice for the candidate at data[i] with four bytes behind
    it (rel = its little-endian operand)."""
    data = bytes(data)
    n = len(data)
    main, call, jump = bytearray(), bytearray(), bytearray()
    rc, probs = _RangeEncoder(), [1024] * 258
    prev, i = 0, 0
    while i < n:
        b = data[i]
        main.append(b)
        i += 1
        if not is_j(prev, b):
            prev = b
            continue
        if i == n:
            break
        idx = prob_index(prev, b)
        if n - i >= 4:
            rel = int.from_bytes(data[i:i + 4], "little")
            take = (rel >> 24) in (0x00, 0xFF) if convert is None else convert(i - 1, rel)
            if take:
                rc.bit(probs, idx, 1)
                (call if b == 0xE8 else jump).extend(((rel + i + 4) & 0xFFFFFFFF).to_bytes(4, "big"))
                i += 4
                prev = rel >> 24
                continue
        rc.bit(probs, idx, 0)
        prev = b
    return bytes(main), bytes(call), bytes(jump), rc.finish()


def decode(main, call, jump, rc, out_len):
    """-> (status, bytes produced)"""
    out = bytearray()
    if out_len == 0:
        return OK, b""
    if len(rc) < 5:
        return ERR_RESULT, b""
    probs = [1024] * 258
    code, rng, rp = int.from_bytes(rc[1:5], "big"), 0xFFFFFFFF, 5
    prev = mp = cp = jp = 0
    st = OK
    while True:
        cand, b = False, 0
        while mp < len(main) and len(out) < out_len:
            b = main[mp]
            mp += 1
            out.append(b)
            if is_j(prev, b):
                cand = True
                break
            prev = b
        if not cand or len(out) == out_len:
            break
        i = prob_index(prev, b)
        p = probs[i]
        bound = (rng >> 11) * p
        bit = code >= bound
        if not bit:
            rng = bound
            probs[i] = p + ((2048 - p) >> 5)
        else:
            rng -= bound
            code -= bound
            probs[i] = p - (p >> 5)
        if rng < TOP:
            if rp == len(rc):
                st = ERR_RESULT
                break
            rng = (rng << 8) & 0xFFFFFFFF
            code = ((code << 8) | rc[rp]) & 0xFFFFFFFF
            rp += 1
        if not bit:
            prev = b
            continue
        if b == 0xE8:
            if len(call) - cp < 4:
                st = ERR_RESULT
                break
            src = int.from_bytes(call[cp:cp + 4], "big")
            cp += 4
        else:
            if len(jump) - jp < 4:
                st = ERR_RESULT
                break
            src = int.from_bytes(jump[jp:jp + 4], "big")
            jp += 4
        dest = (src - (len(out) + 4)) & 0xFFFFFFFF
        out += dest.to_bytes(4, "little")[:out_len - len(out)]
        if len(out) == out_len:
            break
        prev = dest >> 24
    return (OK if st == OK and len(out) == out_len else ERR_RESULT), bytes(out)


def convert_0f_too(i, rel):
    """a `convert` that also takes operands whose top byte is 0F: what makes the prev trap"""
    return (rel >> 24) in (0x00, 0xFF, 0x0F)


def trap_data(lead, tail=40):
    """`lead` plain bytes, then E8 with an operand whose top byte is 0F, then 80 + an operand, then `tail` plain bytes: with
    convert_0f_too the 80 is a candidate only because prev = dest >> 24 = 0F (the byte in front of it in the MAIN stream
    is the E8).  -> (data, index of the E8)"""
    body = bytes([0xE8, 0x11, 0x22, 0x33, 0x0F, 0x80, 0x44, 0x55, 0x66, 0x00])
    return bytes((7 * k + 1) % 0xE0 for k in range(lead)) + body + bytes((5 * k + 3) % 0xE0 for k in range(tail)), lead
