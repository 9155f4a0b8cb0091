"""Crafted inputs for the BCJ2 merge kernel (lzma_amd/csrc/xlz_bcj2_dev.hip, its scheme in xlz_bcj2_dev.h): streams that sit
ON the seams of its work split -- the 16-byte lane, the window of W = 1024 main bytes, the 16-byte lines the rc / call /
jump streams are read in, the head / chunks / tail of a window's store and the trips of its chunk loop (a window's image
holds up to 5 * W bytes: 64 to 320 chunks of sixteen) -- and, in rounds(n), many tiny items of mixed kinds, so that one
workgroup merges several items in turn, a good one behind a failed one.  The streams are made by tests/bcj2_ref.py's
encoder with a `convert` callback and judged by its serial decoder; tests/test_bcj2_edges_cpu.py shows with the reference
alone that every case bites, tests/test_gpu_bcj2_edges.py puts the cases through one launch.  A plain module, not a
conftest.

cases(family=None) -> [(name, (main, call, jump, rc), out_len, probe)].  A name ends in "@rN": N is the residue modulo 16 of
the destination the case wants.  probe(status, out) -- the reference's verdict on the case -- asserts what the case exists
for and returns the facts a family is counted by (a dict, maybe empty).  Everything is seeded.

The families:
  residue  one dense stream, out_len 0..40 x residue 0..15: every head / chunk / tail shape of a small window's store
  chunks   one window whose output has 63, 64, 65, 128, 129, 192, 193, 256, 257 or 320 chunks at residue 0, 1 or 15, as far
           as a window can: 320 chunks are the full image at residue 0 (every byte a converted E8; 319 is the most a
           destination that is no multiple of 16 leaves), and 63 at residue 0 takes a last window of 1008 bytes
  chain    a chain of prev traps: E8 .. .. .. 0F, then 300 x (8x .. .. .. 0F), all converted: the main stream shows ONE
           candidate, the other 300 exist only through prev = dest >> 24.  It crosses some twenty lane seams at every lead,
           and a window seam at the leads from 1008 on
  cuts     1100 x (E8 00 00 00 00), all converted, with out_len round 0, round the seam of the first two windows' outputs
           (5120) and round the end; a mixed stream with out_len round the output position of its second window seam
  lines    a 6000-byte input whose conversions alternate pseudo-randomly: whole, with rc of every length 4..69, with call and
           with jump cut at every length 0..79 -- a side stream's end at every position of a 16-byte line
  seam     an opcode as the last byte of a window (E8, E9, and 0F with its 8x as the next window's first byte), converted
           and not, at the first and the second window seam; and the two cases tests/test_gpu_bcj2.py has"""
import functools
import random
import re

import bcj2_ref as B

W, LANE, IMAGE = 1024, 16, 5 * 1024
FAMILIES = ("residue", "chunks", "chain", "cuts", "lines", "seam")
CHUNK_COUNTS = (63, 64, 65, 128, 129, 192, 193, 256, 257, 320)
CHUNK_RESIDUES = (0, 1, 15)
CHAIN_LEADS = (0, 3, 14, 15, 16, 1008, 1022, 1023, 1024, 2047)
CHAIN_LINKS = 300
ROUND_KINDS = ("dense", "quiet", "call-cut", "no-room", "no-main", "two-windows", "trap")
ROUND_VARIANTS = 37


def plain(n, k0=0):
    return bytes((7 * (k + k0) + 1) % 0xE0 for k in range(n))   # no E8 / E9, no 0F 8x


def always(i, rel):
    return True


def never(i, rel):
    return False


def residue(name):
    return int(re.search(r"@r(\d+)$", name).group(1))


def store_shape(n, res):
    """wave_store restated: a window's n output bytes to a destination at `res` modulo 16 -> (head, chunks, tail, trips)"""
    head = min((16 - res) % 16, n)
    chunks = (n - head) // 16
    return head, chunks, n - head - 16 * chunks, -(-chunks // 64)


def main_candidates(main):
    """the positions the mark phase finds: candidates by the main stream's own bytes (prev = 0 in front of the first)"""
    return [i for i, b in enumerate(main) if B.is_j(main[i - 1] if i else 0, b)]


def out_positions(data, convert=None):
    """the encoder's walk restated -> per main byte the position of that byte in the output"""
    n, pos, prev, i = len(data), [], 0, 0
    while i < n:
        b = data[i]
        pos.append(i)
        i += 1
        if not B.is_j(prev, b):
            prev = b
            continue
        if i == n:
            break
        if n - i >= 4:
            rel = int.from_bytes(data[i:i + 4], "little")
            if (rel >> 24) in (0x00, 0xFF) if convert is None else convert(i - 1, rel):
                i += 4
                prev = rel >> 24
                continue
        prev = b
    return pos


def _prefix_probe(data, n, **facts):
    def probe(st, out):
        assert st == B.OK and out == data[:n] and len(out) == n
        return dict(facts)
    return probe


# ---- residue -----------------------------------------------------------------------------------------------------------------
DENSE40 = (b"\xE8\x10\x00\x00\x00" b"\x41" b"\x0F\x84\x20\x00\x00\x00" b"\xE9\x30\x00\x00\xFF" b"\x42\x43" b"\xE8\x05\x06\x07\x08"
           b"\xE8\x11\x22\x33\x0F\x80\x44\x55\x66\x00" b"\x0F\x44" b"\xE9\xE8\x01\x00\x00\x00" b"\x45\x46\x47\x48")


def _residue_cases(out):
    data = DENSE40
    st4 = B.encode(data, B.convert_0f_too)
    pos = out_positions(data, B.convert_0f_too)
    assert len(data) >= 45 and len(st4[1]) >= 8 and len(st4[2]) >= 12 and len(main_candidates(st4[0])) < (len(data) - len(st4[0])) // 4 + 1
    assert sum(p < 40 for p in pos) <= 40 - 4 * 5   # five conversions and more in the first 40 output bytes, one of them trapped
    for n in range(41):
        for r in range(16):
            head, chunks, tail, _ = store_shape(n, r)
            out.append(("residue/len%d@r%d" % (n, r), st4, n, _prefix_probe(data, n, shape=(head > 0, chunks, tail > 0))))


# ---- chunks ------------------------------------------------------------------------------------------------------------------
def _window(m, k, seed):
    """one window: m main bytes, k of them converted E8 / E9 -> the data (m + 4k bytes)"""
    rnd = random.Random(seed)
    conv = set(rnd.sample(range(m), k))
    v = bytearray()
    for i in range(m):
        if i in conv:
            v += bytes([0xE8 if rnd.randrange(3) else 0xE9, rnd.randrange(1, 0xE0), rnd.randrange(0xE0), rnd.randrange(0xE0), 0x00])
        else:
            v.append((7 * i + 1) % 0xE0)
    return bytes(v)


def _chunks_cases(out):
    for c in CHUNK_COUNTS:
        for r in CHUNK_RESIDUES:
            head = (16 - r) % 16
            if head + 16 * c > IMAGE:
                continue                    # 320 chunks: the full image, at residue 0 alone
            tail = next(t for t in ((5 * c + r + d) % 16 for d in range(16)) if (head + 16 * c + t) % 4 == 0 and head + 16 * c + t <= IMAGE)
            n = head + 16 * c + tail
            m = W if n >= W else n - 4      # (63 chunks at residue 0: a last window of some 1004 bytes, one of them converted)
            k = (n - m) // 4
            data = b"\xE8\x00\x00\x00\x00" * W if n == IMAGE else _window(m, k, 9000 + 16 * c + r)
            st4 = B.encode(data, always)
            assert len(data) == n == m + 4 * k and len(st4[0]) == m <= W and len(st4[1]) + len(st4[2]) == 4 * k, (c, r, n, m, k)

            def probe(st, got, data=data, n=n, r=r, c=c):
                assert st == B.OK and got == data
                head, chunks, tail, trips = store_shape(n, r)
                assert chunks == c and head == (16 - r) % 16 and head + 16 * chunks + tail == n
                return {"chunks": chunks, "trips": trips, "full": n == IMAGE}
            out.append(("chunks/c%d/n%d@r%d" % (c, n, r), st4, n, probe))


# ---- chain -------------------------------------------------------------------------------------------------------------------
def _chain_cases(out):
    for q, lead in enumerate(CHAIN_LEADS):
        rnd = random.Random(9100 + lead)
        v = bytearray(plain(lead)) + bytes([0xE8, rnd.randrange(256), rnd.randrange(256), rnd.randrange(256), 0x0F])
        for _ in range(CHAIN_LINKS):
            v += bytes([0x80 | rnd.randrange(16), rnd.randrange(256), rnd.randrange(256), rnd.randrange(256), 0x0F])
        v += plain(40)
        data = bytes(v)
        st4 = B.encode(data, always)

        def probe(st, got, data=data, st4=st4, lead=lead):
            assert st == B.OK and got == data
            main, call, jump, _ = st4
            assert main_candidates(main) == [lead]                      # the main stream alone shows the E8 and nothing else
            assert len(call) == 4 and len(jump) == 4 * CHAIN_LINKS      # ... and 301 candidates were converted
            assert len(main) == lead + 1 + CHAIN_LINKS + 40
            first, last = lead, lead + CHAIN_LINKS
            return {"lane_seams": last // LANE - first // LANE, "window_seam": last // W > first // W,
                    "trap_opens_a_window": any((p + 1) % W == 0 for p in range(first, last))}
        out.append(("chain/lead%d@r%d" % (lead, (5 * q + 2) % 16), st4, len(data), probe))


# ---- cuts --------------------------------------------------------------------------------------------------------------------
def mixed_stream():
    """4000 bytes with E8 / E9 / 0F 8x at every few bytes, near and far operands: its second window seam lies inside"""
    rnd = random.Random(9200)
    v = bytearray()
    while len(v) < 4000:
        kind = rnd.randrange(6)
        if kind < 3:
            v += plain(rnd.randrange(1, 9), len(v))
        else:
            v += (b"\xE8", b"\xE9", bytes([0x0F, 0x80 | rnd.randrange(16)]))[kind - 3]
            v += bytes([rnd.randrange(256), rnd.randrange(256), rnd.randrange(256), rnd.choice((0x00, 0xFF, 0x0F, 0x37))])
    return bytes(v[:4000])


def _cuts_cases(out):
    data = b"\xE8\x00\x00\x00\x00" * 1100
    st4 = B.encode(data)
    assert len(st4[0]) == 1100 and len(st4[1]) == 4400 and not st4[2]
    for q, n in enumerate(list(range(40)) + list(range(5100, 5140)) + list(range(5490, 5500))):
        # n % 5: 1 a candidate as the last output byte (no bit), 2 - 4 an operand cut after one to three bytes
        out.append(("cuts/e8/len%d@r%d" % (n, (3 * q + 1) % 16), st4, n, _prefix_probe(data, n, phase=n % 5, at_seam=abs(n - IMAGE) <= 4)))
    data = mixed_stream()
    st4 = B.encode(data, B.convert_0f_too)
    pos = out_positions(data, B.convert_0f_too)
    assert len(pos) == len(st4[0]) > 2 * W and len(st4[1]) >= 200 and len(st4[2]) >= 200
    seam = pos[2 * W]
    for q, n in enumerate(range(seam - 20, seam + 20)):
        out.append(("cuts/mixed/len%d@r%d" % (n, (7 * q) % 16), st4, n, _prefix_probe(data, n, seam=seam)))


# ---- lines -------------------------------------------------------------------------------------------------------------------
def _lines_input(seed):
    rnd = random.Random(seed)
    v = bytearray()
    while len(v) < 6000:
        kind = rnd.randrange(4)
        v += (b"\xE8", b"\xE8", b"\xE9", bytes([0x0F, 0x80 | rnd.randrange(16)]))[kind]
        v += bytes([rnd.randrange(1, 0xE0), rnd.randrange(0xE0), rnd.randrange(0xE0), 0x00])
        v += plain(rnd.randrange(4, 10), len(v))
    return bytes(v[:6000])


@functools.lru_cache(None)
def lines_streams():
    """the `lines` input and its streams: the first seed that gives an rc stream of 64 to 69 bytes -- so that its end, and
    the end of what the decoder reads of it, fall among the lengths 4..69 -- and 500 bytes and more of call and of jump"""
    for seed in range(9300, 9400):
        data = _lines_input(seed)
        choice = random.Random(seed + 1000)
        st4 = B.encode(data, lambda i, rel: choice.randrange(2) == 1)
        if 64 <= len(st4[3]) <= 69 and len(st4[1]) >= 500 and len(st4[2]) >= 500:
            return data, st4
    raise AssertionError("no seed gives the lines input")


def _lines_cases(out):
    data, st4 = lines_streams()
    main, call, jump, rc = st4
    assert len(data) == 6000 and len(rc) >= 64 and len(call) >= 500 and len(jump) >= 500

    def probe_of(what, want):
        def probe(st, got):
            assert want is None or st == want, (what, st)
            assert st != B.OK or got == data
            return {what: st}
        return probe
    out.append(("lines/whole@r4", st4, len(data), probe_of("whole", B.OK)))
    for n in range(4, 70):     # (behind its end the stream goes on with bytes the decoder never asks for)
        out.append(("lines/rc%d@r%d" % (n, (n * 5) % 16), (main, call, jump, (rc + bytes([0xEE]) * 8)[:n]), len(data), probe_of("rc", None)))
    for n in range(80):
        out.append(("lines/call%d@r%d" % (n, (n * 3 + 1) % 16), (main, call[:n], jump, rc), len(data), probe_of("call", B.ERR_RESULT)))
        out.append(("lines/jump%d@r%d" % (n, (n * 7 + 2) % 16), (main, call, jump[:n], rc), len(data), probe_of("jump", B.ERR_RESULT)))


# ---- seam --------------------------------------------------------------------------------------------------------------------
def _seam_cases(out):
    q = 0
    for window in (1, 2):
        for tag, op in (("e8", b"\xE8"), ("e9", b"\xE9"), ("0f8x", b"\x0F\x85")):
            for converted in (True, False):
                lead = window * W - 1      # the opcode, or the 0F, is the window's last byte
                data = plain(lead) + op + b"\x10\x20\x30\x00" + plain(30, 3)
                st4 = B.encode(data, always if converted else never)

                def probe(st, got, data=data, st4=st4, lead=lead, op=op, converted=converted):
                    assert st == B.OK and got == data
                    main = st4[0]
                    assert main[:lead] == data[:lead] and main[lead] == op[0] and (lead + 1) % W == 0
                    assert main_candidates(main) == [lead + len(op) - 1]
                    assert len(st4[1]) + len(st4[2]) == (4 if converted else 0)
                    assert len(op) == 1 or (main[lead + 1] & 0xF0) == 0x80
                    return {"converted": converted}
                out.append(("seam/%s/%s/window%d@r%d" % (tag, "converted" if converted else "kept", window, (5 * q + 3) % 16), st4, len(data), probe))
                q += 1
    for tag, data in (("kept-from-test_gpu_bcj2/e8", plain(1023) + b"\xE8\x10\x00\x00\x00" + plain(300)),
                      ("kept-from-test_gpu_bcj2/e9", plain(1024 + 1023) + b"\xE9\x10\x00\x00\xFF" + plain(30))):
        out.append(("seam/%s@r%d" % (tag, (5 * q + 3) % 16), B.encode(data), len(data), _prefix_probe(data, len(data), converted=True)))
        q += 1


_BUILDERS = {"residue": _residue_cases, "chunks": _chunks_cases, "chain": _chain_cases, "cuts": _cuts_cases, "lines": _lines_cases,
             "seam": _seam_cases}


@functools.lru_cache(None)
def _family(name):
    out = []
    _BUILDERS[name](out)
    assert all(c[0].startswith(name + "/") for c in out) and len({c[0] for c in out}) == len(out)
    return tuple(out)


def cases(family=None):
    return [c for f in FAMILIES if family in (None, f) for c in _family(f)]


def family(case):
    return case[0].split("/")[0]


# ---- rounds ------------------------------------------------------------------------------------------------------------------
def _dense(rnd, n):
    v = bytearray()
    while len(v) < n:
        kind = rnd.randrange(5)
        if kind < 2:
            v.append(rnd.randrange(0xE0) if rnd.randrange(4) else 0x0F)
        else:
            v += (b"\xE8", b"\xE9", bytes([0x0F, 0x80 | rnd.randrange(16)]))[kind - 2]
            v += bytes([rnd.randrange(256), rnd.randrange(256), rnd.randrange(256), rnd.choice((0x00, 0xFF))])
    return bytes(v[:n])


@functools.lru_cache(None)
def _round_item(kind, variant):
    """-> (the four streams, out_len, the data when the item is good, else None)"""
    rnd = random.Random(9500 + 100 * kind + variant)
    n = rnd.randrange(5, 61)
    what = ROUND_KINDS[kind]
    if what == "dense":
        data = b"\xE8\x01\x00\x00\x00" + _dense(rnd, n - 5)
        return B.encode(data), n, data
    if what == "quiet":
        data = plain(n, variant)
        return B.encode(data), n, data
    if what == "call-cut":      # the call stream ends inside the word of the item's last call
        data = _dense(rnd, max(n - 10, 0)) + plain(min(n - 5, 5), variant) + b"\xE8\x02\x00\x00\x00"   # (five plain bytes end any operand)
        main, call, jump, rc = B.encode(data)
        return (main, call[:len(call) - 1 - variant % 4], jump, rc), n, None
    if what == "no-room":
        return B.encode(_dense(rnd, n)), 0, b""
    if what == "no-main":
        main, call, jump, rc = B.encode(_dense(rnd, n))
        return (b"", call, jump, rc), n, None
    if what == "two-windows":
        n = 1160 + variant
        data = _dense(rnd, 60) + plain(n - 120, variant) + _dense(rnd, 60)
        st4 = B.encode(data)
        assert W < len(st4[0]) <= 2 * W
        return st4, n, data
    lead = variant % 21
    data = B.trap_data(lead, n - 10 - lead if n - 10 - lead >= 5 else 5)[0]
    return B.encode(data, B.convert_0f_too), len(data), data


def rounds(n):
    """n tiny items whose kind cycles with period 7 (ROUND_KINDS) -> [(the four streams, out_len, data or None)]: 7 is
    coprime to the grid's cap, so a workgroup that takes items g, g + cap, g + 2 cap, ... meets another kind in every
    trip.  "call-cut" and "no-main" fail -- two of every seven -- and the item behind each in the same workgroup is good."""
    return [_round_item(i % 7, (i // 7) % ROUND_VARIANTS) for i in range(n)]
