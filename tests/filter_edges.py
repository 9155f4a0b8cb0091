"""Crafted inputs for the device filter kernels (lzma_amd/csrc/xlz_filter_dev.hip): content that sits ON the seams of their
work split -- the 16-byte lane, the 1 KiB wave, a thread's 4 KiB chunk stride and the 16 KiB tile of the fixed-width BCJ
kernel; the 256-byte window and the 64 KiB tile of the x86 kernels, their nine-byte lookback and their windows without a
sync point; the 16 KiB chunk, the eight-at-a-time row loop and the 256-chunk group of the Delta kernels.  The judge is
liblzma (tests/filter_ref.py); tests/test_filter_edges_cpu.py shows with liblzma alone that every case bites, and
tests/test_gpu_filter_edges.py runs them on the device.  A plain module, not a conftest.

cases() -> [Case(name, steps, data)]: steps = one to three (filter id, parameter) pairs in decoder order, data = the bytes
they are applied to.  probes(case) -> what the case exists for, a dict with some of
  "regions" / "bands": [(lo, hi)]  liblzma changes a byte in every one (an instruction; a band of several) and none outside
  "state":     (steps, data, positions) of a control without the dead opcodes: its calls at the positions convert otherwise
  "unchanged": (steps, data) of a control: the case comes back as it went in, the control does not
  "changed":   True        the property is the whole stream (chains of halfwords, filter chains): every step changes it
  "nosync":    {"windows": [...], "span": n}  x86 windows without a sync point, the longest stretch of them
  "made" / "unmade": [positions] where the converted bytes hold an E8 the originals lack / lack one the originals hold
  "delta":     {"chunks": n, "groups": g}
Everything is seeded."""
import collections
import functools
import lzma
import random

import filter_ref as R

L, V, Q, TB, W, T, G = 16, 1024, 4096, 16384, 256, 65536, 256
C = TB
DICT = 1 << 16
THUMB_OFFSETS = (0, 0xFFFFFFF0)
BCJ_OFFSETS = (0, 4096, 0xFFFFFFF0)
X86_EDGES = (W, 2 * W, T - W, T, T + W, 2 * T)
DELTA_DISTS = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256)
SEG = 1 << 20

Case = collections.namedtuple("Case", "name steps data")

# background bytes: no opcode of any BCJ filter (no E8 / E9, no 0xEB, no 0x48-0x4B, no 0x40 / 0x7F, no 0xF0-0xFF, and an
# IA-64 template below 16, which has no branch slot)
_BG = bytes(list(range(0x01, 0x10)) + list(range(0x20, 0x30)) + list(range(0x60, 0x70)))

_probes = {}
_big = {}     # name -> (first segment, bytes): streams joined from a few 1 MiB segments


_BG_OF = bytes(_BG[b % len(_BG)] for b in range(256))


def background(n, seed):
    return bytearray(random.Random(seed).randbytes(n).translate(_BG_OF))


# ---- ARM-Thumb -------------------------------------------------------------------------------------------------------------
def _first(v, p, rnd):
    v[p:p + 2] = (0xF000 | rnd.randrange(1, 0x7FF)).to_bytes(2, "little")


def _second(v, p, rnd):
    v[p:p + 2] = (0xF800 | rnd.randrange(1, 0x7FF)).to_bytes(2, "little")


def _pair(v, p, rnd):
    _first(v, p, rnd)
    _second(v, p + 2, rnd)


def _thumb_off(off, pairs):
    """a pair whose address + 4 is 0 converts to itself: such a case takes the start offset 4096 instead"""
    return 4096 if any((off + p + 4) & 0xFFFFFFFF == 0 for p in pairs) else off


def _thumb_cases(out):
    n = 2 * TB + 64
    for k, p in enumerate((0, 2, 12, 14, 16, 18, V - 2, V, Q - 2, Q, TB - 4, TB - 2, TB, TB + 2, 2 * TB - 2)):
        for off in THUMB_OFFSETS:
            rnd = random.Random(1000 + k)
            v = background(n, 1100 + k)
            _pair(v, p, rnd)
            off = _thumb_off(off, [p])
            _add(out, "thumb/pair@%d/off%x" % (p, off), [(R.ARMTHUMB, off)], v, regions=[(p, p + 4)])
    for e, E in enumerate((L, V, Q, TB)):
        for off in THUMB_OFFSETS:
            rnd = random.Random(1200 + e)
            v = background(n, 1300 + e)          # first, first, second: the pair is the last two
            _first(v, E - 4, rnd), _first(v, E - 2, rnd), _second(v, E, rnd)
            o = _thumb_off(off, [E - 2])
            _add(out, "thumb/ffs@%d/off%x" % (E, o), [(R.ARMTHUMB, o)], v, regions=[(E - 2, E + 2)])
            v = background(n, 1400 + e)          # first, second, second
            _first(v, E - 2, rnd), _second(v, E, rnd), _second(v, E + 2, rnd)
            _add(out, "thumb/fss@%d/off%x" % (E, o), [(R.ARMTHUMB, o)], v, regions=[(E - 2, E + 2)])
            v = background(n, 1500 + e)          # back to back, the edge between the pairs
            _pair(v, E - 4, rnd), _pair(v, E, rnd)
            o = _thumb_off(off, [E - 4, E])
            _add(out, "thumb/pairs@%d,%d/off%x" % (E - 4, E, o), [(R.ARMTHUMB, o)], v, regions=[(E - 4, E), (E, E + 4)])
            v = background(n, 1600 + e)          # back to back, the edge inside the first pair: the next lane must not store its
            _pair(v, E - 2, rnd), _pair(v, E + 2, rnd)   # first halfword and opens a pair of its own with its second
            o = _thumb_off(off, [E - 2, E + 2])
            _add(out, "thumb/pairs@%d,%d/off%x" % (E - 2, E + 2, o), [(R.ARMTHUMB, o)], v, regions=[(E - 2, E + 2), (E + 2, E + 6)])
    for phase in (0, 1):                         # halfwords alternate over the whole stream: opposite phase at every lane edge
        for off in THUMB_OFFSETS:
            rnd = random.Random(1700 + phase)
            v = bytearray(2 * TB + 6)
            for i in range(0, len(v), 2):
                (_first if (i // 2 + phase) % 2 == 0 else _second)(v, i, rnd)
            _add(out, "thumb/alternating%d/off%x" % (phase, off), [(R.ARMTHUMB, off)], v, changed=True)
    for base in (0, L, TB):
        for off in THUMB_OFFSETS:
            rnd = random.Random(1800 + base)
            v = background(base + 5, 1900 + base)
            _pair(v, base, rnd)
            st = [(R.ARMTHUMB, _thumb_off(off, [base]))]
            tag = "base%d/off%x" % (base, st[0][1])
            _add(out, "thumb/end+4/" + tag, st, v[:base + 4], regions=[(base, base + 4)])
            _add(out, "thumb/end+3/" + tag, st, v[:base + 3], unchanged=(st, bytes(v[:base + 4])))
            _add(out, "thumb/end+2/" + tag, st, v[:base + 2], unchanged=(st, bytes(v[:base + 4])))
            _add(out, "thumb/end+5/" + tag, st, v, regions=[(base, base + 4)])
    for off in THUMB_OFFSETS:
        rnd = random.Random(1990)
        v = background(TB + 2, 1991)
        _pair(v, TB - 2, rnd)
        st = [(R.ARMTHUMB, off)]
        _add(out, "thumb/end/tile+2/off%x" % off, st, v, regions=[(TB - 2, TB + 2)])
        _add(out, "thumb/end/tile+1/off%x" % off, st, v[:TB + 1], unchanged=(st, bytes(v)))


# ---- ARM, PowerPC, SPARC, IA-64 ----------------------------------------------------------------------------------------------
def _arm(rnd):
    return (0xEB000000 | rnd.randrange(1, 1 << 24)).to_bytes(4, "little")


def _ppc(rnd):
    return (0x48000001 | (rnd.randrange(1, 1 << 24) << 2)).to_bytes(4, "big")


def _sparc(rnd):
    if rnd.randrange(2):
        return (0x40000000 | rnd.randrange(1, 1 << 22)).to_bytes(4, "big")
    return (0x7FC00000 | rnd.randrange(1, 1 << 22)).to_bytes(4, "big")


def ia64_bundle(rnd, template):
    """a bundle whose three slots all hold the branch pattern (opcode 5, btype 0) with address bits that are not zero"""
    x = (rnd.getrandbits(128) & ~0x1F) | template
    for slot in range(3):
        at = 5 + 41 * slot
        x &= ~(((0xF << 37) | (0x7 << 9)) << at)
        x |= ((0x5 << 37) | (1 << 36) | (1 << 13) | (1 << 32)) << at
    return x.to_bytes(16, "little")


_WORD = {R.ARM: _arm, R.POWERPC: _ppc, R.SPARC: _sparc}
IA64_BRANCH_TEMPLATES = (16, 17, 18, 19, 22, 23, 24, 25, 28, 29)


def _converts(fid, off, p):
    """a convertible slot at p changes unless the address that is subtracted is zero"""
    return ((off + p + (8 if fid == R.ARM else 0)) & 0xFFFFFFFF) != 0


def _bcj_tail_cases(out):
    for fid in (R.ARM, R.POWERPC, R.SPARC, R.IA64):
        slot = R.ALIGN[fid]
        seen_empty = False
        for b, base in enumerate((0, L, Q, TB - L, TB, 2 * TB)):
            for r in range(16):
                n = base + r
                if n == 0 and seen_empty:
                    continue
                for off in BCJ_OFFSETS:
                    if n == 0 and off:
                        continue
                    rnd = random.Random(2000 + 100 * fid + 16 * b + r)
                    v = background(n + slot, 2500 + 16 * b + r)
                    regions = []
                    for p in range(max(0, n - 32) // slot * slot, n + 1, slot):   # (one slot more than the stream: the control)
                        v[p:p + slot] = ia64_bundle(rnd, rnd.choice(IA64_BRANCH_TEMPLATES)) if fid == R.IA64 else _WORD[fid](rnd)
                        if p + slot <= n and _converts(fid, off, p):
                            regions.append((p, p + slot))
                    name = "bcj%d/tail/base%d+%d/off%x" % (fid, base, r, off)
                    if regions:
                        _add(out, name, [(fid, off)], v[:n], regions=regions)
                    else:   # nothing but an incomplete slot: it comes back untouched; in the control the slot is whole
                        last = n // slot * slot
                        ctl = ([(fid, off if _converts(fid, off, last) else 4096)], bytes(v[:last + slot]))
                        _add(out, name, [(fid, off)], v[:n], unchanged=ctl)
                seen_empty |= n == 0
    for off in BCJ_OFFSETS:       # all 32 templates; the address wraps to zero at byte 16 with the last offset
        rnd = random.Random(2900)
        v = bytearray()
        for t in list(range(32)) + [16, 18, 22]:
            v += ia64_bundle(rnd, t)
        regions = [(16 * k, 16 * k + 16) for k in range(len(v) // 16)
                   if (v[16 * k] & 0x1F) in IA64_BRANCH_TEMPLATES and _converts(R.IA64, off, 16 * k)]
        _add(out, "bcj%d/templates/off%x" % (R.IA64, off), [(R.IA64, off)], v, regions=regions)
    for fid in (R.ARM, R.POWERPC, R.SPARC):   # convertible slots on both sides of the wrap, and over a whole tile edge
        for off in BCJ_OFFSETS:
            rnd = random.Random(2950 + fid)
            v = background(TB + 48, 2960 + fid)
            at = list(range(0, 48, 4)) + list(range(TB - 16, TB + 16, 4))
            for p in at:
                v[p:p + 4] = _WORD[fid](rnd)
            _add(out, "bcj%d/wrap/off%x" % (fid, off), [(fid, off)], v, regions=[(p, p + 4) for p in at if _converts(fid, off, p)])


# ---- x86 -------------------------------------------------------------------------------------------------------------------
def _call(v, p, rnd, op=None):
    """a convertible call: E8 / E9, three background bytes, 00 / FF"""
    v[p] = op or rnd.choice((0xE8, 0xE9))
    v[p + 1:p + 4] = rnd.choices(_BG, k=3)
    v[p + 4] = rnd.choice((0x00, 0xFF))


def _dirty_calls(n, rnd):
    """sort (a): the five-byte convertible call repeated -- every one converts"""
    v = bytearray(n + 5)
    for p in range(0, n, 5):
        _call(v, p, rnd)
    v = v[:n]
    if n:
        v[-1] = 0xE8
    return v


def _dirty_adversarial(n, seed, density):
    """sort (b): filter_ref.x86_adversarial with runs, an opcode forced in wherever eight bytes went without one"""
    v = bytearray(R.x86_adversarial(n, seed, density, runs=True))
    clean = 0
    for i in range(n):
        if clean >= 8 or i == 0 or i == n - 1:
            v[i] = 0xE8
        clean = 0 if (v[i] & 0xFE) == 0xE8 else clean + 1
    return v


def _x86_off(k):
    return (0, 4096)[k % 2]


def _x86_cases(out):
    n = 2 * T + 64
    for k in range(25):           # one convertible call at B + delta; the deltas of a stream differ from edge to edge
        rnd = random.Random(3000 + k)
        v = background(n, 3100 + k)
        regions = []
        for e, B in enumerate(X86_EDGES):
            p = B + (k + 4 * e) % 25 - 12
            _call(v, p, rnd)
            regions.append((p, p + 5))
        _add(out, "x86/call-at-edges/%d" % k, [(R.X86, _x86_off(k))], v, regions=regions)
    k = 0
    for dead in (10, 9, 4, 1):    # the nine-byte lookback: a dead opcode at B - dead, then calls
        for calls in ((0,), (1,), (9,), (0, 1, 9)):
            rnd = random.Random(3200 + k)
            v = background(n, 3300 + k)
            bands = []
            for B in X86_EDGES:
                v[B - dead] = 0xE8
                for c in reversed(calls):
                    _call(v, B + c, rnd)
                for c in calls:
                    v[B + c] = 0xE8
                bands.append((B - dead, B + 14))
            _add(out, "x86/lookback/dead-%d/calls%s" % (dead, "+".join(map(str, calls))), [(R.X86, _x86_off(k))], v, bands=bands)
            k += 1
    # A dead opcode one to three bytes in front of B leaves prev_mask live at B, but it shows only where the byte of the
    # converted operand that the dead opcode fell on is 00 / FF: a call at B made so that it is.  The control has no dead
    # opcode, and liblzma converts the call differently there ("state": the positions of the calls).
    for k, dead in enumerate((3, 2, 1)):
        v, off = background(n, 3380 + k), _x86_off(k)
        ctl, at = bytearray(v), []
        for B in X86_EDGES:
            sub = (off + B + 5) & 0xFFFFFFFF
            for zb in (0x00, 0xFF):
                dest = (0x00221133 & ~(0xFF << (8 * (3 - dead)))) | (zb << (8 * (3 - dead)))
                src = ((dest + sub) & 0xFFFFFFFF).to_bytes(4, "little")
                if src[3] in (0x00, 0xFF) and src[3 - dead] not in (0x00, 0xFF) and not any((b & 0xFE) == 0xE8 for b in src):
                    v[B - dead] = 0xE8
                    v[B], ctl[B] = 0xE8, 0xE8
                    v[B + 1:B + 5], ctl[B + 1:B + 5] = src, src
                    at.append(B)
                    break
        assert len(at) >= 4, (dead, at)
        st = [(R.X86, off)]
        _add(out, "x86/lookback/dead-%d/live-state" % dead, st, v, bands=[(B, B + 5) for B in at], state=(st, bytes(ctl), at))
    for k, density in enumerate((30, 60, 30, 60)):   # prev_mask live across the edge
        v = background(n, 3400 + k)
        off = 0xFFFFFFF0 if k == 3 else _x86_off(k // 2)
        for e, B in enumerate(X86_EDGES):
            for seed in range(3450 + 100 * (6 * k + e), 3550 + 100 * (6 * k + e)):   # the first seed with which liblzma converts
                band = R.x86_adversarial(80, seed, density) + bytes(v[B + 40:B + 48])   # something in the band
                if R.apply(R.X86, (off + B - 40) & 0xFFFFFFFF, band) != band:
                    break
            v[B - 40:B + 40] = band[:80]
        _add(out, "x86/state-across-edges/density%d/off%x" % (density, off), [(R.X86, off)], v, bands=[(B - 40, B + 44) for B in X86_EDGES])
    # windows without a sync point
    extents = [("inside-a-window", 4 * W, 3 * W + 20, 3 * W + 200), ("a-window-and-3", 8 * W, 5 * W - 3, 6 * W + 3)]
    extents += [("%d-windows" % k, (k + 3) * W + 7, W, (k + 1) * W) for k in (2, 255, 256, 257)]
    extents += [("257-windows-from-W-1", 260 * W + 7, W - 1, 258 * W), ("from-byte-0", 5 * W, 0, 3 * W + 7), ("from-mid-window", 8 * W, 2 * W + 100, 6 * W + 50)]
    extents += [("to-the-end-mod%d" % m, 8 * W + m, 5 * W + 17, 8 * W + m) for m in (0, 1, 4, 5, 255)]
    for k, (tag, n, s, e) in enumerate(extents):
        for sort in "ab":
            rnd = random.Random(3500 + k)
            v = background(n, 3600 + k)
            v[s:e] = _dirty_calls(e - s, rnd) if sort == "a" else _dirty_adversarial(e - s, 3700 + k, 30 + 15 * (k % 3))
            bands = [(s, min(n, e + 4))]
            if e + 45 <= n:   # a call behind the run, in the next lane's bytes: a lane that walks on past its end converts it twice
                _call(v, e + 40, rnd)
                bands.append((e + 40, e + 45))
            windows = [j for j in range(1, (n + W - 1) // W) if j * W > s and min((j + 1) * W, n) <= e + 9]
            span = max((len(run) for run in runs_of(windows)), default=0)
            _add(out, "x86/nosync/%s/%s" % (tag, sort), [(R.X86, _x86_off(k))], v, bands=bands, nosync={"windows": windows, "span": span})
    k = 0
    for n in list(range(22)) + [W + d for d in range(-5, 6)] + [T + d for d in range(-5, 6)]:
        rnd = random.Random(3800 + n)
        v = background(n, 3900 + n)
        v[max(0, n - 5):] = b"\xe8" * min(n, 5)
        st = [(R.X86, _x86_off(k))]
        if n == 0:
            _add(out, "x86/end/len0", st, v, unchanged=(st, b"\xe8\x01\x02\x03\x00"))
        else:      # one more opcode as the last byte: the call at len - 5 is dead; the control is longer by a 00
            _add(out, "x86/end/len%d/opcode" % n, st, v, unchanged=(st, bytes(v) + b"\xe8" * max(0, 4 - n) + b"\x00"))
        if n >= 5:   # the call at len - 5 converts, the opcodes behind it never
            v[-1] = rnd.choice((0x00, 0xFF))
            _add(out, "x86/end/len%d/msb" % n, st, v, regions=[(n - 5, n)])
        k += 1
    for k, off in enumerate((0, 4096)):   # an E8 made, and one unmade, by a conversion in the nine bytes in front of an edge
        v = background(2 * T + 64, 3990 + k)
        rnd = random.Random(3995 + k)
        made, unmade, regions = [], [], []
        for e, B in enumerate(X86_EDGES):
            p = B - 10
            sub = (off + p + 5) & 0xFFFFFFFF
            if e % 2 == 0:   # made: the converted operand's first byte is E8
                src = (0x002211E8 + sub) & 0xFFFFFFFF
                made.append(p + 1)
            else:            # unmade: the original operand's first byte is E8
                src = 0x003322E8
                unmade.append(p + 1)
            v[p] = 0xE8
            v[p + 1:p + 5] = src.to_bytes(4, "little")
            _call(v, B, rnd)
            regions += [(p, p + 5), (B, B + 5)]
        _add(out, "x86/made-and-unmade/off%x" % off, [(R.X86, off)], v, regions=regions, made=made, unmade=unmade)


def runs_of(xs):
    run = []
    for x in xs:
        if run and x != run[-1] + 1:
            yield run
            run = []
        run.append(x)
    if run:
        yield run


# ---- Delta -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _segments():
    return [random.Random(4000 + k).randbytes(SEG) for k in range(8)]


def _joined(first, n):
    segs = _segments()
    whole, tail = divmod(n, SEG)
    return b"".join(segs[(first + k) % 8] for k in range(whole)) + segs[(first + whole) % 8][:tail]


def _delta_probe(n):
    chunks = (n + C - 1) // C
    return {"chunks": chunks, "groups": (chunks + G - 1) // G}


def _delta_cases(out):
    for d in DELTA_DISTS:
        lens = sorted({1, d - 1, d, d + 1, 2 * d, C - 1, C, C + 1, C + d - 1, C + d, C + d + 1, 2 * C, 2 * C + 1, 3 * C - 1} - {0})
        for n in lens:
            _add(out, "delta/d%d/len%d" % (d, n), [(R.DELTA, d)], random.Random(4100 + d).randbytes(n), delta=_delta_probe(n))
    for chunks in (8, 9, 10, 16, 17, 18):
        for d in (3, 7, 255, 256):
            n = chunks * C + 5
            _add(out, "delta/d%d/chunks%d+5" % (d, chunks), [(R.DELTA, d)], random.Random(4200 + chunks).randbytes(n), delta=_delta_probe(n))
    # (the last two: three groups, the third of one chunk that is also the stream's last, and of two)
    lens = (G * C, G * C + 1, (G + 1) * C, (G + 1) * C + 1, (G + 8) * C + 5, (G + 9) * C + 5, (G + 10) * C, 2 * G * C + 3, 2 * G * C + C + 3)
    for k, n in enumerate(lens):
        for d in (3, 255, (1, 7, 16, 256)[k % 4]):
            name = "delta/d%d/groups/len%d" % (d, n)
            _big[name] = (k, n)
            _add(out, name, [(R.DELTA, d)], _joined(k, n), delta=_delta_probe(n))
    block = bytes(b for k in range(256) for b in ((0x7F, 0x80, 0xFF, 0x01)[k & 3], (0x7F, 0x80, 0xFF, 0x01)[(k >> 2) & 3],
                                                  (0x7F, 0x80, 0xFF, 0x01)[(k >> 4) & 3], (0x7F, 0x80, 0xFF, 0x01)[(k >> 6) & 3]))
    for d in (3, 255, 256):   # every carry-masking case of add_bytes in every position of a word
        n = 3 * C - 1
        v = (block * (n // len(block) + 1))[:n]
        _add(out, "delta/d%d/carry-bytes" % d, [(R.DELTA, d)], v, delta=_delta_probe(n))


# ---- chains ----------------------------------------------------------------------------------------------------------------
def _chain_cases(out):
    by = {c.name: c for c in out}
    soup = R.opcode_soup(2 * TB + 5, 5000, density=60)
    rand = random.Random(5001).randbytes(9 * C + 5)
    chains = [
        ("x86/nosync/257-windows-from-W-1/a", [(R.X86, 0), (R.DELTA, 255), (R.ARMTHUMB, 0)]),
        ("delta/d3/len%d" % (3 * C - 1), [(R.DELTA, 3), (R.DELTA, 255)]),
        ("delta/d256/chunks17+5", [(R.DELTA, 256), (R.DELTA, 1)]),
        ("thumb/alternating1/off0", [(R.ARMTHUMB, 0), (R.X86, 0)]),
        ("x86/state-across-edges/density60/off0", [(R.X86, 4096), (R.DELTA, 2), (R.ARM, 4096)]),
        ("bcj6/templates/off0", [(R.IA64, 4096), (R.DELTA, 16)]),
        ("thumb/pair@%d/off0" % (TB - 2), [(R.ARMTHUMB, 0xFFFFFFF0), (R.ARMTHUMB, 4096)]),
        ("x86/nosync/to-the-end-mod255/b", [(R.X86, 0), (R.X86, 4096)]),
        ("x86/nosync/256-windows/b", [(R.DELTA, 7), (R.X86, 0), (R.DELTA, 7)]),
    ]
    for name, steps in chains:
        _add(out, "chain/%s/%s" % (name, "-".join(str(f) for f, _ in steps)), steps, by[name].data, changed=True)
    _add(out, "chain/soup/7-8-5", [(R.ARM, 0), (R.ARMTHUMB, 4096), (R.POWERPC, 0xFFFFFFF0)], soup, changed=True)
    _add(out, "chain/soup/5-9-6", [(R.POWERPC, 4096), (R.SPARC, 0), (R.IA64, 4096)], soup[:2 * TB - 16 + 3], changed=True)
    _add(out, "chain/random/3-8-4", [(R.DELTA, 255), (R.ARMTHUMB, 0), (R.X86, 0)], rand, changed=True)


def _add(out, name, steps, data, **probe):
    assert name not in _probes, name
    _probes[name] = probe
    out.append(Case(name, list(steps), bytes(data)))


@functools.lru_cache(None)
def _all():
    out = []
    _thumb_cases(out)
    _bcj_tail_cases(out)
    _x86_cases(out)
    _delta_cases(out)
    _chain_cases(out)
    return tuple(out)


def cases():
    return list(_all())


def probes(case):
    return _probes[case.name]


def kind(case):
    """the heading of the issue a case belongs to: its filter's id, or "chain" """
    return "chain" if case.name.startswith("chain/") else case.steps[0][0]


# ---- step tables -----------------------------------------------------------------------------------------------------------
def single_step_batches():
    """one stream per class: the launch's table has one entry (n_steps == 1)"""
    by = {c.name: c for c in _all()}
    return [[by["thumb/pair@%d/off0" % (TB - 2)]], [by["x86/nosync/257-windows-from-W-1/a"]], [by["delta/d255/chunks17+5"]]]


def alternating_batch():
    """0-byte, one-tile and many-tile streams in turn, for every class in one batch: a launch's table begins and ends with a
    step of one tile, and the streams without bytes are not in it"""
    out = []
    for k, n in enumerate((0, 100, 5 * TB + 3, 0, TB, 3 * T + 1, 0, 257, 0)):
        for fid, prm in ((R.ARM, 4096), (R.X86, 0), (R.DELTA, 255), (R.ARMTHUMB, 0)):
            out.append(Case("table/%d/len%d/filter%d" % (k, n, fid), [(fid, prm)], R.opcode_soup(n + 16, 6000 + k, density=60)[:n]))
    return out


def sentinel(k):
    """a stream no step touches: a multiple of 256 bytes, full of every filter's opcodes"""
    return R.opcode_soup(256 * (1 + k % 7) + 16, 7000 + k % 16, density=90)[:256 * (1 + k % 7)]


# ---- the raw LZMA2 streams the device decodes, and liblzma's verdict -------------------------------------------------------
@functools.lru_cache(None)
def _segment_parts():
    import corpus
    return [corpus.compress_raw_lzma2(s, dict_size=DICT, preset=0)[:-1] for s in _segments()]


def raw_lzma2(data):
    import corpus
    return corpus.lzma2_concat([data[o:o + SEG] for o in range(0, len(data), SEG)] or [b""], dict_size=DICT, preset=0)


def compressed(case):
    """case.data as a raw LZMA2 stream of independent units of at most 1 MiB (dict_size 1 << 16, preset 0).  The multi-MiB
    Delta streams are joined from eight segments that are compressed once."""
    if case.name not in _big:
        return raw_lzma2(case.data)
    first, n = _big[case.name]
    whole, tail = divmod(n, SEG)
    parts = _segment_parts()
    comp = b"".join(parts[(first + k) % 8] for k in range(whole))
    if tail:
        comp += raw_lzma2(_segments()[(first + whole) % 8][:tail])[:-1]
    return comp + b"\x00"


def liblzma(comp, steps):
    """a raw LZMA2 stream decoded and passed through `steps` (decoder order) by liblzma alone"""
    chain = [R.filter_dict(f, p) for f, p in reversed(steps)] + [{"id": lzma.FILTER_LZMA2, "dict_size": DICT}]
    return lzma.decompress(comp, format=lzma.FORMAT_RAW, filters=chain)
