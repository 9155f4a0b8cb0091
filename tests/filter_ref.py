"""The judge of the filter tests: liblzma through Python's lzma module.  It applies a filter (decoder side) to ARBITRARY
bytes B: B is compressed with a raw LZMA2 filter, and that is decompressed with filters=[the filter, LZMA2].  A plain
module, not a conftest."""
import lzma
import random
import sys

DELTA, X86, POWERPC, IA64, ARM, ARMTHUMB, SPARC = 3, 4, 5, 6, 7, 8, 9
ALL = (DELTA, X86, POWERPC, IA64, ARM, ARMTHUMB, SPARC)
ALIGN = {DELTA: 1, X86: 1, POWERPC: 4, IA64: 16, ARM: 4, ARMTHUMB: 2, SPARC: 4}
OFFSETS = (0, 4096, 0xFFFFFFF0)
DISTS = (1, 2, 3, 4, 7, 16, 255, 256)
_L2 = {"id": lzma.FILTER_LZMA2, "preset": 0}


def params(fid):
    return DISTS if fid == DELTA else OFFSETS


def filter_dict(fid, param):
    return {"id": fid, "dist": param} if fid == DELTA else {"id": fid, "start_offset": param}


def apply(fid, param, data):
    """what a decoder's filter `fid` makes of `data`, by liblzma"""
    raw = lzma.compress(bytes(data), format=lzma.FORMAT_RAW, filters=[_L2])
    return lzma.decompress(raw, format=lzma.FORMAT_RAW, filters=[filter_dict(fid, param), _L2])


def apply_steps(steps, data):
    """steps: [(filter id, parameter)] in the order a decoder applies them"""
    for fid, param in steps:
        data = apply(fid, param, data)
    return data


def text(n, seed=1):
    rnd = random.Random(seed)
    words = [b"the ", b"wave ", b"arena ", b"filter ", b"branch ", b"offset ", b"\n", b"call ", b"0x", b"decoder "]
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(words)
    return bytes(out[:n])


def machine_code(n, which=0):
    """real machine code: bytes of the Python binary (which = 0) or of libxlz.so (which = 1), repeated up to n"""
    if which == 0:
        blob = open(sys.executable, "rb").read()
    else:
        from lzma_amd import build
        blob = open(build.SO, "rb").read()
    blob = blob[0x1000:] or blob
    return (blob * (n // len(blob) + 1))[:n]


def opcode_soup(n, seed, density=25):
    """random bytes in which every filter finds work: opcodes of all seven at random places"""
    rnd = random.Random(seed)
    v = bytearray(rnd.randbytes(n))
    for i in range(0, n - 16, 4):
        if rnd.randrange(100) >= density:
            continue
        r = rnd.randrange(8)
        if r == 0:
            v[i + 3] = 0xEB
        elif r == 1:
            v[i] = 0x48 | (v[i] & 3)
            v[i + 3] = (v[i + 3] & ~3) | 1
        elif r == 2:
            v[i], v[i + 1] = 0x40, v[i + 1] & 0x3F
        elif r == 3:
            v[i], v[i + 1] = 0x7F, v[i + 1] | 0xC0
        elif r == 4:
            v[i + 1], v[i + 3] = 0xF0 | (v[i + 1] & 7), 0xF8 | (v[i + 3] & 7)
        elif r == 5:
            v[i + 3], v[i + 5] = 0xF0 | (v[i + 3] & 7), 0xF8 | (v[i + 5] & 7)
        elif r == 6:
            v[i], v[i + 4] = rnd.choice((0xE8, 0xE9)), rnd.choice((0x00, 0xFF))
        else:
            b = i & ~15
            x = int.from_bytes(v[b:b + 16], "little")
            x = (x & ~0x1F) | rnd.choice((16, 17, 18, 19, 22, 23, 24, 25, 28, 29))
            for slot in range(3):
                at = 5 + 41 * slot
                x &= ~(((0xF << 37) | (0x7 << 9)) << at)
                x |= (0x5 << 37) << at
            v[b:b + 16] = x.to_bytes(16, "little")
    return bytes(v)


def x86_adversarial(n, seed, density, runs=False):
    rnd = random.Random(seed)
    v = bytearray(rnd.choice((0xE8, 0xE9)) if rnd.randrange(100) < density else rnd.choice((0, 0xFF, rnd.randrange(256)))
                  for _ in range(n))
    if runs:
        for i in range(0, n - 700, 1500):
            k = 300 + rnd.randrange(400)
            v[i:i + k] = bytes([rnd.choice((0xE8, 0xE9))]) * k
    return bytes(v)
