"""The shared case lists of the .bz2 tests (tests/test_bz2_cpu.py, tests/test_gpu_bz2.py): block shapes -- each the smallest
at which a phase of the decoder can go wrong --, files, defects, cuts and seeded mutations, and the YARDSTICK: Python's bz2.

    cases() -> [(name, file bytes)]      every case, made once per process
    yardstick(data) -> (status, bytes or None, in_consumed)   what bz2.decompress does, with where the last good stream ended
"""
import bz2
import functools
import random

import bz2_craft as craft

OK, ERR_RESULT, ERR_UNEXPECTED_EOF, ERR_OUT_CAP, ERR_UNSUPPORTED = 0, -1, -5, -6, -9


def yardstick(data):
    """bz2.decompress's loop (one decompressor per stream; a stream that raises behind a complete one is ignored with all
    behind it; input that ends inside a stream is an error) -> (OK, bytes, end of the last good stream), (ERR_RESULT, None, 0)
    or (ERR_UNEXPECTED_EOF, None, 0)"""
    out, pos = [], 0
    while pos < len(data):
        d = bz2.BZ2Decompressor()
        try:
            res = d.decompress(data[pos:])
        except OSError:
            if out:
                break
            return ERR_RESULT, None, 0
        if not d.eof:
            return ERR_UNEXPECTED_EOF, None, 0
        out.append(res)
        pos = len(data) - len(d.unused_data)
    return OK, b"".join(out), pos


def text(n, seed):
    r = random.Random(seed)
    words = [bytes(r.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(r.randint(2, 9))) for _ in range(400)]
    out = bytearray()
    while len(out) < n:
        out += r.choice(words) + (b" " if r.random() < 0.9 else b"\n")
    return bytes(out[:n])


def noise(n, seed, values=256):
    r = random.Random(seed)
    return bytes(r.randrange(values) for _ in range(n))


def one(data, **kw):
    return craft.stream([craft.block(data, **kw)], 1)


@functools.lru_cache(maxsize=None)
def shape_cases():
    """single blocks: sizes around the row (64) and the marks, periodic content (the successor vector is many cycles),
    every edge of the run-length stage, the alphabet's ends, the longest run number, nGroups 2..6, codes of length 20, full
    blocks"""
    c = []
    for n in (1, 2, 63, 64, 65, 127, 128, 129):
        c.append(("noise%d" % n, one(noise(n, n))))
        c.append(("noise4v%d" % n, one(noise(n, n, 4))))
    for n in (4095, 4096, 4097):
        c.append(("noise%d" % n, bz2.compress(noise(n, n), 1)))
        c.append(("text%d" % n, bz2.compress(text(n, n), 1)))
    c.append(("ab50", one(b"ab" * 50)))
    c.append(("abc100", one(b"abc" * 100)))
    c.append(("abcd64", one(b"abcd" * 64)))
    c.append(("abcd64_pre", one(b"abcd" * 64, max_run=4)))
    for n in (1, 4, 5, 255, 256, 259, 260, 1000):
        c.append(("x%d" % n, one(b"x" * n)))
        c.append(("x%d_fours" % n, one(b"x" * n, max_run=4)))
        c.append(("x%d_bz2" % n, bz2.compress(b"x" * n, 1)))
    # count bytes that equal the byte: the run-length stage never offers a resynchronisation point
    for name, pre in (("fours_of_4", b"\x04" * 1125), ("fours_of_0", b"\0" * 503), ("fours_of_255", b"\xff" * 322)):
        c.append((name, one(craft.unrle1(pre), pre=pre)))
    c.append(("all256", one(bytes(range(256)))))
    c.append(("all256_twice", one(bytes(range(256)) + bytes(range(255, -1, -1)))))
    c.append(("one_value", one(b"\xff")))
    w, data = craft.long_run_block(0, 100000)
    c.append(("zero_run_full", craft.stream([w], 1)))
    for g in (2, 3, 4, 5, 6):
        c.append(("groups%d" % g, one(text(700, g), n_groups=g)))
        c.append(("groups%d_deep" % g, one(text(300, 10 + g), n_groups=g, deep=True)))
    c.append(("selectors_back", one(text(500, 3), n_groups=3, selectors=[2, 2, 0, 1, 1, 2, 0, 0, 1, 2, 2, 2, 0])))
    # a successor vector that avoids the walk's marks: tt[j] = j + 128 (mod n) is ONE cycle that meets all marks at the stride
    # of 128 in its first sweep and none in the 127 sweeps behind it -- one lane would walk half the block
    c.append(("marks_avoided", one(None, column=(b"\x01" * 128 + b"\0" * 99871, 5))))
    c.append(("marks_avoided_small", one(None, column=(b"\x01" * 8 + b"\0" * 8183, 3))))
    c.append(("full_level1", bz2.compress(text(99000, 7) + noise(2000, 7), 1)))
    c.append(("full_level1_noise", bz2.compress(noise(150000, 8), 1)))
    c.append(("full_level9", bz2.compress(text(899900, 9), 9)))
    return c


@functools.lru_cache(maxsize=None)
def file_cases():
    small = bz2.compress(text(3000, 21), 1)
    c = [("empty_stream", bz2.compress(b"", 9)), ("no_bytes", b""), ("one_block", small)]
    for seed in (31, 32, 33, 34):
        c.append(("blocks15_seed%d" % seed, bz2.compress(text(1400000 + 1000 * seed, seed), 1)))
    c.append(("two_streams", small + bz2.compress(text(500, 22), 5)))
    c.append(("three_streams_one_empty", small + bz2.compress(b"", 2) + bz2.compress(noise(900, 23), 9)))
    c.append(("empty_then_stream", bz2.compress(b"", 1) + small))
    c.append(("levels_differ", bz2.compress(noise(120000, 24), 1) + bz2.compress(noise(250000, 25), 3)))
    c.append(("then_junk", small + b"junk and more junk"))
    c.append(("then_junk_magic", small + b"junk" + craft.BLOCK_MAGIC.to_bytes(6, "big") + b"junk" * 40))
    c.append(("then_junk_magic_bits", small + bytes(((craft.BLOCK_MAGIC << 3) | 5).to_bytes(7, "big")) + noise(300, 26)))
    bad = bytearray(bz2.compress(text(2000, 27), 1))
    bad[len(bad) // 2] ^= 0x10
    c.append(("then_damaged", small + bytes(bad)))
    c.append(("then_cut", small + bz2.compress(text(2000, 28), 1)[:-9]))
    c.append(("then_cut_header", small + b"BZ"))
    c.append(("then_bad_level", small + b"BZh0" + small[4:]))
    c.append(("damaged_first", bytes(bad)))
    c.append(("bad_header", b"BZx9" + small[4:]))
    return c


DEFECTS = ("orig", "groups1", "groups7", "selectors0", "len0", "len21", "empty_map", "crc", "random")


@functools.lru_cache(maxsize=None)
def defect_cases():
    data = text(1500, 41)  # (long enough for the randomised bit to change a byte)
    c = [("defect_" + d, craft.stream([craft.block(data, defect=d)], 1)) for d in DEFECTS]
    c.append(("defect_combined", craft.stream([craft.block(data)], 1, defect="combined")))
    w, _ = craft.long_run_block(7, 100001)
    c.append(("defect_run_past_block", craft.stream([w], 1)))
    c.append(("defect_orig_far", craft.stream([craft.block(data, orig=100011)], 1)))
    # a sound block in front: the defect is the second block's
    c.append(("defect_second_block_crc", craft.stream([craft.block(data), craft.block(text(300, 42), defect="crc")], 1)))
    return c


MUTATION_SEEDS = 2000


@functools.lru_cache(maxsize=None)
def mutation_cases():
    """cuts of a small file at every byte, and MUTATION_SEEDS seeded one-bit and one-byte mutations of three small files"""
    bases = [bz2.compress(text(1500, 51), 1), craft.stream([craft.block(text(200, 52), n_groups=3), craft.block(noise(150, 53, 7))], 1),
             bz2.compress(b"hello " * 40, 9) + bz2.compress(text(400, 54), 2)]
    c = [("cut%d" % k, bases[1][:k]) for k in range(len(bases[1]))]
    c += [("cut2s_%d" % k, bases[2][:k]) for k in range(len(bases[2]) - 60, len(bases[2]))]
    r = random.Random(77)
    for k in range(MUTATION_SEEDS):
        b = bytearray(bases[k % 3])
        at = r.randrange(len(b))
        if k % 2:
            b[at] ^= 1 << r.randrange(8)
        else:
            b[at] = r.randrange(256)
        c.append(("mut%d" % k, bytes(b)))
    return c


@functools.lru_cache(maxsize=None)
def cases():
    return shape_cases() + file_cases() + defect_cases() + mutation_cases()


@functools.lru_cache(maxsize=None)
def expected():
    """[yardstick(file)] for cases(), made once"""
    return [yardstick(f) for _, f in cases()]
