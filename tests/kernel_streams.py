"""Stream sets of tests/test_gpu_kernels.py -- the damaged, cut and crafted streams that the other GPU tests decode in
batches of their own, gathered into corpora that ONE launch of a chosen decode kernel sees -- and the environment that
chooses the kernel.  A plain module like tests/pipeline_streams.py, not a conftest.

The launch picks one of three LDS-model kernels (xlz_kernel.hip: launch_decode): the full model layout when some unit of
the batch announces pb > 2, else the compact layout, and at 24 workgroups per CU its branchy loop.  XLZ_NO_COMPACT and
XLZ_BRANCHY (read with getenv per batch build / per launch) force each of them on any batch.

A job is (Stream, want) as in pipeline_streams: want() is the oracle's (output bytes, status, in_consumed)."""
import functools
import os
import random
import struct

import pipeline_streams as ps  # (puts the repository root and tests/ on sys.path)
from pipeline_streams import Want, alone_job, flat_call, mismatches, raw2_job  # noqa: F401  (re-exported)

import corpus  # noqa: E402
import lzma_amd  # noqa: E402
import lzma_craft  # noqa: E402
from lzma_amd import FMT_LZMA2_RAW, FMT_LZMA_ALONE, Stream  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

KERNEL_NAMES = {"full": "xlz::xlz_decode_kernel", "compact": "xlz::xlz_decode_kernel_pb2",
                "branchy": "xlz::xlz_decode_kernel_pb2_br", "hbm": "xlz::xlz_decode_kernel_hbm_model"}
KERNEL_ENV = {"full": ("XLZ_NO_COMPACT", "1"), "compact": ("XLZ_BRANCHY", "0"), "branchy": ("XLZ_BRANCHY", "1")}
BRANCHY_PER_CU = 24     # xlz_kernel.hip: kBranchyPerCu -- the compact layout's five LDS granules, six waves per SIMD
DEFAULT_LIKE_PROPS = [(3, 0, 2), (0, 0, 0), (1, 1, 1), (0, 2, 0)]   # lc + lp <= 3, pb <= 2: the model keeps five granules


def forced(monkeypatch, kernel):
    """the environment in which every LDS-model launch runs `kernel` ("full", "compact", "branchy"; the last two on
    batches whose units all announce pb <= 2)"""
    unforced(monkeypatch)
    name, value = KERNEL_ENV[kernel]
    monkeypatch.setenv(name, value)


def unforced(monkeypatch):
    """the product's own choice: neither variable set"""
    monkeypatch.delenv("XLZ_NO_COMPACT", raising=False)
    monkeypatch.delenv("XLZ_BRANCHY", raising=False)


def kernel_of(ctx, streams):
    """-> (kernel name, (workgroups, LDS bytes)) of the main launch of a device-resident batch over `streams`, in the
    environment of the moment; nothing runs"""
    b = lzma_amd.Batch(ctx, list(streams))
    try:
        return b.kernel_name(), b.launch_info()
    finally:
        b.close()


def cus(ctx):
    """CUs of the device, read off a launch of many rounds: 65 536 tiny default-parameter streams are more than 3.2 rounds
    of 24 per CU on anything up to 850 CUs, and such a launch has 24 workgroups per CU"""
    tiny = Stream(corpus.compress_alone(b"x"), FMT_LZMA_ALONE, out_cap=1)
    name, (workgroups, _) = kernel_of(ctx, [tiny] * 65536)
    assert name == KERNEL_NAMES["branchy"] and workgroups % BRANCHY_PER_CU == 0, (name, workgroups)
    return workgroups // BRANCHY_PER_CU


# ------------------------------------------------------------------ what the host's scan sees of a stream ----
def visible_props(stream):
    """the (lc, lp, pb) of every properties byte the host reads while it plans `stream` (xlz_host.hip: plan_lzma_alone,
    scan_lzma2 -- the chunk headers as they announce themselves, not what a decode walks into)"""
    d = stream.data

    def split(b):
        return b % 9, (b // 9) % 5, b // 45
    if stream.fmt == FMT_LZMA_ALONE:
        return [split(d[0])] if len(d) >= 13 and d[0] < 225 else []
    assert stream.fmt == FMT_LZMA2_RAW
    out, pos = [], 0
    while pos < len(d):
        c = d[pos]
        if c == 0 or 3 <= c < 0x80:
            break
        hl = 3 if c < 3 else (6 if c >= 0xC0 else 5)
        if pos + hl > len(d):
            break
        if c < 3:
            pos += hl + ((d[pos + 1] << 8) | d[pos + 2]) + 1
            continue
        if c >= 0xC0:
            if d[pos + 5] >= 225:
                break
            out.append(split(d[pos + 5]))
        pos += hl + ((d[pos + 3] << 8) | d[pos + 4]) + 1
    return out


def lds_units(stream):
    """units of `stream` in the LDS-model launch (0: settled while parsing, or a model beyond LDS)"""
    props = visible_props(stream)
    if any(lc + lp > 8 for lc, lp, _ in props):
        return 0
    if stream.fmt == FMT_LZMA_ALONE:
        return len(props)
    return len(lzma_amd.lzma2_units(stream.data))


def announces_pb_up_to_2(stream):
    """the stream alone would keep a launch on the compact layout (a model beyond LDS runs in a launch of its own)"""
    props = visible_props(stream)
    return any(lc + lp > 8 for lc, lp, _ in props) or all(pb <= 2 for _, _, pb in props)


def announces_default_like_props(stream):
    """every properties byte the host sees has lc + lp <= 3 and pb <= 2: a batch of such streams keeps five LDS granules"""
    return all(lc + lp <= 3 and pb <= 2 for lc, lp, pb in visible_props(stream))


# ------------------------------------------------------------------ the sets tests/test_gpu_parity.py decodes ----
def lzma1_edge_blobs():
    """(blobs, out_caps) of test_edge_cases_match_oracle: constructor errors, cut headers, cut and garbage payloads,
    empty plaintexts, sizes that do not fit the payload, too little room"""
    p = corpus.plain("T", 5, 50_000)
    c = corpus.compress_alone(p)
    hdr = bytes([0x5D]) + struct.pack("<I", 65536) + struct.pack("<Q", 10)
    blobs = [
        b"",                                   # constructor: EOF
        bytes([225]) + b"\0" * 20,             # ErrIncorrectProperties
        bytes([0x5D, 0, 0]),                   # header cut
        hdr,                                   # rangeDec.Init: EOF
        hdr + b"\x01\0\0\0\0",                 # first rc byte != 0
        hdr + b"\0\0\0",                       # rc init cut
        c[: len(c) // 2],                      # truncated: clean EOF (parity note 4)
        c[:20],
        c[:14],
        c,                                     # out_cap too small (below)
        corpus.compress_alone(b""),            # empty plaintext, end marker only
        corpus.compress_alone(b"", known_size=True),
        corpus.compress_alone(b"x"),
        c[:13] + bytes(len(c) - 13),           # all-zero payload
        c[:13] + b"\0" + b"\xff" * 200,        # garbage payload
        c[:5] + struct.pack("<Q", len(p) - 100) + c[13:],  # size too small: truncated match / error
        c[:5] + struct.pack("<Q", len(p) + 100) + c[13:],  # size too large: marker with bytesLeft>0
    ]
    caps = [len(p)] * len(blobs)
    caps[9] = 1000
    return blobs, caps


def lzma1_corrupted_blobs():
    """(blobs, out_caps) of test_corrupted_streams_match_oracle: one to three flipped bits behind the header"""
    rnd = random.Random(42)
    blobs = []
    for i in range(48):
        p = corpus.plain("TMZ"[i % 3], 200 + i, 40_000)
        c = bytearray(corpus.compress_alone(p, known_size=(i % 4 == 0)))
        for _ in range(rnd.randint(1, 3)):
            k = rnd.randrange(13, len(c))
            c[k] ^= 1 << rnd.randrange(8)
        blobs.append(bytes(c))
    return blobs, [41_000] * len(blobs)


def lzma2_framing_blobs():
    """(blobs, dictionary sizes, out_caps) of test_lzma2_framing_edge_cases_match_oracle"""
    p = corpus.plain("T", 620, 150_000)
    c = corpus.lzma2_concat([p[:50_000], p[50_000:100_000], p[100_000:]], dict_size=1 << 16)
    blobs = [
        b"", b"\x00", b"\x03garbage", b"\x01\x00", b"\x01\x00\x02abc", b"\x01\x00\x02abc\x00", b"\x01\x00\x04ab",
        b"\x02\x00\x02abc\x00",                       # stored, no dict reset as first chunk
        b"\x80\x00\x00\x00\x04\x00\x00\x00\x00\x00\x00",  # LZMA chunk without props first
        b"\xe0\x00\x00\x00\x04\xe1" + b"\0" * 5,      # bad props byte
        b"\xe0\x00\x00\x00\x04\x5d\x01\0\0\0\0\x00",  # rc first byte != 0
        b"\xe0\x00\x00\x00\x02\x5d\x00\0\0",          # rc init cut by the chunk limit
        c[:-1],                                       # missing end byte -> ErrUnexpectedEOF
        c[: len(c) // 2],                             # cut inside a chunk
        c[: len(c) // 3] + c[len(c) // 3 + 5:],       # bytes dropped: headers no longer line up
        c + b"trailing",                              # bytes after the end marker are ignored
        c,                                            # out_cap too small (below)
    ]
    caps = [200_000] * len(blobs)
    caps[-1] = 70_000
    return blobs, [1 << 16] * len(blobs), caps


def lzma2_corrupted_blobs():
    """(blobs, dictionary sizes, out_caps) of test_lzma2_corrupted_streams_match_oracle: flipped bits anywhere, the chunk
    headers included"""
    rnd = random.Random(7)
    blobs = []
    for i in range(40):
        segs = [corpus.plain("TMZR"[(i + k) % 4], 700 + 10 * i + k, 15_000) for k in range(4)]
        c = bytearray(corpus.lzma2_concat(segs, dict_size=1 << 16))
        for _ in range(rnd.randint(1, 3)):
            k = rnd.randrange(0, len(c))
            c[k] ^= 1 << rnd.randrange(8)
        blobs.append(bytes(c))
    return blobs, [1 << 16] * len(blobs), [80_000] * len(blobs)


# ------------------------------------------------------------------ the corpora ----
def stale_read_jobs(seed=7007, n=40, props=lzma_craft.SMALL_PROPS):
    """crafted LZMA2 streams whose copies read behind dictionary resets: the ordinary launch only flags them, collect()
    decodes them again as one unit each of an exact launch (of the same kernel)"""
    rnd = random.Random(seed)
    jobs = []
    for _ in range(n):
        c, want = lzma_craft.random_lzma2_stream(rnd, dict_size=4096, props=props)
        jobs.append(raw2_job(c, len(want) + 64, dict_size=4096))
    return jobs


def wide_pb_jobs():
    """streams that announce pb 3 and 4 (one of them makes a launch a full-layout launch): whole, cut, with a flipped bit,
    without room -- the full layout's own edges"""
    rnd = random.Random(3434)
    jobs = []
    for i, (lc, lp, pb) in enumerate([(3, 0, 3), (0, 0, 4), (4, 0, 4), (1, 2, 3), (0, 4, 4), (2, 2, 3)]):
        p = corpus.plain("TMZR"[i % 4], 3400 + i, 30_000 + 1111 * i)
        c = corpus.compress_alone(p, dict_size=1 << 16, lc=lc, lp=lp, pb=pb, preset=0, known_size=(i % 2 == 0))
        flip = bytearray(c)
        flip[13 + (len(c) - 13) * rnd.randrange(1, 9) // 10] ^= 1 << rnd.randrange(8)
        jobs += [alone_job(c, len(p)), alone_job(c[: 13 + (len(c) - 13) * rnd.randrange(1, 9) // 10], len(p)),
                 alone_job(bytes(flip), len(p)), alone_job(c, len(p) * rnd.randrange(1, 9) // 10)]
        segs = [p[:10_000], p[10_000:]]
        c2 = corpus.lzma2_concat(segs, dict_size=1 << 16, lc=lc, lp=lp, pb=pb, preset=0)
        jobs += [raw2_job(c2, len(p)), raw2_job(c2[: len(c2) * 2 // 3], len(p))]
    return jobs


@functools.lru_cache(maxsize=None)
def _edge_jobs():
    import test_crafted_streams as tc
    jobs = list(ps.mixed_kind_jobs())
    blobs, caps = lzma1_edge_blobs()
    jobs += [alone_job(b, c) for b, c in zip(blobs, caps)]
    blobs, caps = lzma1_corrupted_blobs()
    jobs += [alone_job(b, c) for b, c in zip(blobs, caps)]
    for blobs, dicts, caps in (lzma2_framing_blobs(), lzma2_corrupted_blobs()):
        jobs += [raw2_job(b, c, ds) for b, ds, c in zip(blobs, dicts, caps)]
    jobs += [alone_job(b, cap) for _, b, cap in tc.crafted_lzma1()]
    jobs += [raw2_job(b, cap, ds) for _, b, ds, cap, _ in tc.crafted_lzma2()]
    jobs += [raw2_job(b, cap, ds) for _, b, ds, cap in tc.crafted_lzma2_framing() + tc.crafted_lzma2_cut_chunks()]
    for blob, ds, cap in (tc._fuzz_find(), tc._fuzz_find_wide(), tc.walks_into_larger_props(), tc.walks_into_larger_pb()):
        jobs.append(raw2_job(blob, cap, ds))
    jobs.append(raw2_job(open(os.path.join(HERE, "golden", "fuzz_reader_11_316.lzma2"), "rb").read(), 8192, 65536))
    # small streams cut at EVERY length: the reference's a.lzma (a known size, no end marker), and a liblzma stream whose
    # cuts fall on both sides of the fast loop's margins (32 bytes of input, 128 of output room) and inside its end marker
    a = open(os.path.join(HERE, "golden", "a.lzma"), "rb").read()
    p = corpus.plain("T", 3535, 1400)
    c = corpus.compress_alone(p, preset=6)
    for blob, cap in ((a, 4096), (c, len(p))):
        jobs += [alone_job(blob[:cut], cap) for cut in range(len(blob))]
    # output room of 0, 1 and one byte less than the stream decodes to
    c2 = corpus.lzma2_concat([p[:700], p[700:]], dict_size=4096, preset=0)
    for cap in (0, 1, len(p) - 1):
        jobs += [alone_job(c, cap), alone_job(corpus.compress_alone(p, known_size=True), cap), raw2_job(c2, cap, 4096)]
    n_pb2 = len(jobs)
    assert all(announces_pb_up_to_2(j[0]) for j in jobs)
    jobs += wide_pb_jobs()
    return tuple(jobs), n_pb2


def edge_jobs():
    """Every damaged, cut and crafted stream of the GPU suite, for ONE launch -> list of (Stream, want):
    pipeline_streams.mixed_kind_jobs(); the LZMA1 edge cases and flipped streams and the LZMA2 framing cases and flipped
    streams of tests/test_gpu_parity.py; the crafted streams of tests/test_crafted_streams.py, the three committed fuzzer
    finds and the two streams that walk off their headers into larger properties; two small streams cut at every length;
    output room of 0, 1 and size - 1; and, behind all of them, streams that announce pb 3 and 4 (wide_pb_jobs)."""
    return list(_edge_jobs()[0])


def pb2_edge_jobs():
    """edge_jobs() without the streams that announce pb > 2: a batch of them is a compact-layout launch"""
    jobs, n_pb2 = _edge_jobs()
    return list(jobs[:n_pb2])


@functools.lru_cache(maxsize=None)
def _default_props_edge_jobs():
    jobs = [j for j in pb2_edge_jobs() if announces_default_like_props(j[0]) and lds_units(j[0]) > 0]
    jobs += stale_read_jobs(seed=8008, n=40, props=DEFAULT_LIKE_PROPS)
    return tuple(jobs)


def default_props_edge_jobs():
    """The streams of edge_jobs() in which every properties byte the host's scan sees has lc + lp <= 3 and pb <= 2 (and that
    have a unit in the LDS-model launch), plus crafted stale-read streams of such properties: a batch of them and of
    liblzma's default streams keeps the five LDS granules that 24 workgroups per CU need.  walks_into_larger_pb() is one of
    them: the chunk that brings pb 4 is hidden from the scan."""
    return list(_default_props_edge_jobs())
