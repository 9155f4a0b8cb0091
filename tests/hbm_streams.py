"""Stream sets of tests/test_gpu_hbm_kernel.py: corpora in which EVERY stream announces a model beyond LDS (lc + lp > 8,
xlz_format.h: kMaxLcLpLds), so that a batch of them has no LDS-model launch at all and every unit is decoded by
xlz_decode_kernel_hbm_model (xlz_kernel.hip: decode_units<true, false>) -- the checked C++ packet path over a model in a
workgroup's slot of HBM scratch, one workgroup per CU looping over the queue.  A plain module like
tests/kernel_streams.py, not a conftest.

liblzma refuses to encode lc + lp > 4: the valid streams are written packet by packet with tests/lzma_craft.py.
Everything is deterministic (fixed seeds).  A job is (Stream, want) as in pipeline_streams: want() is the oracle's
(output bytes, status, in_consumed).  An entry is (name, job, crafted): `crafted` is what the crafter's own window model
expects of a VALID stream (None for a damaged one).

Two things keep a stream out of these corpora, because it would not meet the HBM kernel: an LZMA2 stream cut in front of
its first properties byte (lengths 0 .. 5) is a unit of the LDS-model launch -- short_cut_jobs() has those, for the
mixed batch --, and a flipped bit that hides every large properties byte from the host's scan (flips are drawn again
until the scan still sees one)."""
import functools
import random
import struct

import pipeline_streams as ps  # (puts the repository root and tests/ on sys.path)
from pipeline_streams import alone_job, raw2_job

import corpus  # noqa: E402
import kernel_streams as ks  # noqa: E402
import lzma_amd  # noqa: E402
import lzma_craft  # noqa: E402
from lzma_craft import Encoder, Window, alone_header, lzma2_lzma_chunk, lzma2_stored, props_byte  # noqa: E402

# lc + lp = 9, 10, 11, 12 with pb 0 .. 4
BIG_PROPS = [(8, 1, 0), (5, 4, 2), (6, 4, 0), (8, 2, 3), (7, 4, 4), (8, 4, 2), (8, 4, 4), (7, 2, 1)]
SMALLER_BIG_PROPS = [p for p in BIG_PROPS if p[0] + p[1] <= 10]   # the every-length streams and most tiny units
STALE_PROPS = [(8, 4, 2), (6, 4, 0)]
DICT_SIZES = (4096, 4097, 65536)
MATCH_LENS = (2, 64, 65, 273)
MAX_LC_LP_LDS = 8             # xlz_format.h: kMaxLcLpLds


def announces_a_big_model(stream):
    """some properties byte that the host's scan sees has lc + lp > 8: every unit of the stream is an HBM-model unit"""
    return any(lc + lp > MAX_LC_LP_LDS for lc, lp, _ in ks.visible_props(stream))


# ------------------------------------------------------------------ packets ----
def _packets(e, rnd, n_out, epoch_start, n_lit):
    """n_out .. n_out + 272 more bytes into e's window: n_lit literals, then matches of length 2 / 64 / 65 / 273 (distances 1, the
    whole epoch, the dictionary's size once it is full ...), rep matches, short reps and literals -- every copy inside the
    dictionary epoch that began at output offset epoch_start"""
    w = e.w
    end = len(w.total) + n_out
    for _ in range(max(n_lit, 1)):
        e.literal(rnd.randrange(97, 123) if rnd.random() < 0.8 else rnd.randrange(256))
    while len(w.total) < end:
        avail = min(len(w.total) - epoch_start, w.size)
        r = rnd.random()
        if r < 0.45:
            d = rnd.choice([1, 2, 3, 9, avail, max(1, avail - 1), max(1, avail // 3), rnd.randint(1, avail)])
            e.match(min(d, avail), rnd.choice(MATCH_LENS + (3, 18)))
        elif r < 0.65:
            e.rep(rnd.randrange(4), rnd.choice(MATCH_LENS + (9,)))
        elif r < 0.8:
            e.short_rep()
        else:
            e.literal(rnd.randrange(256) if rnd.random() < 0.5 else rnd.choice(b"abcde "))


def crafted_lzma1(props, dict_size, total, seed, known_size=False, n_lit=300):
    """a VALID .lzma stream of about `total` bytes with an end marker, or with its size in the header and none
    -> (bytes, expected output)"""
    rnd = random.Random(seed)
    e = Encoder(*props, dict_size=dict_size)
    _packets(e, rnd, total, 0, n_lit)
    want = bytes(e.w.total)
    if known_size:
        return alone_header(*props, dict_size, size=len(want)) + e.payload(), want
    e.end_marker()
    return alone_header(*props, dict_size) + e.payload(), want


def _lzma2_chunks(seed, dict_size, plan):
    """plan: per chunk (control, props or None, bytes of output, literals) -- control 1 / 2: a stored chunk of that many
    random bytes.  -> ([[control, uncompressed size, payload, props byte]], expected output)"""
    rnd = random.Random(seed)
    w = Window(dict_size)
    e, cur, epoch_start, chunks = None, None, 0, []
    for control, props, n_out, n_lit in plan:
        if control in (1, 0xE0):
            w.reset()
            epoch_start = len(w.total)
        if control < 3:
            data = bytes(rnd.randrange(256) for _ in range(n_out))
            for b in data:
                w.put(b)
            chunks.append([control, len(data), data, None])
            continue
        if control >= 0xC0:
            cur = props
        if e is None:
            assert control >= 0xC0
            e = Encoder(*cur, dict_size=dict_size, window=w)
        else:
            e.new_chunk()
            if control >= 0xC0:
                e.renew(*cur)
            elif control == 0xA0:
                e.reset_state()
        start = len(w.total)
        _packets(e, rnd, n_out, epoch_start, n_lit)
        chunks.append([control, len(w.total) - start, e.payload(), props_byte(*cur)])
    return chunks, bytes(w.total)


def _lzma2_blob(chunks):
    out = b""
    for control, unc, payload, pbyte in chunks:
        out += lzma2_stored(payload, control == 1) if control < 3 else lzma2_lzma_chunk(control, unc, payload, pbyte)
    return out + b"\x00"


# ------------------------------------------------------------------ the parts of the edge corpus ----
@functools.lru_cache(maxsize=None)
def valid_lzma1_entries():
    """one stream per entry of BIG_PROPS with an end marker and one with a known size: 2 .. 20 KB of output, dictionaries
    of 4096, 4097 and 65536 bytes (the smaller ones wrap)"""
    out = []
    for i, props in enumerate(BIG_PROPS):
        for known in (False, True):
            k = 2 * i + known
            total = 2000 + (k * 4801) % 18_000
            blob, want = crafted_lzma1(props, DICT_SIZES[k % 3], total, 6100 + k, known_size=known)
            name = "valid lzma1 %s %s" % (props, "known size" if known else "end marker")
            out.append((name, alone_job(blob, len(want) + (0 if known else 16)), want))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def small_streams():
    """the streams that are cut at every length and given too little room: (8,1,0) LZMA1 of about 1.4 KB in both forms, and
    an LZMA2 stream of a 0xE0 chunk (8,1,0), a 0xC0 chunk that renews the model with (6,4,0), a stored chunk that resets
    the dictionary -> [(name, format, bytes, dictionary size, expected output)]"""
    a, want_a = crafted_lzma1((8, 1, 0), 4096, 1400, 6201, n_lit=330)
    b, want_b = crafted_lzma1((8, 1, 0), 4096, 1400, 6202, known_size=True, n_lit=330)
    chunks, want_c = _lzma2_chunks(6203, 4096, [(0xE0, (8, 1, 0), 700, 150), (0xC0, (6, 4, 0), 500, 120), (1, None, 40, 0)])
    c = _lzma2_blob(chunks)
    assert 300 < len(a) < 700 and 300 < len(b) < 700 and len(c) <= 600, (len(a), len(b), len(c))
    return (("lzma1 end marker", "alone", a, 4096, want_a), ("lzma1 known size", "alone", b, 4096, want_b),
            ("lzma2 three chunks", "raw2", c, 4096, want_c))


def _job(fmt, blob, cap, dict_size):
    return alone_job(blob, cap) if fmt == "alone" else raw2_job(blob, cap, dict_size)


LZMA2_FIRST_PROPS_AT = 6      # an LZMA2 stream shorter than this shows the host's scan no properties byte

# LZMA1 streams cut inside their 13-byte header never reach the device: settled while parsing (xlz_host.hip: plan_lzma_alone)
HOST_SETTLED = frozenset("%s cut at %d" % (name, cut) for name in ("lzma1 end marker", "lzma1 known size") for cut in range(13))


@functools.lru_cache(maxsize=None)
def cut_entries():
    out = []
    for name, fmt, blob, ds, want in small_streams():
        for cut in range(0 if fmt == "alone" else LZMA2_FIRST_PROPS_AT, len(blob)):
            out.append(("%s cut at %d" % (name, cut), _job(fmt, blob[:cut], len(want) + 16, ds), None))
    return tuple(out)


def short_cut_jobs():
    """the LZMA2 stream of small_streams() cut in front of its first properties byte: units of the LDS-model launch"""
    name, fmt, blob, ds, want = small_streams()[2]
    return [raw2_job(blob[:cut], len(want) + 16, ds) for cut in range(LZMA2_FIRST_PROPS_AT)]


@functools.lru_cache(maxsize=None)
def room_entries():
    out = []
    for name, fmt, blob, ds, want in small_streams():
        for cap in (0, 1, len(want) - 1):
            out.append(("%s room %d" % (name, cap), _job(fmt, blob, cap, ds), None))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def flipped_lzma1_entries():
    """48 streams: one to three flipped bits behind the header of the valid LZMA1 streams"""
    rnd = random.Random(6300)
    valid = valid_lzma1_entries()
    out = []
    for i in range(48):
        name, (s, _), want = valid[i % len(valid)]
        c = bytearray(s.data)
        for _ in range(rnd.randint(1, 3)):
            c[rnd.randrange(13, len(c))] ^= 1 << rnd.randrange(8)
        out.append(("flipped %d of %s" % (i, name), alone_job(bytes(c), len(want) + 1000), None))
    return tuple(out)


def _unit_plan(rnd, n_units, first):
    """chunks of n_units dictionary-reset units: every unit's 0xE0 chunk brings other large properties than the unit before
    (lc + lp = 12 in front of 9 among them), chunks that renew the properties (0xC0), reset the state (0xA0) or nothing
    (0x80) and stored chunks behind it"""
    order = [(8, 4, 2), (8, 1, 0), (6, 4, 0), (7, 4, 4), (5, 4, 2), (8, 4, 4), (7, 2, 1), (8, 2, 3)]
    plan, unit_of = [], []
    for u in range(n_units):
        plan.append((0xE0, order[(first + u) % len(order)], rnd.randint(200, 900), rnd.randint(20, 80)))
        unit_of.append(u)
        for k in range(rnd.randint(1, 3)):
            control = (0xC0, 0xA0, 0x80, 2)[(first + u + k) % 4] if k else (0xC0, 0xA0)[(first + u) % 2]
            props = SMALLER_BIG_PROPS[(first + 3 * u + k) % len(SMALLER_BIG_PROPS)] if control == 0xC0 else None
            plan.append((control, props, rnd.randint(30, 700), rnd.randint(5, 40)))
            unit_of.append(u)
    return plan, unit_of


@functools.lru_cache(maxsize=None)
def multi_unit_entries():
    """12 valid LZMA2 streams of 3 .. 6 dictionary-reset units, and of each one two damaged variants whose units do not
    keep what their headers announce -- a chunk of a unit that is not the last loses the end of its payload (the unit
    makes fewer bytes, and the chunk behind it starts on a half-done packet), or announces more output than its payload
    holds --: the stream is decoded again as ONE unit of the exact HBM-model launch (fold_streams -> again())
    -> (valid entries, damaged entries)"""
    valid, damaged = [], []
    for i in range(12):
        rnd = random.Random(6400 + i)
        n_units = 3 + i % 4
        ds = (4096, 65536)[i % 2]
        plan, unit_of = _unit_plan(rnd, n_units, i)
        chunks, want = _lzma2_chunks(6450 + i, ds, plan)
        blob = _lzma2_blob(chunks)
        assert len(lzma_amd.lzma2_units(blob)) == n_units, (i, n_units)
        valid.append(("multi-unit %d" % i, raw2_job(blob, len(want) + 64, ds), want))
        lzma_chunks = [k for k, c in enumerate(chunks) if c[0] >= 0x80 and unit_of[k] < n_units - 1]
        k = lzma_chunks[rnd.randrange(len(lzma_chunks))]
        cut = [list(c) for c in chunks]
        cut[k][2] = cut[k][2][:-rnd.randint(1, 3)]
        k2 = lzma_chunks[rnd.randrange(len(lzma_chunks))]
        more = [list(c) for c in chunks]
        more[k2][1] += rnd.randint(1, 9)
        for what, cs in (("chunk %d cut" % k, cut), ("chunk %d announces more" % k2, more)):
            b2 = _lzma2_blob(cs)
            assert len(lzma_amd.lzma2_units(b2)) > 1
            damaged.append(("multi-unit %d, %s" % (i, what), raw2_job(b2, len(want) + 64, ds), None))
    return tuple(valid), tuple(damaged)


@functools.lru_cache(maxsize=None)
def flipped_lzma2_entries():
    """40 streams: one to three flipped bits anywhere, the chunk headers included, in the valid multi-unit streams.  A draw
    after which the host's scan sees no large properties byte any more is drawn again (FLIPS_DRAWN_AGAIN counts them)."""
    rnd = random.Random(6500)
    valid = multi_unit_entries()[0]
    out, again = [], 0
    for i in range(40):
        name, (s, _), want = valid[i % len(valid)]
        while True:
            c = bytearray(s.data)
            for _ in range(rnd.randint(1, 3)):
                c[rnd.randrange(0, len(c))] ^= 1 << rnd.randrange(8)
            job = raw2_job(bytes(c), len(want) + 1000, s.dict_size)
            if announces_a_big_model(job[0]):
                break
            again += 1
        out.append(("flipped %d of %s" % (i, name), job, None))
    FLIPS_DRAWN_AGAIN[0] = again
    return tuple(out)


FLIPS_DRAWN_AGAIN = [0]


# The seeds from 9000 on whose random_lzma2_stream(dict_size=4096, props=STALE_PROPS) announces a large model AND reads
# bytes of an earlier epoch behind a dictionary reset (about one seed in twenty does: a chunk that keeps the reps behind a
# stored chunk that resets the dictionary, over a window that the epochs before have filled).  The CPU test shows it of each
# one: decoded with a window that is cleared at every reset they give other bytes.
STALE_SEEDS = (9006, 9027, 9100, 9108, 9138, 9203, 9204, 9206, 9231, 9275, 9312, 9317, 9326, 9328, 9330, 9343, 9370, 9373,
               9385, 9390, 9421, 9428, 9432, 9501, 9506, 9507, 9521, 9549, 9558, 9602, 9609, 9623, 9642, 9652, 9655, 9694,
               9717, 9760, 9766, 9772)


@functools.lru_cache(maxsize=None)
def stale_read_entries():
    """40 crafted LZMA2 streams of large properties whose copies read behind dictionary resets: the HBM-model launch only
    flags them (AUX_STALE), the exact launch with big = true decodes each again as one unit"""
    out = []
    for seed in STALE_SEEDS:
        c, want = lzma_craft.random_lzma2_stream(random.Random(seed), dict_size=4096, props=STALE_PROPS)
        out.append(("stale reads, seed %d" % seed, raw2_job(c, len(want) + 64, dict_size=4096), want))
    return tuple(out)


WALK_HIDDEN_PROPS = [(8, 2, 0), (6, 4, 1), (7, 4, 0), (8, 3, 2), (8, 4, 0), (8, 4, 3)]   # lc + lp = 10, 10, 11, 11, 12, 12


@functools.lru_cache(maxsize=None)
def walk_entries():
    """40 variants of test_crafted_streams.walks_into_larger_props with VISIBLE properties (8,1,0): the first chunk announces
    more compressed bytes than its literals need, so the host's scan jumps over a 0xE0 chunk of lc + lp = 10, 11 or 12 that
    the real decode walks into.  In a batch whose largest visible model is lc + lp = 9 the HBM-model unit stops in front
    of that chunk (AUX_GROW) and the stream goes to the widest re-run -- 40 of them are more than its 32 workgroups."""
    out = []
    for i in range(40):
        rnd = random.Random(6600 + i)
        hidden = WALK_HIDDEN_PROPS[i % len(WALK_HIDDEN_PROPS)]
        e = Encoder(8, 1, 0)
        first = bytes(rnd.randrange(256) if rnd.random() < 0.5 else rnd.choice(b"abc") for _ in range(rnd.randint(5, 40)))
        for b in first:
            e.literal(b)
        p1 = e.payload()
        e2 = Encoder(*hidden)
        _packets(e2, rnd, rnd.randint(0, 400), 0, rnd.randint(3, 30))
        want2 = bytes(e2.w.total)
        second = lzma2_lzma_chunk(0xE0, len(want2), e2.payload(), props_byte(*hidden))
        body = p1 + second
        hdr = bytes([0xE0, 0, len(first) - 1]) + (len(body) + 7 - 1).to_bytes(2, "big") + bytes([props_byte(8, 1, 0)])
        blob = hdr + body + b"\x00" * 8
        out.append(("walks into %s, variant %d" % (hidden, i), raw2_job(blob, len(first) + len(want2) + 64, 1 << 16), first + want2))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def relabelled_entries():
    """liblzma payloads relabelled with a large-model properties byte (deterministic garbage), noise payloads and all-zero
    payloads, as test_gpu_parity.py's test_large_lc_lp_models_live_in_hbm builds them"""
    rnd = random.Random(6700)
    out = []
    for i, props in enumerate(BIG_PROPS):
        p = corpus.plain("TRMZ"[i % 4], 6700 + i, 8000)
        c = bytearray(corpus.compress_alone(p))
        c[0] = props_byte(*props)
        if i % 2:
            c[5:13] = struct.pack("<Q", 5000)
        out.append(("relabelled %s" % (props,), alone_job(bytes(c), 20_000), None))
    for i in range(3):
        hdr = bytes([props_byte(8, 4, 4)]) + struct.pack("<IQ", 1 << 16, 20_000)
        out.append(("noise %d" % i, alone_job(hdr + b"\x00" + bytes(rnd.randrange(256) for _ in range(2000)), 20_000), None))
    for props in [(8, 4, 4), (7, 2, 0), (8, 1, 2)]:
        blob = bytes([props_byte(*props)]) + struct.pack("<IQ", 1 << 16, 0xFFFFFFFFFFFFFFFF) + bytes(1500)
        out.append(("zero payload %s" % (props,), alone_job(blob, 20_000), None))
    return tuple(out)


# ------------------------------------------------------------------ the corpora ----
@functools.lru_cache(maxsize=None)
def hbm_edge_entries():
    valid_multi, damaged_multi = multi_unit_entries()
    return (valid_lzma1_entries() + cut_entries() + room_entries() + flipped_lzma1_entries() + flipped_lzma2_entries() +
            valid_multi + damaged_multi + stale_read_entries() + walk_entries() + relabelled_entries())


def hbm_edge_jobs():
    """Every edge stream of the HBM-model kernel, for ONE launch -> list of (Stream, want): valid crafted LZMA1 streams of
    every entry of BIG_PROPS; three small streams cut at every length that still shows the large model, and given room
    for 0, 1 and size - 1 bytes; flipped LZMA1 and LZMA2 streams; LZMA2 streams of several dictionary-reset units, whole
    and damaged; stale reads; streams that walk into larger properties; relabelled, noise and zero payloads."""
    return [e[1] for e in hbm_edge_entries()]


def rerun_entries():
    """the streams that an exact or the widest re-run settles: stale reads, walks into larger properties, damaged units"""
    return stale_read_entries() + walk_entries() + multi_unit_entries()[1]


MANY_KINDS = ("valid", "known size", "cut", "flipped", "no room", "two units")


@functools.lru_cache(maxsize=None)
def _many_entry(i):
    """tiny stream number i of hbm_many_jobs: depends on i alone"""
    rnd = random.Random(6800 + i)
    props = SMALLER_BIG_PROPS[i % len(SMALLER_BIG_PROPS)]
    if i % 16 == 15:
        props = ((8, 4, 2), (8, 4, 4))[(i // 16) % 2]     # a small model follows a large one in the same slot
    elif i % 32 == 7:
        props = (7, 4, 4)
    kind = MANY_KINDS[i % len(MANY_KINDS)]
    total = 300 + (i * 389) % 2700
    ds = DICT_SIZES[i % 3]
    name = "tiny %d, %s, %s" % (i, kind, props)
    if kind == "two units":
        other = SMALLER_BIG_PROPS[(i + 2) % len(SMALLER_BIG_PROPS)]
        chunks, want = _lzma2_chunks(6900 + i, ds, [(0xE0, props, total // 2 - 30, 30), (0xA0, None, 60, 5), (0xE0, other, total // 2 - 30, 30)])
        blob = _lzma2_blob(chunks)
        assert len(lzma_amd.lzma2_units(blob)) == 2
        return name, raw2_job(blob, len(want) + 16, ds), want, 2
    blob, want = crafted_lzma1(props, ds, total, 6900 + i, known_size=(kind == "known size"), n_lit=60)
    if kind == "cut":
        return name, alone_job(blob[:13 + rnd.randrange(len(blob) - 13)], len(want) + 16), None, 1
    if kind == "flipped":
        c = bytearray(blob)
        c[rnd.randrange(13, len(c))] ^= 1 << rnd.randrange(8)
        return name, alone_job(bytes(c), len(want) + 300), None, 1
    if kind == "no room":
        return name, alone_job(blob, rnd.randrange(len(want))), None, 1
    return name, alone_job(blob, len(want) + 16), want, 1


@functools.lru_cache(maxsize=None)
def _redo_entry(i):
    props = SMALLER_BIG_PROPS[i % len(SMALLER_BIG_PROPS)]
    if i % 16 == 15:
        props = ((8, 4, 2), (8, 4, 4))[(i // 16) % 2]
    other = SMALLER_BIG_PROPS[(i + 3) % len(SMALLER_BIG_PROPS)]
    ds = DICT_SIZES[i % 3]
    n_out = 150 + (i * 97) % 500
    chunks, want = _lzma2_chunks(7300 + i, ds, [(0xE0, props, n_out, 30), (0xA0, None, 60, 5), (0xE0, other, n_out, 30)])
    chunks[i % 2][1] += 1 + i % 9      # a chunk of the FIRST unit announces more output than its payload holds
    blob = _lzma2_blob(chunks)
    return "short first unit %d, %s" % (i, props), raw2_job(blob, len(want) + 16, ds), None


def hbm_redo_entries(n):
    """n tiny LZMA2 streams of two units whose first unit makes fewer bytes than its headers announce: every one is decoded
    again as ONE unit of the exact HBM-model launch (xlz_host.hip: fold_streams -> again(), run_units(big = true)), whose
    grid is min(n, CUs) -- with n > CUs its model slots are used again"""
    return [_redo_entry(i) for i in range(n)]


def hbm_many_entries(n_units):
    """tiny streams of n_units units in all (a two-unit stream that would be one unit too many gives way to the next)"""
    out, units, i = [], 0, 0
    while units < n_units:
        e = _many_entry(i)
        i += 1
        if units + e[3] > n_units:
            continue
        out.append(e[:3])
        units += e[3]
    return out


def hbm_many_jobs(n_units):
    """`n_units` tiny HBM-model units for the slot-reuse test -> list of (Stream, want): outputs of 300 .. 3000 bytes;
    properties cycle through those of lc + lp = 9 and 10, every 16th stream is lc + lp = 12 and every 32nd 11; kinds cycle
    through valid LZMA1, known size, cut, flipped, no room, two-unit LZMA2"""
    return [e[1] for e in hbm_many_entries(n_units)]
