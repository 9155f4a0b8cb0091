"""CPU: the packet matrix of tests/packet_matrix.py -- its coverage records are complete, the oracle agrees with the
crafter's window model and with liblzma on every stream (but for the reference's off-by-one distance, which liblzma
rejects), every section has the statuses it is meant to have, and each of the three committed fast loops decodes
sections 1, 2, 3, 5 and the tails of 6 on the emulator: bytes against the oracle at every hand-back, range / code /
state / reps / input position against tests/lzma_pydec.py at the end, the exits counted and compared with what the
rule `len < min(dist, 64) and rep0 < fill` (tools/gen_fastpath.py: copy_test, cchk) predicts from the coverage record.

What the emulator does not run: the LZMA2 form of section 5 (the chunk behind the reset inherits a model that the harness
cannot set up), section 4 (wave_copy is C++), the sweeps of section 6 (lzma_run is C++), the slots above 2^16 and the
posStates of lengths from 18 on (the high length tree has no posState).  The GPU tests run all of it."""
import collections
import lzma

import pytest

import lzma_pydec
import oracle
import packet_matrix as pm
from test_fastpath_emulated import loop, run_fast_loop  # noqa: F401  (loop: the fixture of the three committed loops)

ALL_PROPS = [(3, 0, 2), (0, 2, 0), (1, 1, 1), (3, 0, 4), (0, 4, 4)]
KINDS = ("match", "rep0", "rep1", "rep2", "rep3")
LEN_CLASSES = (2, 3, 62, 63, 64, 65, 127, 128, 129, 191, 192, 193, 272, 273)


def _sections():
    return {"lengths": pm.lengths(), "slots": pm.slots(), "copies": pm.copies() + pm.copies(dict_size=4096),
            "all_pairs": pm.all_pairs() + pm.last_packets(), "window_fill": pm.window_fill(),
            "limits": pm.limit_tails() + pm.limits(), "hbm": pm.hbm()}


# ------------------------------------------------------------------ the coverage records ----
def test_lengths_cover_every_length_in_every_pos_state():
    want = {(props, kind, n, ps_) for props in ALL_PROPS for kind in KINDS for n in range(2, 274) for ps_ in range(1 << props[2])}
    assert len(want) == 272 * 5 * (4 + 1 + 2 + 16 + 16) == 53040
    assert pm.lengths_coverage(pm.lengths()) == want
    big = {(props, kind, n, ps_) for props in [(8, 1, 0), (5, 4, 2)] for kind in KINDS for n in range(2, 274) for ps_ in range(1 << props[2])}
    assert pm.lengths_coverage([c for c in pm.hbm() if c.name.startswith("lengths")]) == big and len(big) == 6800


def _slot(rep0):
    """the pos slot that encodes rep0 (decompress.go:437-631 read backwards)"""
    for slot in range(64):
        if slot < 4:
            lo, n = slot, 1
        else:
            nbits = (slot >> 1) - 1
            lo, n = (2 | (slot & 1)) << nbits, 1 << nbits
        if lo <= rep0 < lo + n:
            return slot


def test_slots_cover_every_distance_class():
    cases = pm.slots()
    small = {(p.rep0 + 1, p.len) for p in pm.tagged(cases, "small")}
    assert small == {(d, n) for d in range(1, 129) for n in (2, 3, 4, 5)}
    want = set()
    for slot in range(42):              # slot 41: rep0 up to 2^21 - 1, the distance 2^21
        if slot < 4:
            want.add((slot, 0))
            continue
        nbits = (slot >> 1) - 1
        want |= {(slot, 0), (slot, 1), (slot, 1 << (nbits - 1)), (slot, (1 << nbits) - 1)}
        if slot >= 14:
            nd = nbits - 4
            patterns = {0, (1 << nd) - 1, sum(1 << i for i in range(0, nd, 2)), sum(1 << i for i in range(1, nd, 2))}
            want |= {(slot, (d << 4) | a) for d in patterns for a in (0, 15)}
    big = pm.tagged(cases, "big")
    got = set()
    for p in big:
        slot = _slot(p.rep0)
        base = p.rep0 if slot < 4 else (2 | (slot & 1)) << ((slot >> 1) - 1)
        got.add((slot, p.rep0 - base))
        assert p.rep0 < p.fill          # a valid match
    assert got == want and _slot((1 << 21) - 1) == 41
    assert {min(p.len - 2, 3) for p in big} == {0, 1, 2, 3}
    assert sorted(_slot(p.rep0) for p in pm.tagged(cases, "invalid")) == list(range(42, 64))
    markers = pm.tagged(cases, "marker")
    assert sorted(p.state for p in markers) == list(range(12)) and all(p.kind == "marker" for p in markers)
    # the thinned stream of the emulator: the same classes up to 2^16
    thin = {(_slot(p.rep0)) for p in pm.tagged(pm.slots(16), "big")}
    assert thin == set(range(32))


def _copy_pairs():
    dists = list(range(1, 81)) + [127, 128, 129, 255, 256, 257, 272, 273, 274, 300]
    out = set()
    for d in dists:
        for n in {2, 3, d - 1, d, d + 1, 62, 63, 64, 65, 127, 128, 129, 191, 192, 193, 272, 273}:
            if 2 <= n <= 273:
                out.add((d, n))
    return out


@pytest.mark.parametrize("dict_size", [1 << 16, 4096])
def test_copies_cover_every_pair_behind_every_follower(dict_size):
    cases = pm.copies(dict_size=dict_size)
    want = {(kind, d, n, f) for d, n in _copy_pairs() for kind in ("match", "rep")
            for f in ("literal", "short rep", "rep0 long", "match inside")}
    own = {(d, n) for d in range(3, 71) for n in range(2, min(d, 64))}
    assert len(own) == 2325
    want |= {(kind, d, n, "literal") for d, n in own for kind in ("match", "rep")}
    assert pm.copies_coverage(cases) == want
    placed = pm.placed_coverage(cases)
    if dict_size == 4096:
        assert {(pl, n) for pl in pm.PLACES for n in LEN_CLASSES} <= placed
        for c in cases:                 # the placements are where they say: the window's position behind the copy
            pos = 0
            for p in c.log:
                if p.tag and p.tag.startswith("placed"):
                    past = {"ends at the wrap": 0, "ends 1 before": -1, "ends 1 past": 1, "ends len-1 past": p.len - 1}[p.tag[7:]]
                    assert (pos + p.len) % 4096 == past % 4096, (c.name, p)
                pos += p.len
    else:
        assert placed == set()


def test_all_pairs_cover_every_distance_and_length():
    pairs = {(p.rep0 + 1, p.len) for p in pm.tagged(pm.all_pairs(), "pair")}
    assert pairs == {(d, n) for d in range(1, 274) for n in range(2, 274)} and len(pairs) == 273 * 272
    for c in pm.all_pairs():            # a literal behind each match
        assert all(c.log[i + 1].kind == "lit" for i, p in enumerate(c.log) if p.tag == "pair")
    precise = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 272, 273)
    last = pm.last_packets()
    assert {(c.log[-1].rep0 + 1, c.log[-1].len) for c in last} == {(d, n) for d in precise for n in range(2, 274)}
    assert len(last) == 24 * 272
    for c in last:                      # the last packet of a stream of known size without room to spare
        s = c.job[0]
        assert c.log[-1].tag == "last" and s.out_cap == len(c.crafted) == int.from_bytes(s.data[5:13], "little")


def test_window_fill_covers_every_edge_distance():
    got = pm.window_coverage(pm.window_fill())
    fills = (1, 2, 63, 64, 65, 4095)
    want = {("window", "match", f, d) for f in fills for d in (-2, -1, 0, 1) if f + d >= 0}
    want |= {("window", "rep", f, -2) for f in fills if f >= 3}      # (LZMA1: a rep's rep0 is two bytes old at least)
    want |= {("epoch", k, f, d) for k in ("match", "rep") for f in fills for d in (-2, -1, 0, 1) if f + d >= 0}
    for form in ("window", "epoch"):    # the window full: fill = dictSize, dist = dictSize - 1, dictSize, dictSize + 1
        want |= {(form, "match", ds, d) for ds in (4096, 4097) for d in (-2, -1, 0)}
        want |= {(form, "rep", ds, d) for ds in (4096, 4097) for d in (-2, -1)}
    assert got == want


def test_limits_sweep_every_value():
    names = collections.Counter(c.name.split(",")[0] for c in pm.limits())
    assert len(pm.limits()) == 5 * (2 * 342 + 2 * 343 + 4 * 342)
    assert set(names) == {"limits: " + t + k for t in pm.TAILS for k in ("", " behind 1 stored bytes", " behind 2 stored bytes",
                                                                        " behind 3 stored bytes", " behind 4 stored bytes")}
    for t in pm.TAILS:
        cases = [c for c in pm.limits() if c.name.startswith("limits: %s," % t)]
        S = len(next(c for c in pm.limit_tails() if c.name.endswith(t)).crafted) - pm.TRAILER
        caps = sorted(c.job[0].out_cap for c in cases if "end marker" in c.name)
        assert caps == list(range(S - 340, S + 2)) == sorted(c.job[0].out_cap for c in cases if "known size" in c.name)
        sizes = sorted(int.from_bytes(c.job[0].data[5:13], "little") for c in cases if ", size " in c.name)
        assert sizes == list(range(S - 340, S + 3))
        chunk = sorted((((c.job[0].data[0] & 31) << 16) | (c.job[0].data[1] << 8) | c.job[0].data[2]) + 1 for c in cases if "chunk size" in c.name)
        assert chunk == sizes
        assert 380 <= sum(p.len for p in cases[0].log if p.tag == "tail") <= 680
    # behind 1 .. 4 stored bytes the payload starts at every offset in its dword (3 + k bytes of stored chunk + 6 of header)
    assert {(3 + k + 6) % 4 for k in (1, 2, 3, 4)} == {0, 1, 2, 3}


# ------------------------------------------------------------------ oracle = crafter = liblzma ----
def test_the_oracle_agrees_with_the_crafter_on_every_valid_stream():
    n = 0
    for name, cases in _sections().items():
        for c in cases:
            if c.crafted is not None:
                assert c.job[1]() == (c.crafted, 0, len(c.job[0].data)), c.name
                n += 1
    assert n > 7000


def _liblzma(stream):
    """-> bytes liblzma decodes, None where it rejects the stream"""
    try:
        if stream.fmt == pm.ps.FMT_LZMA_ALONE:
            d = lzma.LZMADecompressor(format=lzma.FORMAT_ALONE)
        else:
            d = lzma.LZMADecompressor(format=lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA2, "dict_size": max(4096, stream.dict_size)}])
        return d.decompress(stream.data)
    except lzma.LZMAError:
        return None


def _reads_in_front_of_the_window(c):
    """the stream has a copy with rep0 >= fill: the reference's off-by-one distance (window.go:89-91), or a rep that
    reaches behind a dictionary reset"""
    return any(p.kind not in ("lit", "marker") and p.rep0 >= p.fill for p in c.log)


def test_the_oracle_agrees_with_liblzma_but_for_the_off_by_one_distance():
    """On every stream liblzma accepts, the oracle's bytes are liblzma's (all of them where the oracle says OK, the bytes
    that fit where room or size cut the stream short).  Where the oracle says OK and liblzma rejects or differs, the
    stream has a copy that reads in front of the window -- exactly those.  Left out: lc + lp > 4 (liblzma has no such
    model), a 4097-byte dictionary that has wrapped (the reference's posState wraps with it: parity note 1), and the
    LZMA2 form of section 5: liblzma demands new properties behind a stored chunk that resets the dictionary and rejects
    every one of them at that chunk header, and an LZMA2 chunk that announces more bytes than its payload holds, which the
    reference ends quietly and liblzma rejects: both asserted."""
    cache, odd, compared = {}, [], 0
    for name, cases in _sections().items():
        if name == "hbm":
            continue
        for c in cases:
            s = c.job[0]
            if s.dict_size == 4097 or (s.fmt == pm.ps.FMT_LZMA_ALONE and int.from_bytes(s.data[1:5], "little") == 4097):
                continue
            if c.name.startswith("epoch 2") or ("chunk size" in c.name and int(c.name.split()[-3]) > int(c.name.split()[-1])):
                assert _liblzma(s) is None, c.name
                continue
            key = (s.data, s.fmt, s.dict_size)
            if key not in cache:
                cache[key] = _liblzma(s)
            lib = cache[key]
            out, status, _ = c.job[1]()
            reads = _reads_in_front_of_the_window(c)
            if lib is None or (reads and lib[:len(out)] != out):
                if status == 0:
                    odd.append(c.name)
                    assert reads, c.name
                continue
            compared += 1
            assert lib[:len(out)] == out and (status != 0 or len(lib) == len(out)), c.name
    valid_off_by_one = [c.name for n, cs in _sections().items() if n != "hbm" for c in cs
                       if _reads_in_front_of_the_window(c) and c.job[1]()[1] == 0 and "4097" not in c.name and not c.name.startswith("epoch 2")]
    assert sorted(odd) == sorted(valid_off_by_one), (odd, valid_off_by_one)
    assert len(odd) == 6 + 4, odd     # rep0 == fill at six fills as a match, and in front of the rep at four
    assert compared > 17_000           # (of 20 692: liblzma also rejects the 3400 sizes that are too small, as the oracle does)


# ------------------------------------------------------------------ the statuses of every section ----
def _statuses(cases):
    return dict(collections.Counter(c.job[1]()[1] for c in cases))


def test_status_counts_of_every_section():
    OK, ERR, CAP, EOF = oracle.OK, oracle.ERR_RESULT, oracle.ERR_OUT_CAP, oracle.OK_INPUT_EOF
    sec = _sections()
    assert _statuses(sec["lengths"]) == {OK: 25}
    assert _statuses(sec["slots"]) == {OK: 2 + 12, ERR: 22}
    assert _statuses(sec["copies"]) == {OK: 42}
    assert _statuses(sec["all_pairs"]) == {OK: 273 + 24 * 272}
    # LZMA1: rep0 == fill + 1 at six fills and dist == dictSize + 1 at two sizes; LZMA2: the same twice (match only: a rep
    # needs no valid distance)
    wf = sec["window_fill"]
    assert _statuses([c for c in wf if c.name.startswith("window")]) == {OK: 37 - 8, ERR: 8}
    assert _statuses([c for c in wf if c.name.startswith("epoch")]) == {OK: 56 - 8, ERR: 8}
    assert _statuses(pm.limit_tails()) == {OK: 5}
    lim = pm.limits()
    for t in pm.TAILS:
        mine = [c for c in lim if c.name.startswith("limits: " + t)]
        # room: S and S + 1 fit, the 340 smaller ones do not
        for k in ("end marker", "known size", "behind 1", "behind 2", "behind 3", "behind 4"):
            assert _statuses([c for c in mine if k in c.name]) == {OK: 2, CAP: 340}, (t, k)
        # a size that is too small ends in an error (a packet is left over, or is cut), the true size is OK, a larger one
        # runs out of input: the end of an LZMA1 stream (OK_INPUT_EOF), of the chunk alone in LZMA2 (the next one ends it)
        assert _statuses([c for c in mine if ", size " in c.name]) == {ERR: 340, OK: 1, EOF: 2}, t
        assert _statuses([c for c in mine if "chunk size" in c.name]) == {ERR: 340, OK: 3}, t
    hb = sec["hbm"]
    assert _statuses([c for c in hb if not c.name.startswith(("window", "epoch"))]) == {OK: 10 + 42}
    assert _statuses([c for c in hb if c.name.startswith(("window", "epoch"))]) == {OK: 93 - 16, ERR: 16}


# ------------------------------------------------------------------ the three committed loops on the emulator ----
_STATE = {}


def _reference_state(emu, stop):
    """tests/lzma_pydec.py in front of the packet at output position `stop` (None: run to the end) -> (result, rc, state)"""
    key = (emu.payload, stop)
    if key not in _STATE:
        st = lzma_pydec._State(*emu.props)
        w = lzma_pydec.Window(emu.dict_size)
        rc = lzma_pydec._Rc(emu.payload, 0, len(emu.payload))
        assert rc.init()
        try:
            res, _ = lzma_pydec._run(rc, st, w, None, stop_at=stop)
        except lzma_pydec._Eof:
            res = "eof"
        _STATE[key] = (res, rc.range, rc.code, rc.p, st.state, list(st.reps), len(w.total))
    return _STATE[key]


def own_copy(p):
    """the rule of tools/gen_fastpath.py (copy_test, cchk): the loop does the copy itself"""
    return p.len < min(p.rep0 + 1, 64) and p.rep0 < p.fill


def emulate(prog, case, size=None):
    """one stream through one loop: every check of the module docstring -> exits by code"""
    emu = case.emu
    want, status, n_in = case.job[1]()
    lc, lp, pb = emu.props
    copies_ = [p for p in case.log if p.kind not in ("lit", "marker")]
    if emu.ends == "trailer":
        room = len(want) + pm.ROOM if size is None else size
        out, m, entries, exits, in_pos = run_fast_loop(prog, emu.payload, lc, lp, pb, emu.dict_size, room, want)
        s = m.s
        assert out == want[:len(out)] and exits[1] == 0 and exits[2] == 0, case.name
        if size is None:
            # every packet of the section went through the loop: it stopped inside the trailer, short of input
            assert status == 0 and len(want) - pm.TRAILER <= len(out) and len(emu.payload) - in_pos < 40, (case.name, len(out), in_pos)
            assert exits[3] == sum(1 for p in copies_ if not own_copy(p)), (case.name, exits)
        else:
            assert size - 128 - 273 < len(out) <= size, (case.name, len(out), size)
            ends, pos = set(), 0
            for p in case.log:
                pos += p.len
                ends.add(pos)
            if len(out) not in ends:        # the harness has cut the last copy at `size`, as lzma_run does: no packet boundary
                assert len(out) == size, (case.name, len(out), size)
                return exits
        res, rng, code, rp, state, reps, total = _reference_state(emu, len(out))
        assert res == "stop" and total == len(out), case.name
        assert (s["range"], s["code"], s["state"], in_pos) == (rng, code, state, rp), case.name
        assert [s["rep0"], s["rep1"], s["rep2"], s["rep3"]] == reps and s["prev"] == want[len(out) - 1], case.name
        return exits
    # the stream ends inside the loop: 64 bytes behind it keep the loop going up to the marker or the bad distance
    out, m, entries, exits, in_pos = run_fast_loop(prog, emu.payload + bytes(64), lc, lp, pb, emu.dict_size, len(want) + 4096, want + bytes(8192))
    s = m.s
    res, rng, code, rp, state, reps, total = _reference_state(emu, None)
    assert out == want and total == len(want), case.name
    if emu.ends == "marker":
        assert status == 0 and res == "marker" and (exits[1], exits[2]) == (0, 1), (case.name, exits)
        assert in_pos == len(emu.payload) == rp and s["code"] == 0 == code and s["rep0"] == 0xFFFFFFFF == reps[0], case.name
        assert (s["range"], s["state"]) == (rng, state) and [s["rep1"], s["rep2"], s["rep3"]] == reps[1:], case.name
    else:
        assert status == oracle.ERR_RESULT and res == "err" and (exits[1], exits[2]) == (1, 0), (case.name, exits)
        assert s["rep0"] == reps[0] == [p for p in case.log if p.tag][-1].rep0, case.name
    return exits


def _emulated(prog, cases):
    total = collections.Counter()
    for c in cases:
        total.update(emulate(prog, c))
    return total


def _emulated_lengths(full):
    """the compact layout's three properties on the compact loops, the two of pb 4 on the full loop"""
    return pm.lengths(tuple(pm.FULL_PROPS if full else pm.COMPACT_PROPS), thin=True)


def test_the_emulated_packets_stay_within_their_budget():
    """at most 40 000 packets per loop (about 1.3 ms each)"""
    for full in (False, True):
        cases, thin = _emulated_copies()
        n = pm.packets(_emulated_lengths(full) + pm.slots(16) + cases + thin + pm.limit_tails() * 2)
        n += pm.packets([c for c in pm.window_fill() if c.name.startswith("window")])
        assert 30_000 < n <= 40_000, (full, n)


def test_lengths_on_each_committed_loop(loop):
    """every length in every posState of the low and mid trees, every length of the high tree, match and rep0 .. 3: the
    compact layout's three properties on the compact loops, pb 4 on the full loop"""
    cases = _emulated_lengths(loop.lay["POS_STATES"] != 4)
    assert len(cases) == (15 if loop.lay["POS_STATES"] == 4 else 10)
    got = pm.lengths_coverage(cases)
    for props in {c.emu.props for c in cases}:
        assert {(props, k, n, ps_) for k in KINDS for n in range(2, 18) for ps_ in range(1 << props[2])} <= got
        assert {(k, n) for (pr, k, n, _) in got if pr == props} == {(k, n) for k in KINDS for n in range(2, 274)}
    _emulated(loop, cases)


def test_slots_on_each_committed_loop(loop):
    """distances 1 .. 128 x len_state, the slots up to 2^16, the invalid slots (exit 1), the end marker behind every
    state (exit 2)"""
    cases = pm.slots(16)
    exits = _emulated(loop, cases)
    assert (exits[1], exits[2]) == (22, 12)


# Up to 66 every distance; beyond it the loop's own test is `len < 64` whatever the distance (their slots: section 2)
EMULATED_DISTS = tuple(range(1, 67)) + (127, 128, 256, 273, 300)
EMULATED_OWN_REPS = (3, 4, 5, 31, 32, 33, 62, 63, 64, 65, 66, 70)


def _emulated_copies():
    return (pm.copies(dists=EMULATED_DISTS, own_rep_dists=EMULATED_OWN_REPS),
            pm.copies(dict_size=4096, dists=(1, 64, 300), own_dists=(3, 33)))


def test_copies_on_each_committed_loop(loop):
    """EMULATED_DISTS x copy_lens x {match, rep} x four followers, and every copy of the loop's own behind a literal (as a
    match at every distance, as a rep at twelve); the section again over a 4096-byte window for the distances 1, 64 and
    300 with every copy placed at the wrap.  Both kinds of copy occur, in the numbers the rule predicts (emulate()
    asserts the count of every stream)."""
    cases, thin = _emulated_copies()
    section = [p for c in cases + thin for p in c.log if p.tag and p.tag.startswith(("copy", "placed"))]
    mine = sum(1 for p in section if own_copy(p))
    assert mine >= 2325 + 12 * 30 and len(section) - mine >= 7000
    assert {(p.rep0 + 1, p.len) for p in section if own_copy(p) and p.kind == "match"} == \
        {(d, n) for d in range(3, 71) for n in range(2, min(d, 64))} | {(d, n) for d in EMULATED_DISTS if d > 70 for n in (2, 3, 62, 63)}
    assert any(p.len == 63 and own_copy(p) for p in section) and not any(p.len >= 64 and own_copy(p) for p in section)
    exits = _emulated(loop, cases + thin)
    assert exits[3] == sum(1 for c in cases + thin for p in c.log if p.kind not in ("lit", "marker") and not own_copy(p))


def test_window_fill_on_each_committed_loop(loop):
    """LZMA1: rep0 == fill - 2 .. fill + 1 while the window fills, dist == dictSize - 1 .. dictSize + 1 once it is full.
    rep0 == fill leaves the loop as a copy (exit 3, the reference's off-by-one), rep0 == fill + 1 as an error (exit 1)."""
    cases = [c for c in pm.window_fill() if c.name.startswith("window")]
    assert len(cases) == 37
    exits = _emulated(loop, cases)
    assert exits[1] == 8 and exits[2] == 0
    for c in cases:
        edge = [p for p in c.log if p.tag and p.tag.startswith("edge")]
        assert len(edge) == 1
        if edge[0].rep0 == edge[0].fill < c.emu.dict_size:     # the off-by-one distance: a copy the loop hands back
            assert not own_copy(edge[0]) and c.emu.ends == "trailer", c.name


def test_limit_tails_on_each_committed_loop(loop):
    """the five tails of section 6 with room to spare, and with a size 100 bytes short of the tail's end as room and
    bytesLeft: the loop starts no packet in the last 128 bytes in front of it and stores nothing at or behind it"""
    for c in pm.limit_tails():
        emulate(loop, c)
        emulate(loop, c, size=len(c.crafted) - pm.TRAILER - 100)     # (inside the tail: a copy may cross it)
