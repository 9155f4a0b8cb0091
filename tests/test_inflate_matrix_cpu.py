"""CPU: the stream lists of tests/inflate_matrix.py before the device sees them (tests/test_gpu_inflate_matrix.py).  First
every list BITES -- the judge (Python's zlib) and the token reader (tests/inflate_trace.py) alone say that the list holds
what it was made for: the long codes, the blocks, the distances, the classes, the seam inside and at the start of every
kind of field, the ordered pairs.  Then every list through the library's serial decoder (lzma_amd.inflate_host) and through
the g++ lane scheme (tests/c/inflate_dev_selftest.cpp --inflate-list: the wave scheme lane by lane with ONE Wave that is
never cleared, and the serial twin), and the crafted lists with a sample of the others through the sanitizer build of that
stand-alone program.  Compared: the class of the status, and for OK the bytes and the input bytes used."""
import collections
import zlib

import pytest

import inflate_edges as E
import inflate_matrix as M
import inflate_trace as T
from test_inflate_edges_cpu import SAN, _build, _host, _inflate_list

CLASSES = {E.OK, E.RESULT, E.EOF, E.OUT_CAP}
PAIR_GRID = 144     # the grid the CPU twins see the pair list at: the fewest workgroups that hold every pair in rounds one and two


def _classes(items):
    memo = {}
    return collections.Counter(memo.setdefault((d, c), E.judge(d, c))[0] for d, c, _ in items)


@pytest.fixture(scope="module")
def traces():
    return [(name, T.trace(stream), stream, size) for name, stream, size in M.corpus_streams()]


def test_the_token_reader_counts_what_zlib_produces(traces):
    assert len(traces) == len(M.KINDS) * len(M.SIZES) * len(M.SETTINGS) == 378
    for name, t, stream, size in traces:
        assert t["produced"] == len(zlib.decompress(stream, -15)) == size and t["used"] == len(stream), name
    # and on the crafted streams whose codes are known
    t = T.trace(next(c[1] for c in E.cases() if c[0] == "table/codes-of-15-bits:ok"))
    assert (t["blocks"], t["lit_max"], t["lit_long"], t["produced"]) == ([0, 0, 1], 15, 3, 7)   # 110, the length symbol 257 and the end of the block
    t = T.trace(next(c[1] for c in E.cases() if c[0] == "table/distance-codes-of-8-and-9-bits:ok"))
    assert (t["dist_max"], t["dist_long"], t["produced"]) == (9, 2, 54)
    t = T.trace(next(c[1] for c in E.cases() if c[0] == "dist/symbol-29-distance-32768-of-32768:ok"))
    assert (t["blocks"], t["dist_far"], t["produced"]) == ([1, 1, 0], 32768, 32771)


def test_the_corpus_bites(traces):
    """MEASURED by the token reader over the 378 streams: 17 698 literal/length symbols through codes above 10 bits, 4 460
    distance symbols through codes above 8 bits, decoded codes of 15 (literal), 15 (distance) and 7 (code length) bits, a
    distance of 32 505, 775 matches of 258 in one stream, 7 dynamic and 7 stored blocks in one stream; 240 stored, 135
    fixed and 288 dynamic blocks in all"""
    ts = [t for _, t, _, _ in traces]
    assert sum(t["lit_long"] for t in ts) >= 1000
    assert sum(t["dist_long"] for t in ts) >= 300
    assert max(t["lit_max"] for t in ts) == 15 and max(t["dist_max"] for t in ts) >= 13
    assert max(t["cl_max"] for t in ts) == 7
    assert max(t["dist_far"] for t in ts) >= 32000
    assert max(t["len_258"] for t in ts) >= 500
    assert max(t["blocks"][2] for t in ts) >= 5 and max(t["blocks"][0] for t in ts) >= 4
    assert all(sum(t["blocks"][k] for t in ts) >= 100 for k in range(3))
    corpus = M.corpus()
    assert len(corpus) == 4 * len(ts) and {res for _, _, res in corpus} == set(range(16))
    assert set(_classes(corpus)) == CLASSES
    assert max(cap for _, cap, _ in corpus) == 200000


def test_the_seam_sweep_bites():
    """the probe is 406 bits long: 439 (L, j) pairs put the seam on every bit of it, 72 more move a stored block's LEN /
    NLEN over bytes 1020 ... 1028; 1022 streams with the ones cut to exactly 1024 bytes"""
    start0, bits = M._probe_frame()
    met = {M.SEAM - (start0 + 8 * L + 9 * j) for L, j in M.seam_params()}
    assert set(range(bits)) <= met                       # the seam on every bit of the probe
    for stream, cap, spans in M.seam_sweep_spans():
        cls, out, used = E.judge(stream, cap)
        assert cls == E.OK and len(out) == cap and used == len(stream) >= M.WINDOW - 2
        assert spans[0][0] == "block-header" and spans[-1][1] + spans[-1][2] <= 8 * len(stream)
    for name, how in M.seam_coverage().items():
        assert how == {"inside", "begins"}, name
    # the probe holds what it was made for
    _, _, spans = M.seam_stream(0, 0)
    widths = collections.defaultdict(set)
    for kind, _, n in spans:
        widths[kind].add(n)
    assert widths["cl-length"] == {3} and len([s for s in spans if s[0] == "cl-length"]) == 19 and 7 in widths["cl-symbol"]
    assert (widths["cl-extra-16"], widths["cl-extra-17"], widths["cl-extra-18"]) == ({2}, {3}, {7})
    assert {15, 3, 4, 1} <= widths["literal"] and widths["length-extra"] == {5} and widths["distance"] == {9}
    assert widths["distance-extra"] == {13} and widths["counts"] == {14}
    t = T.trace(M.seam_stream(0, 0)[0])
    assert t["dist_far"] == 32468 and t["len_258"] == 132 and t["lit_max"] == 15 and t["cl_max"] == 7 and t["blocks"] == [1, 2, 1]
    sweep = M.seam_sweep()
    assert len(sweep) == 2 * len(M.seam_sweep_spans()) and all(len(d) <= M.WINDOW for d, _, _ in sweep[1::2])
    cut = sum(len(d) > M.WINDOW for d, _, _ in sweep[0::2])
    assert _classes(sweep) == {E.OK: len(sweep) - cut, E.EOF: cut} and cut >= 480


def test_the_stored_matrix_bites():
    m = M.stored_matrix()
    seen = set()
    for stream, cap, res in m:
        k = int.from_bytes(stream[1:3], "little")
        n = int.from_bytes(stream[6 + k:8 + k], "little")
        assert len(stream) == 10 + k + n
        if cap == k + n:
            seen.add((k, n, res))                        # the second block's bytes begin at input offset 10 + k
    small = {(k, n, res) for k in range(16) for n in M.STORED_N for res in range(16)}
    assert small <= seen and {(k, 65535, res) for k, res in M.STORED_BIG} == seen - small
    assert {(10 + k) % 16 for k in range(16)} == set(range(16))
    cls = _classes(m)
    assert set(cls) == {E.OK, E.OUT_CAP} and cls[E.OK] == len(seen) and cls[E.OUT_CAP] >= 500


def test_the_block_orders_bite():
    """nothing else here puts a fixed block behind a dynamic one behind a fixed one: a decoder that keeps its fixed tables
    over a dynamic block passes every other list"""
    orders = M.block_orders()
    assert len(orders) == 2 * 4 ** 3
    assert _classes(orders) == {E.OK: 64, E.OUT_CAP: 64}
    seen = {tuple(T.trace(d)["order"]) for d, _, _ in orders[::2]}
    assert len(seen) == 27 and (1, 2, 1) in seen        # (0 stored, 1 fixed, 2 dynamic)


def test_the_mutations_bite():
    small, big = M.mutation_lists()
    cls = _classes(small)
    assert (len(small), len(big)) == (6000, 2000)
    assert cls[E.OK] >= 1000 and cls[E.EOF] >= 1000 and cls[E.RESULT] >= 1000 and cls[E.OUT_CAP] >= 500, cls
    assert [(d, c) for d, c, _ in small[:100]] == E.mutations(100, 31337)     # the default pool draws what it drew
    pool = M.big_pool()
    assert len(pool) >= 100 and all(2048 <= len(s) <= 40960 for s, _ in pool)
    cls = _classes(big)
    assert all(cls[c] >= 200 for c in CLASSES), cls
    assert sum(len(d) > 2 * M.WINDOW for d, _, _ in big) >= 1500                # the damage lies in later windows


@pytest.mark.parametrize("grid", [PAIR_GRID, 4096])
def test_the_pairs_bite(grid):
    """in_len 0 cannot be padded: an empty input sorts behind every other item, so nothing but another empty input can
    follow one in a launch.  133 of the 144 ordered pairs of the twelve kinds can occur on the device, and do"""
    items, kinds = M.pairs(grid), M.pair_kinds_at(grid)
    assert len(items) == 4 * grid + 11 and len(M.PAIR_KINDS) == 11
    lens = [len(d) for d, _, _ in items]
    assert lens == sorted(lens, reverse=True)            # the stable sort keeps the list as it is
    assert all(lens[p] == M.PAIR_LENGTHS[p // grid] for p in range(3 * grid)) and set(lens[3 * grid:]) == {0}
    every = set(M.PAIR_KINDS) | {M.EMPTY}
    want = {(a, b) for a in every for b in every if a != M.EMPTY or b == M.EMPTY}
    assert M.pairs_met(grid) == want and len(want) == 133
    triples = {(kinds[p], kinds[p + grid], kinds[p + 2 * grid]) for p in range(grid)}
    assert len(triples) >= 121
    want_class = {"fixed": E.OK, "dynamic-286-30-15-bit": E.OK, "dynamic-one-literal-code": E.OK, "stored": E.OK,
                  "code-lengths-over-subscribed": E.RESULT, "repeats-run-over-the-lengths": E.RESULT,
                  "distances-over-subscribed": E.RESULT, "eof-with-literals-pending": E.EOF, "out-cap-with-literals-pending": E.OUT_CAP,
                  "long-good-stream": E.OK, "code-lengths-without-any-code": E.RESULT, M.EMPTY: E.EOF}
    memo = {}
    for (d, c, _), kind in zip(items, kinds):
        assert memo.setdefault((d, c), E.judge(d, c))[0] == want_class[kind], kind
    t = T.trace(M._pair_item("dynamic-286-30-15-bit", 2400)[0])
    assert (t["lit_max"], t["dist_max"], t["lit_long"], t["dist_long"]) == (15, 15, 4, 4)


def _lists():
    """name -> [(stream, out_cap, residue)], the pair list in the order one Wave meets it"""
    small, big = M.mutation_lists()
    pairs = M.lds_order(M.pairs(PAIR_GRID), PAIR_GRID)
    # in list order too: there an empty input does stand in front of every kind
    every = list(M.PAIR_KINDS)
    pairs += [x for kind in every for x in ((b"", 3, 1), M._pair_item(kind, 2400) + (2,))]
    return {"corpus": M.corpus(), "seam sweep": M.seam_sweep(), "stored matrix": M.stored_matrix(), "block orders": M.block_orders(), "mutations": small,
            "mutations of the big pool": big, "pairs": pairs}


def _jobs(items, what):
    return [("%s %d" % (what, k), d, c, res) for k, (d, c, res) in enumerate(items)]


def _san_sample():
    """the crafted lists whole; of the corpus every variant of the streams of up to 32 769 bytes of output, every eighth of
    the others; every fifth mutation"""
    ls = _lists()
    corpus = [x for k, x in enumerate(ls["corpus"]) if x[1] <= 32769 or k % 8 == 0]
    return (_jobs(ls["seam sweep"], "seam sweep") + _jobs(ls["stored matrix"], "stored matrix") + _jobs(ls["pairs"], "pairs")
            + _jobs(ls["block orders"], "block orders")
            + _jobs(corpus, "corpus") + _jobs(ls["mutations"][::5], "mutations") + _jobs(ls["mutations of the big pool"][::5], "big pool"))


def test_inflate_host_equals_zlib_on_every_list(xlz_so):
    for what, items in _lists().items():
        memo = {}
        for k, (data, cap, _) in enumerate(items):
            if (data, cap) not in memo:
                memo[(data, cap)] = True
                assert _host(data, cap) == E.judge(data, cap), (what, k)


def test_lane_scheme_equals_zlib_on_every_list(tmp_path):
    exe = _build(tmp_path, ["-O2", "-Wall", "-Werror"], "")
    for what, items in _lists().items():
        _inflate_list(exe, tmp_path, _jobs(items, what))


def test_lane_scheme_under_the_sanitizers_on_the_crafted_lists_and_a_sample(tmp_path):
    _inflate_list(_build(tmp_path, ["-O1", "-g", "-Wall", "-Werror"] + SAN, "_san"), tmp_path, _san_sample())
