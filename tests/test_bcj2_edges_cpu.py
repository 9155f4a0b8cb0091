"""CPU: the crafted seam cases of tests/bcj2_edges.py, without a GPU.  With the Python reference alone (tests/bcj2_ref.py)
every case BITES: its probe restates what the case is named for -- the head / chunks / tail of its window's store, the one
candidate the main stream of a trap chain shows, the side stream that runs out -- and the totals are asserted so that an
edit cannot quietly thin the cases.  Then every case through the library's serial merge (lzma_amd.bcj2_host) and through
the g++ lane scheme (tests/c/bcj2_dev_selftest.cpp --merge-list: lanes in descending order, the destination at the residue
the case names, guard bytes compared), also built with AddressSanitizer and UBSan: the reference's status, and its bytes
when that is OK.  The items of rounds(n) share one Wave that is not cleared between them."""
import collections
import os
import subprocess

import pytest

import bcj2_edges as E
import bcj2_ref as B
import lzma_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
ROUNDS = 7 * E.ROUND_VARIANTS * 2 + 3

COUNTS = {"residue": 656, "chunks": 28, "chain": 10, "cuts": 130, "lines": 227, "seam": 14}


@pytest.fixture(scope="module")
def judged():
    """per case name: the reference's (status, bytes) -- computed once, never changed"""
    return {name: B.decode(*st4, n) for name, st4, n, _ in E.cases()}


def test_totals():
    cs = E.cases()
    assert dict(collections.Counter(E.family(c) for c in cs)) == COUNTS
    assert len({c[0] for c in cs}) == len(cs) == sum(COUNTS.values())
    assert [len(E.cases(f)) for f in E.FAMILIES] == [COUNTS[f] for f in E.FAMILIES]
    assert sum(len(s) for _, st4, _, _ in cs for s in st4) < 2_500_000     # (the Python coder does some 2 MB/s)
    assert {E.residue(c[0]) for c in cs} == set(range(16))
    for f in ("chain", "cuts", "lines", "seam"):
        assert len({E.residue(c[0]) for c in E.cases(f)}) >= 8, f


def test_every_case_bites(judged):
    facts = collections.defaultdict(list)
    for c in E.cases():
        name, st4, n, probe = c
        st, out = judged[name]
        got = probe(st, out)
        assert isinstance(got, dict), name
        facts[E.family(c)].append(got)
    # residue: every out_len x residue, and every head / chunk / tail shape a window of up to 40 bytes has
    assert {(n, r) for n in range(41) for r in range(16)} == {(c[2], E.residue(c[0])) for c in E.cases("residue")}
    assert {f["shape"] for f in facts["residue"]} == {(h, k, t) for h in (False, True) for k in (0, 1, 2) for t in (False, True)}
    # chunks: every count at every residue that can have it, every trip count of the store's loop, the full image
    by = collections.defaultdict(set)
    for c, f in zip(E.cases("chunks"), facts["chunks"]):
        by[f["chunks"]].add(E.residue(c[0]))
    assert dict(by) == {k: ({0} if k == 320 else set(E.CHUNK_RESIDUES)) for k in E.CHUNK_COUNTS}
    assert {f["trips"] for f in facts["chunks"]} == {1, 2, 3, 4, 5}
    assert {k: -(-k // 64) for k in E.CHUNK_COUNTS} == {63: 1, 64: 1, 65: 2, 128: 2, 129: 3, 192: 3, 193: 4, 256: 4, 257: 5, 320: 5}
    assert sum(f["full"] for f in facts["chunks"]) == 1
    # chain: lane seams at every lead; a window seam, with a trapped byte as the next window's first, at four of them (a chain
    # of 301 main bytes behind a lead of 0 to 16, or from a window's first byte on, lies inside one window)
    assert [int(c[0].split("lead")[1].split("@")[0]) for c in E.cases("chain")] == list(E.CHAIN_LEADS)
    assert all(f["lane_seams"] >= 18 for f in facts["chain"])
    assert [f["window_seam"] for f in facts["chain"]] == [lead + E.CHAIN_LINKS >= E.W > lead or lead + E.CHAIN_LINKS >= 2 * E.W > lead
                                                          for lead in E.CHAIN_LEADS]
    assert sum(f["window_seam"] for f in facts["chain"]) == 4 and [f["trap_opens_a_window"] for f in facts["chain"]] == [f["window_seam"] for f in facts["chain"]]
    # cuts: a candidate as the last byte and an operand cut after one, two and three bytes -- at the start, at the seam
    e8 = [f for f in facts["cuts"] if "phase" in f]
    assert len(e8) == 90 and {f["phase"] for f in e8} == {0, 1, 2, 3, 4} == {f["phase"] for f in e8 if f["at_seam"]}
    mixed = [c for c in E.cases("cuts") if "/mixed/" in c[0]]
    seam = facts["cuts"][-1]["seam"]
    assert [c[2] for c in mixed] == list(range(seam - 20, seam + 20)) and 2 * E.W < seam < len(E.mixed_stream())
    # lines: the whole stream is good, every call / jump cut fails, among the rc lengths both happen
    flat = collections.defaultdict(list)
    for f in facts["lines"]:
        for k, v in f.items():
            flat[k].append(v)
    assert flat["whole"] == [B.OK] and flat["call"] == [B.ERR_RESULT] * 80 == flat["jump"]
    assert len(flat["rc"]) == 66 and set(flat["rc"]) == {B.OK, B.ERR_RESULT}
    _, (main, call, jump, rc) = E.lines_streams()
    assert 64 <= len(rc) <= 69 and len(call) >= 500 and len(jump) >= 500
    assert flat["rc"] == [B.ERR_RESULT] * (len(rc) - 4) + [B.OK] * (70 - len(rc))     # the decoder asks for the stream's last byte
    # seam: each opcode at each window, converted and kept
    assert sum(f["converted"] for f in facts["seam"]) == 6 + 2 and len(facts["seam"]) == 14


def test_rounds_fail_two_of_seven():
    items = E.rounds(ROUNDS)
    assert len(items) == ROUNDS and len({id(it) for it in items}) == 7 * E.ROUND_VARIANTS
    for i, (st4, n, data) in enumerate(items):
        st, out = B.decode(*st4, n)
        kind = E.ROUND_KINDS[i % 7]
        assert (st == B.OK) == (data is not None) == (kind not in ("call-cut", "no-main")), (i, kind)
        if st == B.OK:
            assert out == data and len(data) == n, (i, kind)
        assert (n == 0) == (kind == "no-room") and (len(st4[0]) == 0) == (kind == "no-main"), (i, kind)
        assert kind == "two-windows" or 5 <= n <= 60 or kind == "no-room", (i, kind, n)
        if kind == "two-windows":
            assert E.W < len(st4[0]) <= 2 * E.W and 1100 <= n <= 1200
        if kind == "quiet":
            assert not E.main_candidates(st4[0]) and not st4[1] and not st4[2]
        if kind == "dense":
            assert len(st4[1]) >= 4
        if kind == "call-cut":   # whole, the streams are good: the item fails by the one to four bytes its call stream lacks
            assert B.decode(st4[0], st4[1] + bytes(4), st4[2], st4[3], n)[0] == B.OK
            assert B.decode(st4[0], st4[1] + bytes(4 - len(st4[1]) % 4)[:-1], st4[2], st4[3], n)[0] == B.ERR_RESULT
        if kind == "trap":
            assert len(E.main_candidates(st4[0])) == 1 and len(st4[1]) == 4 == len(st4[2])
    for lo in range(0, ROUNDS - 6):
        assert sum(it[2] is None for it in items[lo:lo + 7]) == 2


def test_host_merge_equals_the_reference(judged, xlz_so):
    for name, st4, n, _ in E.cases():
        st, out = judged[name]
        try:
            got = (B.OK, lzma_amd.bcj2_host(*st4, n))
        except lzma_amd.LzmaError as e:
            got = (e.status, None)
        assert got[0] == st == (lzma_amd.OK if st == B.OK else lzma_amd.ERR_RESULT), name
        assert st != B.OK or got[1] == out, name


def _build(tmp, flags, tag):
    exe = str(tmp / ("bcj2_dev_selftest" + tag))
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-I", os.path.join(ROOT, "lzma_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "bcj2_dev_selftest.cpp"), "-o", exe])
    return exe


def _merge_list(exe, tmp, jobs):
    """jobs: [(name, the four streams, out_len, residue, keep, (status, bytes))] through --merge-list in one run"""
    with open(tmp / "list.txt", "w") as lst, open(tmp / "in.bin", "wb") as blob:
        for _, st4, n, res, keep, _ in jobs:
            lst.write("%d %d %d %d %d %d %d\n" % (len(st4[0]), len(st4[1]), len(st4[2]), len(st4[3]), n, res, keep))
            blob.write(b"".join(st4))
    run = subprocess.run([exe, "--merge-list", str(tmp / "list.txt"), str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True,
                         text=True, timeout=600)
    with open(tmp / "out.bin", "rb") as got:
        for name, _, n, res, _, (st, out) in jobs:
            assert got.read(1) == (b"\0" if st == B.OK else b"\1"), (name, res)
            if st == B.OK:
                assert got.read(n) == out, (name, res)
        assert got.read(1) == b""
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.strip().endswith("%d items, 0 failures" % len(jobs))


def _jobs(judged):
    jobs = [(name, st4, n, E.residue(name), 0, judged[name]) for name, st4, n, _ in E.cases()]
    for i, (st4, n, data) in enumerate(E.rounds(ROUNDS)):   # one Wave from item to item: what a workgroup carries along
        jobs.append(("rounds/%d/%s" % (i, E.ROUND_KINDS[i % 7]), st4, n, (5 * i + 1) % 16, 1 if i else 0,
                     (B.OK, data) if data is not None else (B.ERR_RESULT, b"")))
    return jobs


def test_lane_scheme_equals_the_reference(judged, tmp_path):
    _merge_list(_build(tmp_path, ["-O2", "-Wall", "-Werror"], ""), tmp_path, _jobs(judged))


def test_lane_scheme_under_the_sanitizers(judged, tmp_path):
    """the same list through the same stand-alone program built with AddressSanitizer and UBSan: every stream lies in a heap
    block of exactly its length rounded up to 16"""
    _merge_list(_build(tmp_path, ["-O1", "-g", "-Wall", "-Werror"] + SAN, "_san"), tmp_path, _jobs(judged))
