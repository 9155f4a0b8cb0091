"""CPU: the raw-deflate decoder of lzma_amd/csrc/xlz_inflate_dev.h without a GPU.  The judge everywhere is Python's zlib
(tests/inflate_edges.py: judge).  Every crafted case BITES -- zlib alone puts it in the class its name says --; then every
case through the library's serial decoder (lzma_amd.inflate_host) and through the g++ lane scheme
(tests/c/inflate_dev_selftest.cpp --inflate-list: the wave scheme lane by lane, twice with different bytes behind the
input's end, and the serial twin, compared with each other inside the program), built plain and with AddressSanitizer
and UBSan; then 20 000 seeded mutations through inflate_host and 4 000 of them through the sanitizer build.  Compared:
the class of the status, and for OK the bytes and the input bytes used."""
import collections
import os
import subprocess

import pytest

import inflate_edges as E
import lzma_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
CLASS = {lzma_amd.OK: E.OK, lzma_amd.ERR_RESULT: E.RESULT, lzma_amd.ERR_UNEXPECTED_EOF: E.EOF, lzma_amd.ERR_OUT_CAP: E.OUT_CAP}
CLASS_BYTE = {0: E.OK, 1: E.RESULT, 2: E.EOF, 3: E.OUT_CAP}
COUNTS = {"block": 28, "len": 51, "dist": 61, "copy": 36, "table": 28, "input": 37, "output": 40, "grace": 12}


def test_totals():
    cs = E.cases()
    assert dict(collections.Counter(E.family(c) for c in cs)) == COUNTS
    assert len({c[0] for c in cs}) == len(cs) == sum(COUNTS.values())
    assert {c[3] for c in cs} == {E.OK, E.RESULT, E.EOF, E.OUT_CAP}
    assert all(c[0].endswith(":" + c[3]) for c in cs)
    assert {c[4] for c in cs} == set(range(16)) and sum(c[4] == 5 for c in cs) > 100
    assert sum(len(c[1]) for c in cs) < 600_000


def test_every_case_bites():
    names = {c[0] for c in E.cases()}
    for name, data, cap, cls, _ in E.cases():
        got, out, used = E.judge(data, cap)
        assert got == cls, name
        if cls == E.OK:
            assert len(out) <= cap and 0 < used <= len(data), name
    # the edges the list is made for, by name
    for s in range(257, 286):
        assert sum(n.startswith("len/symbol-%d-" % s) for n in names) >= 1
    assert {"len/symbol-284-length-258:ok", "len/symbol-285-length-258:ok"} <= names
    for s in range(30):
        assert sum(n.startswith("dist/symbol-%d-" % s) for n in names) >= 1
    assert "dist/symbol-29-distance-32768-of-32768:ok" in names and "dist/32768-of-32767:result" in names
    for d in (1, 2, 3, 63, 64, 65):
        for n in (3, 63, 64, 65, 258):
            assert "copy/distance-%d-length-%d:ok" % (d, n) in names
    assert sum(n.startswith("input/dynamic-block-cut-at-") for n in names) >= 12 and "input/dynamic-block-cut-at-0:eof" in names
    # a far distance is what zlib's own deflate never writes: the crafted streams are needed
    far = [c for c in E.cases() if c[0].startswith("dist/symbol-29-distance-32768")][0]
    assert len(E.judge(far[1], far[2])[1]) == 32771


def _host(data, cap):
    try:
        out, used = lzma_amd.inflate_host(data, cap)
        return E.OK, out, used
    except lzma_amd.LzmaError as e:
        return CLASS[e.status], None, None


def test_inflate_host_equals_zlib_on_every_case(xlz_so):
    for name, data, cap, cls, _ in E.cases():
        assert _host(data, cap) == E.judge(data, cap), name


def test_inflate_host_equals_zlib_on_20000_mutations(xlz_so):
    seen = collections.Counter()
    for k, (data, cap) in enumerate(E.mutations(20000, 2024)):
        want = E.judge(data, cap)
        assert _host(data, cap) == want, (k, len(data), cap)
        seen[want[0]] += 1
    assert all(seen[c] >= 1000 for c in (E.OK, E.RESULT, E.EOF)) and seen[E.OUT_CAP] >= 100, seen


def _build(tmp, flags, tag):
    exe = str(tmp / ("inflate_dev_selftest" + tag))
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-I", os.path.join(ROOT, "lzma_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "inflate_dev_selftest.cpp"), "-o", exe])
    return exe


def _inflate_list(exe, tmp, jobs):
    """jobs: [(name, stream, out_cap, residue)] through --inflate-list in one run, each compared with the judge"""
    with open(tmp / "list.txt", "w") as lst, open(tmp / "in.bin", "wb") as blob:
        for _, data, cap, res in jobs:
            lst.write("%d %d %d\n" % (len(data), cap, res))
            blob.write(data)
    run = subprocess.run([exe, "--inflate-list", str(tmp / "list.txt"), str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True,
                         text=True, timeout=900)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.strip().endswith("%d items, 0 failures" % len(jobs))
    with open(tmp / "out.bin", "rb") as got:
        for name, data, cap, res in jobs:
            cls, out, used = E.judge(data, cap)
            assert CLASS_BYTE[got.read(1)[0]] == cls, (name, res)
            if cls == E.OK:
                assert int.from_bytes(got.read(4), "little") == used, (name, res)
                assert got.read(len(out)) == out, (name, res)
        assert got.read(1) == b""


def _jobs():
    jobs = [(name, data, cap, res) for name, data, cap, _, res in E.cases()]
    jobs += [("mutation %d" % k, data, cap, (7 * k) % 16) for k, (data, cap) in enumerate(E.mutations(4000, 2024))]
    return jobs


def test_the_selftest_speaks_for_itself(tmp_path):
    run = subprocess.run([_build(tmp_path, ["-O2", "-Wall", "-Werror"], "")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().endswith("comparisons, 0 failures"), run.stdout[-2000:]


def test_lane_scheme_equals_zlib(tmp_path):
    _inflate_list(_build(tmp_path, ["-O2", "-Wall", "-Werror"], ""), tmp_path, _jobs())


def test_lane_scheme_under_the_sanitizers(tmp_path):
    """the same list through the same stand-alone program built with AddressSanitizer and UBSan: every input lies in a heap
    block of exactly its length rounded up to 16, every destination in one of exactly residue + out_cap bytes"""
    _inflate_list(_build(tmp_path, ["-O1", "-g", "-Wall", "-Werror"] + SAN, "_san"), tmp_path, _jobs())
