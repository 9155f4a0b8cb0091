"""CPU: the device Adler-32's lane / row / segment / fold scheme (lzma_amd/csrc/xlz_adler_dev.h) run lane by lane by a g++
program (tests/c/adler_dev_selftest.cpp) over the edge list of tests/adler_edges.py, judged by zlib.adler32 -- built
plain, and as a stand-alone program with the address and undefined-behaviour sanitizers, which also see every range run
over a heap block of exactly its bytes.  And xlz_adler32_host / xlz_adler32_combine against zlib on random splits."""
import os
import random
import subprocess
import zlib

import pytest

import adler_edges as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = {"plain": ["-O2"], "sanitizers": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}


@pytest.fixture(scope="module")
def edge_list():
    buf, rs = E.buffer(), E.ranges()
    return buf, rs, E.expected(buf, rs)


def test_every_named_edge_occurs(edge_list):
    _, rs, _ = edge_list
    seen = set()
    for _, _, names in rs:
        seen |= names
    assert sorted(seen) == E.EDGES
    assert E.SEG == 131072 and max(ln for _, ln, _ in rs) > 2 * E.DEFERRAL
    header = open(os.path.join(ROOT, "lzma_amd", "csrc", "xlz_adler_dev.h")).read()
    assert "kMaxLaneRows = %d" % E.MAX_LANE_ROWS in header  # (the bound the list is built around is the one the header states)


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_the_scheme_on_the_cpu(tmp_path, edge_list, build):
    buf, rs, want = edge_list
    exe = str(tmp_path / "adler_dev_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + FLAGS[build] + ["-I", os.path.join(ROOT, "lzma_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "adler_dev_selftest.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)   # the built-in sweep
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout[-3000:] + run.stderr[-3000:]
    (tmp_path / "arena").write_bytes(buf)
    (tmp_path / "list").write_text("".join("%d %d\n" % (off, ln) for off, ln, _ in rs))
    run = subprocess.run([exe, "--list", str(tmp_path / "list"), str(tmp_path / "arena"), str(tmp_path / "out")], capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout[-3000:] + run.stderr[-3000:]
    got = [int(x, 16) for x in (tmp_path / "out").read_text().split()]
    assert len(got) == len(rs)
    bad = [(rs[k][0], rs[k][1], sorted(rs[k][2]), hex(got[k]), hex(want[k])) for k in range(len(rs)) if got[k] != want[k]]
    assert not bad, bad[:10]


def test_host_digest_and_combine_against_zlib(xlz_so):
    from lzma_amd import gz
    r = random.Random("adler-host")
    assert gz.adler32_host(b"") == 1 == zlib.adler32(b"") and gz.adler32_combine(1, 1, 0) == 1
    for k in range(300):
        n = r.choice((0, 1, 2, 5551, 5552, 5553, 65521, r.randrange(200000)))
        data = r.choice((r.randbytes(n), b"\xff" * n, b"\0" * n))
        cut = r.randrange(n + 1)
        whole, a, b = zlib.adler32(data), zlib.adler32(data[:cut]), zlib.adler32(data[cut:])
        assert gz.adler32_host(data) == whole
        assert gz.adler32_host(data[cut:], adler=a) == whole
        assert gz.adler32_combine(a, b, n - cut) == whole
    big = b"\xfe" * (1 << 20)   # a len_b far above 65521, put together from halves
    half = zlib.adler32(big)
    assert gz.adler32_combine(half, half, len(big)) == zlib.adler32(big + big)
