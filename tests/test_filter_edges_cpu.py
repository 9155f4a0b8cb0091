"""CPU: the crafted seam cases of tests/filter_edges.py, without a GPU.  For every case the library's serial filter
(lzma_amd.filter_host) and the g++ lane scheme (tests/c/filter_dev_selftest.cpp --apply-list) give liblzma's bytes, step by
step -- and, with liblzma alone, every case BITES: its single instruction converts exactly where it was put, its
must-not-convert bytes stay while a control converts, its x86 windows have no sync point, its Delta stream has the chunks
and groups it is named for.  The totals are asserted so that an edit cannot quietly thin the cases."""
import collections
import os
import re
import subprocess

import numpy as np
import pytest

import filter_edges as E
import filter_ref as R
import lzma_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def outputs():
    """per case: liblzma's bytes after every step.  A single step is undone by liblzma while it decodes the raw LZMA2 stream
    the GPU test uploads; the steps of a chain are applied one by one (filter_ref.apply), and the chained decode agrees."""
    outs = {}
    for c in E.cases():
        comp = E.compressed(c)
        assert E.liblzma(comp, []) == c.data, c.name
        final = E.liblzma(comp, c.steps)
        if len(c.steps) == 1:
            outs[c.name] = [final]
        else:
            seq, cur = [], c.data
            for f, p in c.steps:
                cur = R.apply(f, p, cur)
                seq.append(cur)
            assert seq[-1] == final, c.name
            outs[c.name] = seq
    return outs


def _step_inputs(c, outs):
    return [c.data] + outs[c.name][:-1]


def test_host_filter_equals_liblzma(outputs, xlz_so):
    for c in E.cases():
        for (f, p), src, want in zip(c.steps, _step_inputs(c, outputs), outputs[c.name]):
            assert lzma_amd.filter_host(f, p, src) == want, (c.name, f, p)


def test_lane_scheme_equals_liblzma(outputs, tmp_path):
    """every step of every case through the g++ program in one run: lanes, windows and chunks last to first, and the
    fixed-width lanes also with all loads in front of all stores, in both store orders"""
    exe = str(tmp_path / "filter_dev_selftest")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lzma_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "filter_dev_selftest.cpp"), "-o", exe])
    jobs = [(c.name, f, p, src, want) for c in E.cases()
            for (f, p), src, want in zip(c.steps, _step_inputs(c, outputs), outputs[c.name])]
    with open(tmp_path / "list.txt", "w") as lst, open(tmp_path / "in.bin", "wb") as blob:
        for _, f, p, src, _ in jobs:
            lst.write("%d %d %d\n" % (f, p, len(src)))
            blob.write(src)
    rc = subprocess.call([exe, "--apply-list", str(tmp_path / "list.txt"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    with open(tmp_path / "out.bin", "rb") as got:
        for name, f, p, src, want in jobs:
            assert got.read(len(src)) == want, (name, f, p)
        assert got.read(1) == b""
    assert rc == 0


def _diffs(a, b):
    assert len(a) == len(b)
    return np.flatnonzero(np.frombuffer(a, dtype=np.uint8) != np.frombuffer(b, dtype=np.uint8))


def _is_op(b):
    return (b & 0xFE) == 0xE8


def window_table(data):
    """the x86 window table restated: per 256-byte window the first position, relative to the window, that follows nine bytes
    without E8 / E9 (position 0 of the stream is one by itself), or None"""
    clean, run = [], 0
    for b in data:            # clean[p] = bytes without an opcode in front of p
        clean.append(run)
        run = 0 if _is_op(b) else run + 1
    table = []
    for lo in range(0, len(data), E.W):
        hits = [p - lo for p in range(lo, min(lo + E.W, len(data))) if p == 0 or clean[p] >= 9]
        table.append(hits[0] if hits else None)
    return table


def test_every_case_bites(outputs):
    for c in E.cases():
        pr, out = E.probes(c), outputs[c.name][-1]
        assert set(pr) & {"regions", "bands", "unchanged", "changed", "delta"}, c.name
        for key in ("regions", "bands"):   # a byte changes in every region, and none outside them
            if key in pr:
                assert pr[key], c.name
                d = _diffs(c.data, out)
                inside = np.zeros(len(d), dtype=bool)
                for lo, hi in pr[key]:
                    hit = (d >= lo) & (d < hi)
                    assert hit.any(), (c.name, lo, hi)
                    inside |= hit
                assert inside.all(), (c.name, d[~inside][:5])
        if "unchanged" in pr:
            steps, data = pr["unchanged"]
            assert out == c.data, c.name
            assert R.apply_steps(steps, data) != data, c.name
            assert len(data) >= len(c.data) and data != c.data and [f for f, _ in steps] == [f for f, _ in c.steps], c.name
        if "changed" in pr:
            for src, dst in zip(_step_inputs(c, outputs), outputs[c.name]):
                assert src != dst, c.name
            if c.name.startswith("thumb/alternating"):   # every pair of the chain converts
                assert len(_diffs(c.data, out)) >= len(c.data) // 4, c.name
        if "nosync" in pr:
            table = window_table(c.data)
            assert len(table) == (len(c.data) + E.W - 1) // E.W and table[0] == 0
            assert [j for j, s in enumerate(table) if s is None] == pr["nosync"]["windows"], c.name
            spans = [len(r) for r in E.runs_of(pr["nosync"]["windows"])]
            assert max(spans, default=0) == pr["nosync"]["span"], c.name
            # the table's entries are sync points: from there on liblzma alone gives what it gives inside the whole stream
            off = c.steps[0][1]
            marks = [j for j in range(1, len(table)) if table[j] is not None and (table[j - 1] is None or j + 1 == len(table))]
            for j in marks[:2]:
                at = j * E.W + table[j]
                assert R.apply(R.X86, (off + at) & 0xFFFFFFFF, c.data[at:]) == out[at:], (c.name, j)
        for key in ("made", "unmade"):
            a, b = (out, c.data) if key == "made" else (c.data, out)
            for at in pr.get(key, ()):
                assert a[at] == 0xE8 and not _is_op(b[at]), (c.name, key, at)
                edge = (at + 9) // E.W   # the window whose lookback holds the byte: its entry depends on which bytes are read
                assert window_table(c.data)[edge] != window_table(out)[edge], (c.name, key, at)
        if "state" in pr:   # without the dead opcodes in front of them the same calls convert to other bytes
            steps, ctl, at = pr["state"]
            ctl_out = R.apply_steps(steps, ctl)
            assert len(at) >= 4 and steps == c.steps
            for B in at:
                assert ctl[B:B + 5] == c.data[B:B + 5] and ctl_out[B + 1:B + 5] != ctl[B + 1:B + 5], (c.name, B)
                assert out[B + 1:B + 5] != ctl_out[B + 1:B + 5], (c.name, B)
        if "delta" in pr:
            d, n = c.steps[0][1], len(c.data)
            assert (out != c.data) == (n > d), c.name
            assert pr["delta"] == {"chunks": -(-n // E.C), "groups": -(-n // (E.C * E.G))}, c.name
            m = re.search(r"/chunks(\d+)\+5$", c.name)
            if m:
                assert pr["delta"]["chunks"] == int(m.group(1)) + 1 and pr["delta"]["groups"] == 1, c.name
    by = {c.name: c for c in E.cases()}
    assert E.probes(by["x86/nosync/257-windows-from-W-1/a"])["nosync"]["span"] >= 257
    assert E.probes(by["x86/nosync/257-windows-from-W-1/b"])["nosync"]["span"] >= 257
    assert E.probes(by["x86/nosync/256-windows/a"])["nosync"]["windows"] == list(range(2, 257))
    assert E.probes(by["x86/nosync/a-window-and-3/a"])["nosync"]["windows"] == [5]
    assert E.probes(by["x86/nosync/inside-a-window/b"])["nosync"]["windows"] == []
    G, C = E.G, E.C
    named = {G * C: (256, 1), G * C + 1: (257, 2), (G + 1) * C: (257, 2), (G + 1) * C + 1: (258, 2), (G + 8) * C + 5: (265, 2),
             (G + 9) * C + 5: (266, 2), (G + 10) * C: (266, 2), 2 * G * C + 3: (513, 3), 2 * G * C + C + 3: (514, 3)}
    for n, (chunks, groups) in named.items():
        for d in (3, 255):
            assert E.probes(by["delta/d%d/groups/len%d" % (d, n)])["delta"] == {"chunks": chunks, "groups": groups}
    assert sum("/groups/" in name for name in by) == 3 * len(named)


def test_background_holds_no_opcode():
    bg = bytes(E.background(3 * E.TB + 7, 1))
    for f in R.ALL:
        if f != R.DELTA:
            for p in R.OFFSETS:
                assert R.apply(f, p, bg) == bg, (f, p)


def test_totals():
    cs = E.cases()
    count, size = collections.Counter(E.kind(c) for c in cs), collections.Counter()
    for c in cs:
        size[E.kind(c)] += len(c.data)
        assert 1 <= len(c.steps) <= 3 and not any(lzma_amd.filter_host(f, p, b"") for f, p in c.steps)
    assert len({c.name for c in cs}) == len(cs)
    assert dict(count) == COUNTS, dict(count)
    assert dict(size) == BYTES, dict(size)
    assert len(E.alternating_batch()) == 36 and [len(b) for b in E.single_step_batches()] == [1, 1, 1]


COUNTS = {R.DELTA: 341, R.X86: 161,R.POWERPC: 289, R.IA64: 289, R.ARM: 289, R.ARMTHUMB: 94, R.SPARC: 289, "chain": 12}
BYTES = {R.DELTA: 149579810, R.X86: 8572060, R.POWERPC: 3393792, R.IA64: 3346176, R.ARM: 3393792, R.ARMTHUMB: 2363506, R.SPARC: 3393792,
         "chain": 873156}
