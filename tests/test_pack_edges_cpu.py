"""CPU: the crafted tables of tests/pack_edges.py, without a GPU.  Every probe restates portion / head / chunks / tail from
(src, dst, len) alone and asserts that the shapes a family is named for really occur -- every case bites -- and the totals
are asserted so that an edit cannot quietly thin the tables.  Then every table, at both misalignments of the destination
pointer, through the g++ tile / lane scheme (tests/c/pack_dev_selftest.cpp --pack-list: all tiles, against memcpy per item,
the whole destination and its guards compared), also built with AddressSanitizer and UBSan."""
import os
import subprocess

import pytest

import pack_edges as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
ROUND_TILES = 3 * 7 + 2

ITEMS = {"seam": 320 + 64, "chunks": 104 * 6, "empty": 9, "crowd": 16384 + 1024}
COUNTED = {"seam": {"seams": 320}, "chunks": {"shapes": 104, "whole_tiles": 6}, "empty": {"empty_tiles": 12}, "crowd": {"items": 17408}}


@pytest.fixture(scope="module")
def tables():
    out = [(f, mis) + E.plan(f, mis) for f in E.FAMILIES for mis in E.MIS]
    return out + [("rounds", mis) + E.rounds(ROUND_TILES, mis) for mis in E.MIS]


def test_every_table_bites(tables):
    assert [(f, mis) for f, mis, *_ in tables] == [(f, mis) for f in E.FAMILIES + ("rounds",) for mis in E.MIS]
    for f, mis, sizes, items, cap, probe in tables:
        assert sizes == E.SIZES and all(65536 <= n <= 204800 for n in sizes) and len(sizes) == 5
        assert all(0 <= off and 0 < n and off + n <= sizes[s] and 0 <= d and d + n <= cap for s, off, n, d in items), (f, mis)
        got = probe()
        if f == "rounds":
            assert got["tiles"] == ROUND_TILES == got["items"] and got["split_items"] == 7
        else:
            assert len(items) == ITEMS[f] and got == COUNTED[f], (f, mis, got)
        # the seams are where the KERNEL's tiles are: an item's place modulo a tile, in its coordinates, is the same at both
        # misalignments
        other = next(t for t in tables if t[0] == f and t[1] != mis)
        assert sorted((d + mis) % E.TILE for _, _, _, d in items) == sorted((d + other[1]) % E.TILE for _, _, _, d in other[3]), f
    assert len(E.chunk_shapes()) == 104 and {c for c, _, _ in E.chunk_shapes()} == set(E.CHUNK_COUNTS)
    assert sum(n for _, _, n, _ in E.rounds(3 * 8 * 256 + 1, 5)[1]) < 4 << 20


def test_expectation_of_a_small_table():
    """expect_pack on a table one can read: three items, one clipped, one empty"""
    plains = [bytes(range(100)), bytes(range(100, 200))]
    want, copied, st = E.expect_pack([(0, 10, 5, 3), (1, 90, 20, 16), (0, 100, 4, 40)], plains, 48, 10)
    assert copied == [5, 10, 0] and st == {"items": 2, "bytes": 15, "congruent_items": 1, "empty_items": 1}
    assert want == bytes([E.FILL]) * 3 + bytes(range(10, 15)) + bytes([E.FILL]) * 8 + bytes(range(190, 200)) + bytes([E.FILL]) * 22


def _run(tables, tmp, flags, tag):
    exe = str(tmp / ("pack_dev_selftest" + tag))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", os.path.join(ROOT, "lzma_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "pack_dev_selftest.cpp"), "-o", exe])
    with open(tmp / "list.txt", "w") as lst:
        for _, mis, sizes, items, cap, _ in tables:
            lst.write("%d %d %d %d\n%s\n" % (len(sizes), len(items), cap, mis, " ".join(map(str, sizes))))
            lst.write("".join("%d %d %d %d\n" % it for it in items))
    out = subprocess.run([exe, "--pack-list", str(tmp / "list.txt")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip().endswith("%d tables, 0 failures" % len(tables))


def test_lane_scheme_on_every_table(tables, tmp_path):
    _run(tables, tmp_path, ["-O2"], "")


def test_lane_scheme_under_the_sanitizers(tables, tmp_path):
    """the same list through the same stand-alone program built with AddressSanitizer and UBSan; the header's load helper
    asserts that every aligned load stays inside the arena"""
    _run(tables, tmp_path, ["-O1", "-g"] + SAN, "_san")
