"""GPU: .bz2 files as one batch (lzma_amd/csrc/xlz_bz2.hip) through lzma_amd.bzip2.  ONE call over the whole crowd of
tests/bz2_files.py -- block shapes, files, defects, cuts and 2000 mutations, some 2400 files -- into a destination of 0xA5
with guard bytes between the windows and a window at every residue modulo 16.  Every status, out_len, in_consumed and byte
is compared with bzip2.decode_host (the serial twin) and with the yardstick, Python's bz2.  Then: every failing file alone;
windows one byte short and empty; three rounds forced by a small scratch budget; bz2 mode 2, the host form, the tensor form
and a destination that is 5 modulo 16; the statistics.  Every file is bounds-checked data: a damaged one is a status,
nothing here reads or writes out of range."""
import numpy as np
import pytest
import torch   # (before libxlz.so is loaded: torch brings its own HIP runtime, which must be the one that initialises the device)

import bz2_files as F
from lzma_amd import bzip2

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xA5, 48


def same_class(got, want):
    return got == want or (want == F.ERR_RESULT and got == F.ERR_UNSUPPORTED)


@pytest.fixture(scope="module")
def crowd():
    """-> [(name, file, cap, (status, bytes, in_consumed) of the yardstick)]; an accepted file's window is exact"""
    return [(name, f, len(ex[1]) if ex[0] == F.OK else 5000, ex) for (name, f), ex in zip(F.cases(), F.expected())]


@pytest.fixture(scope="module")
def twin(crowd, xlz_so):
    """what bzip2.decode_host says of every file: computed once, never changed"""
    return [bzip2.decode_host(f, cap) for _, f, cap, _ in crowd]


def _windows(crowd):
    windows, at = [], GUARD
    for k, (_, _, cap, _) in enumerate(crowd):
        at += (5 * k) % 16   # (every residue modulo 16)
        windows.append((at, cap))
        at += cap + GUARD
    return windows, at


def _compare(crowd, twin, windows, res, image, what, untouched=()):
    """res against the twin (all five numbers and the bytes) and the yardstick; everything outside the windows, and the
    windows of the files in `untouched`, still holds the fill"""
    image = np.frombuffer(image, dtype=np.uint8)
    covered = np.zeros(len(image), dtype=bool)
    for k, ((name, f, cap, ex), (off, _), r) in enumerate(zip(crowd, windows, res)):
        status, out_len, used, blocks, streams = r
        out = image[off:off + out_len].tobytes() if status == F.OK else None
        assert (out,) + tuple(r) == twin[k], (what, name, cap, r, twin[k][1:])
        if ex is not None:
            assert same_class(status, ex[0]), (what, name, r, ex[0])
            if ex[0] == F.OK:
                assert out == ex[1] and used == ex[2], (what, name)
        if status != F.OK and status != F.ERR_OUT_CAP:
            assert out_len == 0 and used == 0
        if k not in untouched:
            covered[off:off + cap] = True
    assert bool((image[~covered] == FILL).all()), what


def _device_call(ctx, crowd, shift=0, verify=True):
    windows, total = _windows(crowd)
    dst = torch.full((total + 16,), FILL, dtype=torch.uint8, device="cuda")
    res = bzip2.decode_many_device(ctx, [f for _, f, _, _ in crowd], dst.data_ptr() + shift, total, windows, verify=verify)
    return windows, res, dst.cpu().numpy().tobytes()[shift:shift + total]


def test_one_call_over_the_whole_crowd(ctx, crowd, twin):
    assert len(crowd) >= 2400
    windows, res, image = _device_call(ctx, crowd)
    _compare(crowd, twin, windows, res, image, "device")
    s = bzip2.last_stats(ctx)
    assert s["files"] == len(crowd) and s["failed_files"] == sum(1 for t in twin if t[1] != F.OK)
    assert s["rounds"] == 1 and s["uploads"] == 1 and s["host_blocks"] == 2 and s["discarded_blocks"] >= 1   # (the two marks_avoided blocks are the host's)
    assert s["device_blocks"] + s["host_blocks"] == sum(t[4] for t in twin if t[1] == F.OK) > 700
    assert s["chain_blocks"] + s["discarded_blocks"] <= s["candidates"]
    assert s["symbols_ms"] > 0 and s["walk_ms"] > 0 and s["expand_ms"] > 0 and s["crc_ms"] > 0


def test_every_failing_file_alone_gives_the_same_result(ctx, crowd, twin):
    seen = set()
    for k, (name, f, cap, ex) in enumerate(crowd):
        if twin[k][1] == F.OK or f in seen:
            continue
        seen.add(f)
        w, r, image = _device_call(ctx, [crowd[k]])
        _compare([crowd[k]], [twin[k]], w, r, image, "alone: " + name)
    assert len(seen) > 1000


def test_a_window_one_byte_short_and_an_empty_one_are_out_cap_with_the_true_size(ctx, crowd):
    by = {c[0]: c for c in crowd}
    short = []
    for name in ("one_block", "blocks15_seed31", "two_streams", "then_damaged", "then_junk_magic", "x260", "full_level1", "levels_differ"):
        _, f, cap, ex = by[name]
        short += [(name, f, cap - 1, None), (name, f, 0, None), (name, f, cap, ex)]
    windows, res, image = _device_call(ctx, short)
    tw = [bzip2.decode_host(f, cap) for _, f, cap, _ in short]
    _compare(short, tw, windows, res, image, "short", untouched={k for k, c in enumerate(short) if c[3] is None})
    for (name, f, cap, ex), r in zip(short, res):
        if ex is None:
            assert r == (F.ERR_OUT_CAP, len(by[name][3][1]), 0, 0, 0), (name, cap, r)
        else:
            assert r[0] == F.OK
    # the retry with exact room, as bzip2.decompress does it
    assert bzip2.decompress(ctx, by["two_streams"][1], out_cap=3) == by["two_streams"][3][1]
    assert bzip2.decompress(ctx, by["blocks15_seed32"][1]) == by["blocks15_seed32"][3][1]


def test_three_rounds_give_the_same_results(ctx, crowd, twin):
    # files of level-1 streams: a candidate takes about 600 KB of scratch (levels_differ: one of 1.8 MB), some 150 of them
    idx, need = [], 0
    for k, (name, f, _, _) in enumerate(crowd):
        if name.startswith(("mut", "cut", "blocks15")) and name != "blocks15_seed33":
            continue
        if f[:4] != b"BZh1":
            continue
        idx.append(k)
        need += bzip2.probe(f)["candidates"] * (6 * 100000 + 1024)
    part, tw = [crowd[k] for k in idx], [twin[k] for k in idx]
    assert need > 80 * 600000
    windows, res1, image1 = _device_call(ctx, part)
    s1 = bzip2.last_stats(ctx)
    assert s1["rounds"] == 1
    # a budget of 0.4 of what they take in all is three rounds
    bzip2.set_scratch(ctx, int(0.4 * need))
    try:
        windows, res3, image3 = _device_call(ctx, part)
        s3 = bzip2.last_stats(ctx)
    finally:
        bzip2.set_scratch(ctx, 0)
    assert s3["rounds"] == 3 and s3["uploads"] == 1, s3
    assert res3 == res1
    _compare(part, tw, windows, res3, image3, "three rounds")
    assert s3["chain_blocks"] == s1["chain_blocks"] and s3["device_blocks"] == s1["device_blocks"]


def test_other_forms_mode_2_host_tensor_and_an_odd_pointer(ctx, crowd, twin):
    pick = [k for k, c in enumerate(crowd) if not c[0].startswith(("mut", "cut"))] + [k for k, c in enumerate(crowd) if c[0].startswith("mut")][:200]
    part, tw = [crowd[k] for k in pick], [twin[k] for k in pick]
    files = [f for _, f, _, _ in part]
    # a destination pointer that is 5 modulo 16
    windows, res, image = _device_call(ctx, part, shift=5)
    _compare(part, tw, windows, res, image, "pointer 5 mod 16")
    # bz2 mode 2: every block on host threads, uploaded
    bzip2.set_mode(ctx, bzip2.HOST_THREADS)
    try:
        windows, res2, image2 = _device_call(ctx, part)
        s = bzip2.last_stats(ctx)
    finally:
        bzip2.set_mode(ctx, bzip2.DEVICE)
    _compare(part, tw, windows, res2, image2, "mode 2")
    assert res2 == res and s["device_blocks"] == 0 and s["host_blocks"] == sum(t[4] for t in tw if t[1] == F.OK) and s["uploads"] == 0
    # the host form: into the caller's buffer, only the good files scattered
    windows, total = _windows(part)
    out = bytearray([FILL]) * total
    resh = bzip2.decode_many_into(ctx, files, out, windows)
    assert resh == res
    _compare(part, tw, windows, resh, bytes(out), "host form", untouched={k for k, t in enumerate(tw) if t[1] != F.OK})
    got = bzip2.decode_many(ctx, files[:40], caps=[c[2] for c in part[:40]])
    assert [g[:4] for g in got] == [t[:4] for t in tw[:40]]
    # the tensor form
    t, views, rest = bzip2.decode_many_tensor(ctx, files, caps=[c[2] for c in part], align=16)
    assert rest == res
    for v, tv in zip(views, tw):
        assert (v is None) == (tv[1] != F.OK) and (v is None or v.cpu().numpy().tobytes() == tv[0])


def test_stats_of_the_junk_with_magic_file(ctx, crowd):
    by = {c[0]: c for c in crowd}
    for name in ("then_junk_magic", "then_junk_magic_bits"):
        windows, res, image = _device_call(ctx, [by[name]])
        s = bzip2.last_stats(ctx)
        assert res[0][0] == F.OK and res[0][2] == by[name][3][2] < len(by[name][1])
        assert s["discarded_blocks"] >= 1 and s["uploads"] == 1 and s["candidates"] == 2 and s["chain_blocks"] == 1, (name, s)
    # a block whose successor vector avoids the marks is given up by the walk and decoded by the host's twin
    windows, res, image = _device_call(ctx, [by["marks_avoided"], by["one_block"]])
    s = bzip2.last_stats(ctx)
    assert [r[0] for r in res] == [F.OK, F.OK] and s["host_blocks"] == 1 and s["device_blocks"] == 1, s
    assert image[windows[0][0]:windows[0][0] + res[0][1]] == by["marks_avoided"][3][1]
    windows, res, image = _device_call(ctx, [by["levels_differ"]])
    s = bzip2.last_stats(ctx)
    assert res[0][0] == F.OK and s["host_blocks"] == 0 and s["device_blocks"] == s["chain_blocks"] == 3, s   # (each stream's size was seen)
