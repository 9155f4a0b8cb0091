"""GPU: many .xz files as one batch, each with a status of its own (xlz_xz_decode_many / xlz_xz_decode_many_device;
DESIGN.md section 3.16).  The judge for bytes is liblzma through Python; the judge for status, out_len and unverified is
the single-file front-end (xlz_xz_decode / xlz_xz_decode_device) on the same context, file by file.  The files
(tests/xz_many_files.py) are small on purpose: a block of 1 byte, one of 16385 (past the 16 KiB pack tile), the 14 blocks
of xz_ranges_files.checked() on the edges of the 16-byte lane and the 256-byte arena alignment, and damaged ones."""
import ctypes
import lzma
import os
import sys

import pytest

import lzma_amd
from lzma_amd import LzmaError
from lzma_amd import _native as N

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xz_chains  # noqa: E402
import xz_many_files as M  # noqa: E402
import xz_ranges_files as X  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 64


def _torch():
    import torch
    return torch


def _filled(n):
    torch = _torch()
    t = torch.full((max(n, 1),), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def _bytes(t):
    return t.cpu().numpy().tobytes()


@pytest.fixture
def modes(ctx):
    """set(check mode, filter mode) for the test, both back to 0 behind it"""
    def set_modes(check, flt):
        ctx.set_check_mode(check)
        ctx.set_filter_mode(flt)
    yield set_modes
    ctx.set_check_mode(0)
    ctx.set_filter_mode(0)


_SINGLE = {}


def _single(ctx, name, data, cap, device):
    """the single-file call's (status, out_len, unverified), once per (file, room, form, modes of the context)"""
    key = (name, cap, device, ctx.check_mode(), ctx.filter_mode())
    if key not in _SINGLE:
        _SINGLE[key] = M.single(ctx, data, cap, device=device)[:3]
    return _SINGLE[key]


def _seven():
    """(name, file, decoded): the six good files and, for filter mode 1, the chains file"""
    return [(k, f, p) for k, (f, p) in M.good().items()] + [("chained", *X.chained())]


def _run(ctx, files, windows, device, verify=True):
    """one many-call over [(name, file, ...)] with the windows given, into a destination filled with 0xA5 ->
    ([(status, out_len, unverified)], the destination's bytes afterwards)"""
    cap = max([GUARD] + [o + c for o, c in windows if c]) + GUARD
    datas = [f[1] for f in files]
    if device:
        t = _filled(cap)
        res = lzma_amd.xz_decode_many_device(ctx, datas, t.data_ptr(), cap, windows, verify=verify)
        return res, _bytes(t)
    out = bytearray([FILL]) * cap
    res = lzma_amd.xz_decode_many_into(ctx, datas, out, windows, verify=verify)
    return res, bytes(out)


def _back_to_back(files, start=GUARD, gap=0, extra=0, align=1):
    """windows of the decoded sizes + extra, one behind the other from `start` with `gap` bytes between them"""
    w, at = [], start
    for f in files:
        at = (at + align - 1) // align * align
        w.append((at, len(f[2]) + extra))
        at += len(f[2]) + extra + gap
    return w


@pytest.mark.parametrize("form", ["host_check_mode_0", "host_check_mode_1", "host_check_mode_2", "device"])
def test_seven_files_equal_the_single_file_call(ctx, modes, form):
    device = form == "device"
    modes(0 if device else int(form[-1]), 1)
    files = _seven()
    assert [len(lzma_amd.xz_index_chains(f[1])[0]) for f in files] == [1, 1, 14, 1, 3, 0, 14]
    windows = _back_to_back(files)
    res, got = _run(ctx, files, windows, device)
    # (the call's statistics, before the single-file calls below start the context's over)
    ms, flt, chk, pk = ctx.last_xz_many_stats(), ctx.last_filter_stats(), ctx.last_check_stats(), ctx.last_pack_stats()
    for (name, data, plain), (off, cap), r in zip(files, windows, res):
        assert r == _single(ctx, name, data, cap, device), name
        assert r == (N.OK, len(plain), 2 if name == "reserved" else 0), name
        assert got[off:off + cap] == plain, name  # (lzma.decompress, stream by stream)
    assert got[:GUARD] == got[-GUARD:] == bytes([FILL]) * GUARD
    assert ms == {"files": 7, "failed_files": 0, "blocks": 34, "comp_bytes": sum(b["comp_len"] for f in files for b in lzma_amd.xz_index_chains(f[1])[0]),
                  "decoded_bytes": sum(len(f[2]) for f in files)}
    assert flt["device_steps"] + flt["host_steps"] == 3  # Delta, ARM and x86 of the chains file
    if form == "host_check_mode_0":
        assert chk["device_ranges"] + chk["host_ranges"] == 0        # (host threads inside the front-end: not the stage's)
    else:
        # every block with a known check, none of them empty: 1 + 1 + 14 + 0 + 1 + 0 + 14
        assert chk["device_ranges"] + chk["host_ranges"] + chk["empty_ranges"] == 31
    if device:
        assert (pk["launches"], pk["items"], pk["bytes"]) == (1, 34, ms["decoded_bytes"])


def _isolation_files():
    bad = M.bad()
    good = [(k, f, p) for k, (f, p) in M.good().items()]
    short = ("short_window", *M.good()["crc32_16385"])
    files = good[:2] + [("bad_crc", bad["bad_crc"], bytes(2048))] + good[2:4] + [("bad_chunk", bad["bad_chunk"], bytes(2048)),
                                                                                    ("cut", bad["cut"], bytes(100))]
    files += good[4:] + [("chained", *X.chained()), short]
    return files


@pytest.mark.parametrize("form", ["host_check_mode_0", "host_check_mode_2", "device"])
def test_a_bad_file_fails_alone(ctx, modes, form):
    device = form == "device"
    modes(0 if device else int(form[-1]), 0)
    files = _isolation_files()
    windows = _back_to_back(files, gap=5)
    windows[-1] = (windows[-1][0], windows[-1][1] - 1)  # one byte short of what the index announces
    res, got = _run(ctx, files, windows, device)        # (the call itself is XLZ_OK: the wrapper raises otherwise)
    bad_names = {"bad_crc", "bad_chunk", "cut", "chained", "short_window"}
    for (name, data, plain), (off, cap), r in zip(files, windows, res):
        assert r == _single(ctx, name, data, cap, device), name
        if name in bad_names:
            assert r[0] < 0 and r[1:] == (0, 0), name
        else:
            assert r[0] == N.OK and got[off:off + cap] == plain, name
        assert got[off + cap:off + cap + 5] == bytes([FILL]) * 5, name
    by_name = {f[0]: r[0] for f, r in zip(files, res)}
    assert by_name["bad_crc"] == N.ERR_RESULT and by_name["chained"] == N.ERR_UNSUPPORTED and by_name["short_window"] == N.ERR_OUT_CAP
    assert by_name["bad_chunk"] == N.ERR_PROPS and by_name["cut"] == M.index_status(M.bad()["cut"], False)[0] < 0
    ms = ctx.last_xz_many_stats()
    assert (ms["files"], ms["failed_files"]) == (len(files), 5)
    assert ms["blocks"] == 1 + 1 + 1 + 14 + 1 + 1 + 3 + 0  # (cut, chained and short_window put nothing into the batch)
    assert ms["decoded_bytes"] == sum(len(f[2]) for f in files if f[0] not in bad_names)
    # without verification the flipped byte is not seen, the damaged chunk header is
    res, got = _run(ctx, files, windows, device, verify=False)
    by_name = {f[0]: r for f, r in zip(files, res)}
    assert by_name["bad_crc"] == (N.OK, 2048, 0) and by_name["bad_chunk"][0] < 0 and by_name["reserved"] == (N.OK, len(X.reserved()[1]), 0)
    assert ctx.last_xz_many_stats()["failed_files"] == 4


@pytest.mark.parametrize("align", [1, 256])
@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_nothing_is_written_outside_the_windows(ctx, modes, device, align):
    """gaps between the windows and a guard at each end stay 0xA5; so do the bytes behind out_len inside the larger window
    of a good file.  align 1: every window starts at an odd offset; 256: at a multiple of the arena's alignment"""
    modes(0, 1)
    files = _seven() + [("bad_crc", M.bad()["bad_crc"], bytes(2048))]
    extra = 37
    windows = _back_to_back(files, start=GUARD + 1 if align == 1 else 256, gap=3, extra=extra, align=align)
    if align == 1:
        windows = [(o | 1, c) for o, c in windows]  # (gaps of 3 leave room for that)
    for (a, ca), (b, _) in zip(windows, windows[1:]):
        assert a + ca < b and a % align == 0
    res, got = _run(ctx, files, windows, device)
    want = bytearray([FILL]) * len(got)
    for (name, data, plain), (off, cap), r in zip(files, windows, res):
        if name == "bad_crc":
            assert r[0] == N.ERR_RESULT
            want[off:off + cap] = got[off:off + cap]  # (a failed file: the contents of its window are unspecified)
        else:
            assert r == (N.OK, len(plain), 2 if name == "reserved" else 0), name
            want[off:off + len(plain)] = plain
    assert got == bytes(want)
    assert len(got) == windows[-1][0] + windows[-1][1] + GUARD


def test_a_host_call_of_more_than_one_piece(ctx, modes):
    """the smallest count of 128 KiB files that decode_batch_plan cuts into pieces: the host form keeps xlz_decode_batch's
    pipeline, and the verdicts are still per file.  Five distinct files, named over and over."""
    modes(0, 0)
    size = 128 << 10
    plain = [bytes([k]) * size for k in range(3)]
    good = [lzma.compress(p, format=lzma.FORMAT_XZ, check=lzma.CHECK_CRC32, preset=0) for p in plain]
    assert all(len(lzma_amd.xz_index(g)[0]) == 1 for g in good)
    b0 = M.first_block(good[0])
    flipped = bytearray(good[0])
    flipped[b0["check_off"]] ^= 1           # the CRC32 field: the block decodes, the check fails
    chunk = bytearray(good[1])
    at = M.first_block(good[1])["comp_off"]
    assert chunk[at] >= 0xE0                # (an LZMA chunk with new properties: control, two sizes, the properties byte)
    chunk[at + 5] = 0xFF                    # properties no decoder accepts: the block's own status is XLZ_ERR_PROPS
    kinds = good + [bytes(flipped), bytes(chunk)]
    count = next(n for n in range(4096, 20000, 512) if len(lzma_amd.decode_batch_plan([size] * n)[0]) > 2)
    assert count == 8192                    # (8 k streams and 1 GiB: what plan_sub_batches asks for before it cuts)
    pick = [(i * 7 + i // 11) % 5 for i in range(count)]
    datas = [kinds[k] for k in pick]
    windows = [(i * size, size) for i in range(count)]
    out = bytearray(count * size)
    res = lzma_amd.xz_decode_many_into(ctx, datas, out, windows)
    assert ctx.last_call_stats()["sub_batches"] > 1
    want_bad = {3: _single(ctx, "piece_flipped", kinds[3], size, False), 4: _single(ctx, "piece_chunk", kinds[4], size, False)}
    assert want_bad[3] == (N.ERR_RESULT, 0, 0) and want_bad[4] == (N.ERR_PROPS, 0, 0)
    view = memoryview(out)
    for i, k in enumerate(pick):
        if k < 3:
            assert res[i] == (N.OK, size, 0) and view[i * size:(i + 1) * size] == plain[k], i
        else:
            assert res[i] == want_bad[k], i
    ms = ctx.last_xz_many_stats()
    assert (ms["files"], ms["blocks"], ms["failed_files"]) == (count, count, sum(k >= 3 for k in pick))


def test_64_files_are_one_batch_and_one_pack(ctx, modes):
    modes(0, 0)
    files = [("f%d" % i, lzma.compress(M.text(700 + 13 * i, i), format=lzma.FORMAT_XZ, check=lzma.CHECK_CRC64, preset=1), M.text(700 + 13 * i, i))
             for i in range(64)]
    windows = _back_to_back(files)
    res, got = _run(ctx, files, windows, True)
    assert res == [(N.OK, len(f[2]), 0) for f in files]
    assert all(got[o:o + c] == f[2] for f, (o, c) in zip(files, windows))
    ms = ctx.last_xz_many_stats()
    assert (ms["files"], ms["failed_files"], ms["blocks"]) == (64, 0, 64)
    pk = ctx.last_pack_stats()
    assert (pk["launches"], pk["items"], pk["bytes"]) == (1, 64, sum(len(f[2]) for f in files))
    chk = ctx.last_check_stats()
    assert chk["device_ranges"] + chk["host_ranges"] == 64


def test_the_same_file_twice_and_no_file_at_all(ctx, modes):
    modes(0, 0)
    name, data, plain = "checked", *X.checked()
    files = [(name, data, plain)] * 3
    for device in (True, False):
        res, got = _run(ctx, files, _back_to_back(files, gap=1), device)
        assert res == [(N.OK, len(plain), 0)] * 3
        for off, cap in _back_to_back(files, gap=1):
            assert got[off:off + cap] == plain
        assert ctx.last_xz_many_stats()["blocks"] == 42
    before = ctx.last_xz_many_stats()
    assert lzma_amd.xz_decode_many(ctx, []) == []
    assert lzma_amd.xz_decode_many_device(ctx, [], 0, 0, []) == []
    assert lzma_amd.xz_decode_many_into(ctx, [], bytearray(8), []) == []
    assert ctx.last_xz_many_stats() == before  # (a call of nothing makes no statistics)
    # the bytes form: a list of (bytes or None, status, unverified)
    bad = M.bad()["bad_crc"]
    got = lzma_amd.xz_decode_many(ctx, [data, bad, lzma.compress(b""), bytearray(data)])
    assert got == [(plain, N.OK, 0), (None, N.ERR_RESULT, 0), (b"", N.OK, 0), (plain, N.OK, 0)]
    with pytest.raises(LzmaError) as e:
        lzma_amd.xz_decode_many(ctx, [data, data], max_size=2 * len(plain) - 1)
    assert e.value.status == N.ERR_OUT_CAP
    # files that all fail before the batch: the call ran, nothing was launched
    res = lzma_amd.xz_decode_many_into(ctx, [data[:-1], b""], bytearray(8), [(0, 4), (4, 4)])
    assert [r[0] < 0 for r in res] == [True, True]
    ms = ctx.last_xz_many_stats()
    assert (ms["files"], ms["failed_files"], ms["blocks"]) == (2, 2, 0)
    assert ctx.last_pack_stats()["items"] == 0


def test_tensor_form(ctx, modes):
    torch = _torch()
    modes(0, 1)
    files = _seven() + [("bad_crc", M.bad()["bad_crc"], None)]
    datas = [f[1] for f in files]
    for align in (1, 256):
        t, res = lzma_amd.xz_decode_many_tensor(ctx, datas, align=align)
        laid, total = lzma_amd.xz_many_layout(datas, ctx=ctx, align=align)
        assert isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.device == torch.device("cuda", 0) and t.shape == (total,)
        got = _bytes(t)
        for (name, data, plain), (off, n, st, nu), (want_off, _, _) in zip(files, res, laid):
            assert off == want_off and off % align == 0
            if name == "bad_crc":
                assert (st, n) == (N.ERR_RESULT, 0)
            else:
                assert (st, n, nu) == (N.OK, len(plain), 2 if name == "reserved" else 0) and got[off:off + n] == plain, name
    total = lzma_amd.xz_many_layout(datas, ctx=ctx)[1]
    out = _filled(total + 100)
    t, res = lzma_amd.xz_decode_many_tensor(ctx, datas, out=out)
    assert t.data_ptr() == out.data_ptr() and _bytes(out)[total:] == bytes([FILL]) * 100
    assert [r[2] for r in res] == [N.OK] * 7 + [N.ERR_RESULT]
    with pytest.raises(LzmaError) as e:
        lzma_amd.xz_decode_many_tensor(ctx, datas, out=torch.empty(total - 1, dtype=torch.uint8, device="cuda"))
    assert e.value.status == lzma_amd.ERR_OUT_CAP
    with pytest.raises(ValueError):
        lzma_amd.xz_decode_many_tensor(ctx, datas, out=torch.empty(total, dtype=torch.int8, device="cuda"))


def test_argument_errors_on_a_live_context(ctx, modes):
    """what the CPU tests show with a context that is none, on a real one: refused, nothing written, no statistics made;
    a destination that is host memory; and windows of no bytes, which overlap nothing"""
    modes(0, 0)
    data, plain = M.good()["crc32_16385"]
    empty = lzma.compress(b"")
    lzma_amd.xz_decode_many(ctx, [data])
    before = (ctx.last_xz_many_stats(), ctx.last_pack_stats(), ctx.last_check_stats())
    t = _filled(40000)
    for windows in ([(0, 16385), (16384, 16385)], [(30000, 16385), (0, 16385)]):
        with pytest.raises(LzmaError) as e:
            lzma_amd.xz_decode_many_device(ctx, [data, data], t.data_ptr(), 40000, windows)
        assert e.value.status == N.ERR_BAD_ARG
    host = ctypes.create_string_buffer(20000)
    with pytest.raises(LzmaError) as e:
        lzma_amd.xz_decode_many_device(ctx, [data], ctypes.addressof(host), 20000, [(0, 16385)])
    assert e.value.status == N.ERR_BAD_ARG and host.raw == bytes(20000)
    assert _bytes(t) == bytes([FILL]) * 40000
    assert (ctx.last_xz_many_stats(), ctx.last_pack_stats(), ctx.last_check_stats()) == before
    # empty files with windows of no bytes inside another file's window, at its end and far outside the destination
    res = lzma_amd.xz_decode_many_device(ctx, [empty, data, empty, empty], t.data_ptr(), 40000, [(100, 0), (64, 16385), (64 + 16385, 0), (1 << 63, 0)])
    assert res == [(N.OK, 0, 0), (N.OK, 16385, 0), (N.OK, 0, 0), (N.OK, 0, 0)]
    got = _bytes(t)
    assert got[64:64 + 16385] == plain and got[:64] == bytes([FILL]) * 64 and got[64 + 16385:] == bytes([FILL]) * (40000 - 64 - 16385)
    # ... and so does a file whose blocks hold no bytes (two of them, CRC64 of nothing each)
    hollow = xz_chains.stream([(b"", [X.L2]), (b"", [X.L2])])
    assert lzma.decompress(hollow) == b"" and len(lzma_amd.xz_index(hollow)[0]) == 2
    windows = [(1 << 63, 0), (64, 16385), ((1 << 64) - 1, 0)]
    assert lzma_amd.xz_decode_many_device(ctx, [hollow, data, hollow], t.data_ptr(), 40000, windows) == [(N.OK, 0, 0), (N.OK, 16385, 0), (N.OK, 0, 0)]
    out = bytearray([FILL]) * 40000
    assert lzma_amd.xz_decode_many_into(ctx, [hollow, data, hollow], out, windows) == [(N.OK, 0, 0), (N.OK, 16385, 0), (N.OK, 0, 0)]
    assert bytes(out) == got == _bytes(t)
    assert ctx.last_xz_many_stats()["blocks"] == 5
