"""GPU: the entries of a .zip archive as one batch (xlz_zip_extract / xlz_zip_extract_device).
The judge for bytes is Python's zipfile.read; the judge for statuses is the order include/xlz.h states plus the invariant
that an entry's result in a call of many equals its result alone.  The archives (tests/zip_files.py) are small on
purpose: entries of 0, 1, 15 .. 17, 255 .. 257, 16 383 .. 16 385 (the 16 KiB pack tile) and 70 001 bytes, payloads that
start at every offset modulo 16, and one defect per damaged entry."""
import io
import os
import random
import sys
import zipfile

import pytest

import lzma_amd
from lzma_amd import _native as N

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zip_files as Z  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 64


def _torch():
    import torch
    return torch


@pytest.fixture(scope="session", autouse=True)
def _torch_before_the_library():
    """torch finds no device once another HIP runtime has opened it in the process: where this file runs on its own, torch
    goes first (in the whole suite an earlier file has seen to it)"""
    _torch().cuda.init()


def _filled(n):
    torch = _torch()
    t = torch.full((max(n, 1),), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def _judge(arc):
    """zipfile's bytes per entry; None where zipfile cannot tell"""
    out = []
    with zipfile.ZipFile(io.BytesIO(arc)) as z:
        for zi in z.infolist():
            try:
                out.append(z.read(zi))
            except Exception:
                out.append(None)
    return out


def _windows(z, order, gap=3, extra=0):
    """wants with windows of size + extra from GUARD on, `gap` bytes between them -> (wants, cap)"""
    wants, at = [], GUARD
    for i in order:
        e = z.entries[i]
        size = 0 if e["is_dir"] else e["size"]
        wants.append((i, at, size + extra))
        at += size + extra + gap
    return wants, at + GUARD


def _run(ctx, z, wants, cap, device, verify=True):
    """one call into a destination filled with 0xA5 -> ([(status, out_len)], the destination's bytes afterwards)"""
    if device:
        t = _filled(cap)
        res = z.extract_device(ctx, wants, t.data_ptr(), cap, verify=verify)
        return res, t.cpu().numpy().tobytes()
    out = bytearray([FILL]) * cap
    res = z.extract_into(ctx, wants, out, verify=verify)
    return res, bytes(out)


def _untouched(got, wants, res, writable=()):
    """nothing is written outside the windows, nor behind out_len inside one; writable: the wants (by position) that failed
    by what is known only when their bytes lie in the window, which may therefore be written"""
    mask = bytearray(len(got))
    for k, ((i, off, cap), (st, n)) in enumerate(zip(wants, res)):
        keep = cap if k in writable else n
        mask[off:off + keep] = b"\x01" * keep
    return all(m or b == FILL for m, b in zip(mask, got))


def _check_good(z, wants, res, got, plain):
    for (i, off, cap), (st, n) in zip(wants, res):
        want = b"" if z.entries[i]["is_dir"] else plain[i]
        assert (st, n) == (N.OK, len(want)), (z.names[i], st, n)
        assert got[off:off + n] == want, z.names[i]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("order", ["archive", "shuffled_with_a_duplicate"])
def test_every_entry_of_the_mixed_archive(ctx, device, order):
    arc = Z.mixed()
    plain = _judge(arc)
    with lzma_amd.ZipFile(arc) as z:
        idx = [i for i, e in enumerate(z.entries) if e["method"] != 8]
        if order != "archive":
            random.Random(5).shuffle(idx)
            idx.insert(7, idx[2])
        wants, cap = _windows(z, idx, extra=5)
        res, got = _run(ctx, z, wants, cap, device)
        stats, pk, chk = ctx.last_zip_extract_stats(), ctx.last_pack_stats(), ctx.last_check_stats()
        _check_good(z, wants, res, got, plain)
        assert _untouched(got, wants, res)
        with_bytes = [i for i in idx if z.entries[i]["size"] and not z.entries[i]["is_dir"]]
        n_lzma = sum(z.entries[i]["method"] == 14 for i in with_bytes)
        assert stats == {"entries": len(idx), "empty_entries": len(idx) - len(with_bytes), "failed_entries": 0, "lzma_entries": n_lzma,
                         "stored_entries": len(with_bytes) - n_lzma, "comp_bytes": sum(z.entries[i]["comp_size"] for i in with_bytes),
                         "copied_bytes": sum(z.entries[i]["size"] for i in with_bytes), "stored_uploads": 1}
        assert pk["items"] == len(with_bytes) and pk["launches"] == 2 and pk["bytes"] == stats["copied_bytes"]
        assert chk["device_ranges"] == len(with_bytes) and chk["host_ranges"] == 0  # every CRC32 on the device


def test_both_end_marker_forms_give_the_same_bytes(ctx):
    arc, plains = Z.both_markers()
    with lzma_amd.ZipFile(arc) as z:
        assert [bool(e["flags"] & N.ZIP_ENTRY_END_MARKER) for e in z.entries] == [True, False] * len(plains)
        got = z.extract(ctx, range(len(z.entries)))
        for k, p in enumerate(plains):
            assert got[2 * k] == got[2 * k + 1] == (N.OK, p), k
        assert z.read(ctx, "n3") == plains[3]


def test_verify_and_check_mode_change_nothing_for_good_entries(ctx):
    arc = Z.mixed()
    with lzma_amd.ZipFile(arc) as z:
        idx = [i for i, e in enumerate(z.entries) if e["method"] != 8]
        wants, cap = _windows(z, idx)
        seen = []
        try:
            for mode in (0, 1):
                ctx.set_check_mode(mode)
                for verify in (True, False):
                    for device in (False, True):
                        seen.append(_run(ctx, z, wants, cap, device, verify=verify))
                    assert ctx.last_check_stats()["device_ranges"] == (ctx.last_zip_extract_stats()["lzma_entries"] +
                                                                       ctx.last_zip_extract_stats()["stored_entries"] if verify else 0)
        finally:
            ctx.set_check_mode(0)
        assert all(s == seen[0] for s in seen[1:])
        assert all(st == N.OK for st, _ in seen[0][0])


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_three_hundred_entries_at_all_sixteen_residues(ctx, device):
    arc, plain = Z.residues()
    with lzma_amd.ZipFile(arc) as z:
        assert {(e["data_off"] + 9) % 16 for e in z.entries if e["method"] == 14} == set(range(16))
        assert {e["data_off"] % 16 for e in z.entries if e["method"] == 0} == set(range(16))
        assert plain == _judge(arc)
        wants, cap = _windows(z, range(len(z.entries)), gap=3)
        res, got = _run(ctx, z, wants, cap, device)
        _check_good(z, wants, res, got, plain)
        assert _untouched(got, wants, res)
        assert {w[1] % 16 for w in wants} == set(range(16))  # ... and so do the windows


def _expected(kind, st, verify=True):
    own = (N.ERR_RESULT, N.ERR_PROPS, N.ERR_HEADER_EOF, N.ERR_RC_INIT, N.ERR_UNEXPECTED_EOF)  # a stream's own, or the CRC's
    return {"stream_or_crc": st in own, "crc": st == (N.ERR_RESULT if verify else N.OK), "result": st == N.ERR_RESULT,
            "unsupported": st == N.ERR_UNSUPPORTED, "bad": st == N.ERR_RESULT}[kind]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_damaged_entries_fail_alone(ctx, device):
    arc, what, plain = Z.damaged()
    kind_of = {i: (name, kind) for name, (i, kind) in what.items()}
    with lzma_amd.ZipFile(arc) as z:
        wants, cap = _windows(z, range(len(z.entries)), extra=2)
        res, got = _run(ctx, z, wants, cap, device)
        stats = ctx.last_zip_extract_stats()
        for (i, off, wcap), (st, n) in zip(wants, res):
            if i in kind_of:
                assert _expected(kind_of[i][1], st) and n == 0, (kind_of[i], st, n)
            else:  # the neighbours
                assert (st, n) == (N.OK, len(plain[i])) and got[off:off + n] == plain[i], z.names[i]
        # (the host form writes nothing into a failed entry's window; the device form may have where only the CRC32 could tell)
        assert _untouched(got, wants, res, {k for k, w in enumerate(wants) if device and kind_of.get(w[0], ("", ""))[1] in ("crc", "stream_or_crc")})
        assert stats["failed_entries"] == len(what) and stats["entries"] == len(z.entries)
        # alone equals many, entry by entry
        for (i, off, wcap), r in zip(wants, res):
            alone, got1 = _run(ctx, z, [(i, GUARD, wcap)], wcap + 2 * GUARD, device)
            assert alone == [r], (z.names[i], alone, r)
            assert got1[GUARD:GUARD + r[1]] == got[off:off + r[1]]
        # without verify only the CRC's own failures go away
        res2, _ = _run(ctx, z, wants, cap, device, verify=False)
        for (i, _, _), (st, n), r in zip(wants, res2, res):
            if i in kind_of and kind_of[i][1] == "crc":
                assert st == N.OK and n == z.entries[i]["size"]
            elif i not in kind_of or kind_of[i][1] != "stream_or_crc":
                assert (st, n) == r


def test_a_short_window_is_out_cap_and_changes_nothing_else(ctx):
    arc = Z.mixed()
    plain = _judge(arc)
    with lzma_amd.ZipFile(arc) as z:
        idx = [z.index("dir/lzma_16385.txt"), z.index("s257.bin"), z.index("dir/lzma_17.txt"), z.index("s16.bin")]
        wants, cap = _windows(z, idx)
        full, _ = _run(ctx, z, wants, cap, True)
        for k in (0, 1):
            short = list(wants)
            short[k] = (wants[k][0], wants[k][1], wants[k][2] - 1)
            res, got = _run(ctx, z, short, cap, True)
            assert res[k] == (N.ERR_OUT_CAP, 0) and [r for j, r in enumerate(res) if j != k] == [r for j, r in enumerate(full) if j != k]
            assert got[short[k][1]:short[k][1] + short[k][2]] == bytes([FILL]) * short[k][2]
            stats = ctx.last_zip_extract_stats()
            assert stats["lzma_entries"] + stats["stored_entries"] == 3  # (it asked nothing of the batch)
            for j, (i, off, c) in enumerate(short):
                if j != k:
                    assert got[off:off + c] == plain[i]


def test_two_thousand_stored_entries_go_up_in_one_transfer(ctx):
    arc, plain = Z.many_stored(2000, 1, 300)
    with lzma_amd.ZipFile(arc) as z:
        tensor, table = z.extract_tensor(ctx, range(2000))
        stats, chk = ctx.last_zip_extract_stats(), ctx.last_check_stats()
        got = tensor.cpu().numpy().tobytes()
        for (i, off, n, st), p in zip(table, plain):
            assert (st, n) == (N.OK, len(p)) and got[off:off + n] == p, i
        assert stats["stored_uploads"] == 1 and stats["stored_entries"] == 2000 and stats["lzma_entries"] == 0
        assert chk["device_ranges"] == 2000 and chk["host_ranges"] == 0
        # a wrong CRC among them is seen where the bytes lie
        bad = bytearray(arc)
        bad[z.entries[1234]["data_off"]] ^= 1
    with lzma_amd.ZipFile(bytes(bad)) as z:
        res = z.extract(ctx, range(2000))
        assert [k for k, (st, _) in enumerate(res) if st != N.OK] == [1234] and res[1234] == (N.ERR_RESULT, b"")
        assert ctx.last_zip_extract_stats()["stored_uploads"] == 1


def test_extract_tensor_gives_the_same_bytes_as_extract(ctx):
    arc = Z.mixed()
    with lzma_amd.ZipFile(arc) as z:
        idx = [i for i, e in enumerate(z.entries) if e["method"] != 8]
        host = z.extract(ctx, idx)
        for align in (1, 256):
            tensor, table = z.extract_tensor(ctx, idx, align=align)
            got = tensor.cpu().numpy().tobytes()
            assert [(st, got[off:off + n]) for _, off, n, st in table] == host
            assert all(off % align == 0 for _, off, _, _ in table)
        with pytest.raises(lzma_amd.LzmaError) as ei:
            z.read(ctx, "deflated.txt")
        assert ei.value.status == N.ERR_UNSUPPORTED
        assert z.read(ctx, "dir/") == b""


@pytest.mark.parametrize("which", ["prepended_1000", "prepended_1000_zip64", "descriptors", "forced_zip64", "zip64_ones", "comment_65535"])
def test_archives_extract_as_zipfile_reads_them(ctx, which):
    arc = Z.descriptors() if which == "descriptors" else Z.forced_zip64() if which == "forced_zip64" else Z.end_variants()[which]
    plain = _judge(arc)
    with lzma_amd.ZipFile(arc) as z:
        assert z.extract(ctx, range(len(z.entries))) == [(N.OK, p) for p in plain]
        tensor, table = z.extract_tensor(ctx, range(len(z.entries)))
        got = tensor.cpu().numpy().tobytes()
        assert [got[off:off + n] for _, off, n, _ in table] == plain


def test_the_info_zip_archive(ctx):
    sys.path.insert(0, Z.GOLDEN)
    import make_infozip_zip as R
    with lzma_amd.ZipFile(Z.infozip()) as z:
        res = dict(zip(z.names, z.extract(ctx, range(len(z.entries)))))
        for name, data in R.STORED.items():
            assert res[name] == (N.OK, data), name
        for name in R.DEFLATED:
            assert res[name] == (N.ERR_UNSUPPORTED, b""), name
        assert res["sub/"] == (N.OK, b"")
