"""GPU: chosen files of a .7z archive as ONE batch (include/xlz.h: xlz_7z_extract / xlz_7z_extract_device; DESIGN.md
section 3.17).  One archive of a few hundred KiB holds every kind of folder: a solid LZMA folder whose files have sizes 1,
15, 17, 4097 (zeros, and the file behind them begins with zeros: a cut falls inside one long match) and 70 001, an LZMA2
folder of one unit, one of several units, a Copy folder, an x86 chain, a BCJ2 folder, an empty file and a directory.  What
an entry must come back as is computed by a model in this file from the CPU oracle's decode of the folder's (cut) payload
-- the precedence of include/xlz.h, status by status."""
import ctypes
import shutil
import subprocess
import zlib

import pytest

import lzma_amd
import oracle
import sevenzip_bcj2 as B
import sevenzip_chains
import sevenzip_craft as C
import sevenzip_files as F
from lzma_amd import _native as N

pytestmark = pytest.mark.gpu

FILL = 0xA5
OK, RESULT, OUT_CAP, UNSUPPORTED, BAD_ARG = N.OK, N.ERR_RESULT, N.ERR_OUT_CAP, N.ERR_UNSUPPORTED, N.ERR_BAD_ARG


def _noise(n, seed):
    out, x = bytearray(n), seed * 2654435761 % (1 << 32) or 1
    for i in range(n):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out[i] = (x >> 16) & 0xFF if i % 9 else 0x20
    return bytes(out)


SOLID = [b"a", _noise(15, 1), _noise(17, 2), bytes(4097), bytes(300) + _noise(70001 - 300, 3)]
ONE_UNIT = [_noise(5000, 4), b"text " * 801]
UNITS = [_noise(3001, 5), b"z" * 5003, _noise(2, 6) * 2500, bytes(range(256)) * 9]
COPIED = [b"stored as it is", _noise(33, 7)]
X86 = [bytes([0xE8, 1, 2, 3, 0, 0x90, 0x90, 0xE9, 9, 8, 7, 0]) * 700, _noise(1234, 8)]
BCJ2 = [bytes([0x55, 0xE8, 0x10, 0x20, 0x00, 0x00, 0xC3]) * 300]


def _build(crc_override=None, no_crc=()):
    """-> (archive bytes, entries [(name, bytes or None)]).  Folder k's files are named fK_i."""
    rec0, pk0 = C.lzma_folder(b"".join(SOLID))
    rec1, pk1 = C.lzma2_folder(b"".join(ONE_UNIT))
    rec2, pk2 = F.lzma2_units_folder(UNITS)
    rec3, pk3 = C.copy_folder(b"".join(COPIED))
    rec4, pk4, n4 = sevenzip_chains.chain_folder(b"".join(X86), [{"id": 4}])
    groups = [SOLID, ONE_UNIT, UNITS, COPIED, X86, BCJ2]
    folders = [B.plain_folder(rec0, pk0, SOLID), B.plain_folder(rec1, pk1, ONE_UNIT), B.plain_folder(rec2, pk2, UNITS),
               B.plain_folder(rec3, pk3, COPIED), B.plain_folder(rec4, pk4, X86, n_coders=n4), B.bcj2_folder(BCJ2, form=4)]
    entries, content = [F.entry("a dir", "dir")], [("a dir", None)]
    for k, g in enumerate(groups):
        for i, data in enumerate(g):
            entries.append(F.entry("f%d_%d" % (k, i), mtime=F.filetime(1_700_000_000 + i)))
            content.append((entries[-1]["name"], data))
        if k == 0:
            entries.append(F.entry("nothing in it", "empty")), content.append(("nothing in it", None))
    return F.archive(folders, entries, crc_override=crc_override, no_crc=no_crc), content


@pytest.fixture(scope="module")
def built():
    return _build()


@pytest.fixture()
def modes(ctx):
    """the context's filter and bcj2 mode, put back behind the test"""
    def set_modes(filter_mode, bcj2_mode=0):
        ctx.set_filter_mode(filter_mode), ctx.set_bcj2_mode(bcj2_mode)
    yield set_modes
    ctx.set_filter_mode(0), ctx.set_bcj2_mode(0)


def _folder_status(z, arc, item, filter_mode):
    """the model of a covering folder's stream: -> (status for every wanted entry of it, the folder's decoded bytes)"""
    k, decode_len, in_len = item
    f = z.folders[k]
    chain = f["method"] in (1, 2) and k == 4
    if f["method"] not in (1, 2, 3) or (chain and filter_mode != 1):
        return UNSUPPORTED, b""
    payload = arc[f["pack_off"]:f["pack_off"] + in_len]
    if f["method"] == 3:
        return (OK, bytes(payload)) if f["pack_len"] == f["unpack_len"] else (RESULT, b"")
    if f["method"] == 1:
        out, st, used = oracle.lzma1_raw(f["props"], f["dict_size"], f["unpack_len"], bytes(payload), decode_len)
    else:
        out, st, used = oracle.lzma2_raw(bytes(payload), f["dict_size"], decode_len)
    if decode_len == f["unpack_len"]:
        good, expected = st >= 0 and len(out) == decode_len, None
    elif in_len == f["pack_len"]:
        good, expected = st == OUT_CAP and len(out) == decode_len, OUT_CAP
    else:
        good, expected = st == N.ERR_UNEXPECTED_EOF and len(out) == decode_len and used == in_len, N.ERR_UNEXPECTED_EOF
    if not good:
        return (st if st < 0 and st != expected else RESULT), b""
    if chain:
        import lzma
        out = lzma.decompress(bytes(arc[f["pack_off"]:f["pack_off"] + f["pack_len"]]), format=lzma.FORMAT_RAW,
                              filters=[{"id": lzma.FILTER_X86}, {"id": lzma.FILTER_LZMA1, "dict_size": 1 << 16, "lc": 3, "lp": 0, "pb": 2}])
    return OK, out


def _model(z, arc, wants, filter_mode, verify=True):
    """[(status, bytes or None, unverified)] per want (entry, dst_off, dst_cap), and the cover of the wants that ask for
    their folder"""
    asking = [w[0] for w in wants if z.entries[w[0]].size and w[2] >= z.entries[w[0]].size]
    usable = [i for i in asking if z.folders[z.entries[i].folder]["method"] in (1, 2, 3) and (z.entries[i].folder != 4 or filter_mode == 1)]
    cover = z.cover(usable)
    folder = {it[0]: _folder_status(z, arc, it, filter_mode) for it in cover}
    out = []
    for i, _, cap in wants:
        e = z.entries[i]
        if not e.size:
            out.append((OK, b"", 0))
        elif cap < e.size:
            out.append((OUT_CAP, None, 0))
        elif e.folder not in folder:
            out.append((UNSUPPORTED, None, 0))
        else:
            st, data = folder[e.folder]
            got = data[e.folder_off:e.folder_off + e.size]
            if st != OK:
                out.append((st, None, 0))
            elif verify and e.crc is not None and zlib.crc32(got) != e.crc:
                out.append((RESULT, None, 0))
            else:
                out.append((OK, got, 1 if verify and e.crc is None else 0))
    return out, cover


def _device(n):
    import torch
    t = torch.full((max(n, 1),), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def _run(form, ctx, z, wants, cap, verify=True, align=1):
    """-> ([(status, out_len, unverified)], the destination's bytes afterwards); the destination is filled with FILL.  The
    tensor form goes through SevenZipFile.extract_tensor with the caller's tensor: it lays the windows out itself (which must
    be the layout the caller made, every window as long as its entry) and does not report `unverified` (None here)."""
    if form == "tensor":
        assert all(w[2] == z.entries[w[0]].size for w in wants)
        t = _device(cap)
        out, laid = z.extract_tensor(ctx, [w[0] for w in wants], verify=verify, align=align, out=t)
        assert out.data_ptr() == t.data_ptr() and out.shape == t.shape
        assert [(i, off) for i, off, _, _ in laid] == [(w[0], w[1]) for w in wants]
        return [(st, n, None) for _, _, n, st in laid], bytes(t.cpu().numpy().tobytes()[:cap])
    if form == "host":
        buf = bytearray([FILL]) * max(cap, 1)
        res = z.extract_into(ctx, wants, buf, verify=verify) if cap else z._extract("xlz_7z_extract", ctx, wants, None, 0, verify)
        return res, bytes(buf[:cap])
    t = _device(cap)
    res = z.extract_device(ctx, wants, t.data_ptr() if cap else 0, cap, verify=verify)
    return res, bytes(t.cpu().numpy().tobytes()[:cap])


def _check(form, ctx, z, arc, idx, filter_mode, verify=True, align=1, slack=0):
    """extract entries idx into windows laid out back to back (each `slack` bytes longer than its entry) and compare with
    the model, byte by byte, FILL everywhere else -> (results, cover)"""
    wants, at = [], 0
    for i in idx:
        at = (at + align - 1) // align * align
        wants.append((i, at, z.entries[i].size + slack))
        at += z.entries[i].size + slack
    want, cover = _model(z, arc, wants, filter_mode, verify)
    res, dest = _run(form, ctx, z, wants, at + 7, verify, align)
    image = bytearray([FILL]) * (at + 7)
    for (i, off, cap), (st, data, nu), got in zip(wants, want, res):
        assert got == (st, len(data) if st == OK else 0, nu if got[2] is not None else None), (form, i, z.names[i], got, st)
        if st == OK:
            image[off:off + len(data)] = data
        else:
            image[off:off + cap] = dest[off:off + cap]  # (inside a failed entry's window the contents are unspecified)
    assert dest == bytes(image), (form, idx)
    stats = ctx.last_7z_extract_stats()
    assert stats["entries"] == len(idx) and stats["failed_entries"] == sum(st != OK for st, _, _ in want)
    assert stats["empty_entries"] == sum(not z.entries[i].size for i in idx)
    assert stats["folders"] == len(cover) and stats["decoded_bytes"] == sum(c[1] for c in cover)
    assert stats["comp_bytes"] == sum(c[2] for c in cover) and stats["folder_bytes"] == sum(z.folders[c[0]]["unpack_len"] for c in cover)
    assert stats["copied_bytes"] == sum(len(d) for st, d, _ in want if st == OK)
    return res, cover


@pytest.mark.parametrize("form", ["host", "device", "tensor"])
@pytest.mark.parametrize("filter_mode", [0, 1])
def test_every_entry_alone_and_all_together(ctx, built, modes, form, filter_mode):
    """(a), (b), (e): the bytes that were packed; in filter mode 1 (with bcj2 mode 1, so that the whole archive decodes) also
    the slices of sevenzip_decode on the same context; decoded_bytes / folder_bytes are the cover's; a chain entry in filter
    mode 0 and a BCJ2 entry in any mode are XLZ_ERR_UNSUPPORTED, alone too"""
    arc, content = built
    modes(filter_mode, 1 if filter_mode else 0)
    with lzma_amd.SevenZipFile(arc) as z:
        assert z.names == [n for n, _ in content]
        whole = lzma_amd.sevenzip_decode(ctx, arc) if filter_mode else None
        everything = list(range(len(z.entries)))
        res, cover = _check(form, ctx, z, arc, everything, filter_mode)
        assert [c[0] for c in cover] == ([0, 1, 2, 3, 4] if filter_mode else [0, 1, 2, 3])
        assert all(c[1] == z.folders[c[0]]["unpack_len"] for c in cover)  # (every last file is wanted: nothing is cut)
        for i in everything:
            e, data = z.entries[i], content[i][1]
            (st, n, _), = _check(form, ctx, z, arc, [i], filter_mode)[0]
            unsupported = e.size and (e.folder == 5 or (e.folder == 4 and not filter_mode))
            assert st == (UNSUPPORTED if unsupported else OK) == res[i][0], z.names[i]
            if st == OK:  # (_check compared the bytes with the model's: here the model against what was packed)
                assert _model(z, arc, [(i, 0, e.size)], filter_mode)[0][0][1] == (data or b"")
                if whole is not None and e.size:
                    at = z.folders[e.folder]["unpack_off"] + e.folder_off
                    assert whole[at:at + e.size] == data
        # (b) a first file costs less than its folder, a last one all of it
        first, last = z.index("f0_0"), z.index("f0_4")
        _, cover = _check(form, ctx, z, arc, [first], filter_mode)
        assert cover == [(0, 1, z.folders[0]["pack_len"])] and ctx.last_7z_extract_stats()["decoded_bytes"] == 1 < z.folders[0]["unpack_len"]
        _, cover = _check(form, ctx, z, arc, [last], filter_mode)
        assert ctx.last_7z_extract_stats()["decoded_bytes"] == ctx.last_7z_extract_stats()["folder_bytes"] == z.folders[0]["unpack_len"]
        # cuts that are no multiple of 16, inside the run of zeros, at a unit boundary, in a one-unit LZMA2 folder; pack
        # sources at odd offsets, aligned windows
        _, cover = _check(form, ctx, z, arc, [z.index("f0_3"), z.index("f0_1"), z.index("f1_0"), z.index("f2_1"), z.index("f3_1")], filter_mode, align=16)
        assert [(c[0], c[1]) for c in cover] == [(0, 33 + 4097), (1, 5000), (2, 3001 + 5003), (3, len(b"".join(COPIED)))]
        assert cover[2][2] < z.folders[2]["pack_len"] and cover[1][2] == z.folders[1]["pack_len"]


def test_the_python_forms(ctx, built, modes):
    """read / extract / extract_tensor give the same bytes; only call-level failures are raised"""
    arc, content = built
    modes(1)
    with lzma_amd.SevenZipFile(arc) as z:
        assert z.read(ctx, "f2_2") == UNITS[2] and z.read(ctx, "a dir") == b"" and z.read(ctx, z.index("f4_0")) == X86[0]
        with pytest.raises(lzma_amd.LzmaError) as ei:
            z.read(ctx, "f5_0")
        assert ei.value.status == UNSUPPORTED
        names = ["f0_2", "f5_0", "nothing in it", "f3_0", "f1_1"]
        got = z.extract(ctx, names)
        assert [g.status if isinstance(g, lzma_amd.LzmaError) else g for g in got] == [SOLID[2], UNSUPPORTED, b"", COPIED[0], ONE_UNIT[1]]
        t, laid = z.extract_tensor(ctx, names, align=64)
        flat = t.cpu().numpy().tobytes()
        assert [(z.names[i], st) for i, _, _, st in laid] == list(zip(names, [OK, UNSUPPORTED, OK, OK, OK]))
        assert all(off % 64 == 0 for _, off, _, _ in laid)
        assert [flat[off:off + n] for _, off, n, st in laid if st == OK] == [SOLID[2], b"", COPIED[0], ONE_UNIT[1]]
        assert z.extract(ctx, []) == []
        # the caller's tensor: used as it is where it is large enough; refused where it is too small, of another type, not
        # contiguous or not on the context's device
        import torch
        need = z.layout(names, 64)[1]
        mine = _device(need + 10)
        t2, laid2 = z.extract_tensor(ctx, names, align=64, out=mine)
        assert t2.data_ptr() == mine.data_ptr() and laid2 == laid
        assert mine.cpu().numpy().tobytes()[need:] == bytes([FILL]) * 10 and mine.cpu().numpy().tobytes()[:need][laid[4][1]:] == ONE_UNIT[1]
        with pytest.raises(lzma_amd.LzmaError) as ei:
            z.extract_tensor(ctx, names, align=64, out=torch.empty(need - 1, dtype=torch.uint8, device="cuda"))
        assert ei.value.status == OUT_CAP
        for bad in (torch.empty(need, dtype=torch.int8, device="cuda"), torch.empty(2 * need, dtype=torch.uint8, device="cuda")[::2],
                    torch.empty((need, 1), dtype=torch.uint8, device="cuda"), torch.empty(need, dtype=torch.uint8)):
            with pytest.raises(ValueError):
                z.extract_tensor(ctx, names, align=64, out=bad)


def _damaged(arc, z, folder, back):
    """a payload byte of `folder` flipped, `back` bytes in front of its end"""
    bad = bytearray(arc)
    bad[z.folders[folder]["pack_off"] + z.folders[folder]["pack_len"] - back] ^= 0x55
    return bytes(bad)


@pytest.mark.parametrize("form", ["host", "device"])
def test_damage_stays_with_its_folder_or_its_file(ctx, built, modes, form):
    """(c): a flipped payload byte in one folder, a wrong CRC on one file of a solid folder, damage behind a cut: the statuses
    are the model's -- the precedence of include/xlz.h over the oracle's decode --, every other entry is good, and an entry
    that is good in a set is good alone, with the same bytes"""
    arc, content = built
    modes(1)
    with lzma_amd.SevenZipFile(arc) as z:
        everything = list(range(len(z.entries)))
        names = z.names
        cases = {"payload of the one-unit folder": _damaged(arc, z, 1, 40), "behind every cut of the solid folder": _damaged(arc, z, 0, 12),
                 "in the last unit": _damaged(arc, z, 2, 9)}
    cases["a wrong CRC"] = _build(crc_override={2: 0x12345678})[0]
    cases["files without a CRC"] = _build(no_crc=(1, 6))[0]
    for name, bad in cases.items():
        with lzma_amd.SevenZipFile(bad) as z:
            assert z.names == names
            res, _ = _check(form, ctx, z, bad, everything, 1)
            failed = [z.names[i] for i in everything if res[i][0] != OK]
            if name == "a wrong CRC":
                assert failed == ["f0_2", "f5_0"] and res[z.index("f0_2")][0] == RESULT, name
            elif name == "files without a CRC":
                assert failed == ["f5_0"] and [z.names[i] for i in everything if res[i][2]] == ["f0_1", "f1_1"], name
            else:
                k = {"payload of the one-unit folder": 1, "behind every cut of the solid folder": 0, "in the last unit": 2}[name]
                damaged = set(failed) - {"f5_0"}  # (the BCJ2 entry fails in every case)
                assert damaged and damaged <= {n for n in names if n.startswith("f%d_" % k)}, (name, failed)
            # good in the set => good alone, the same bytes (alone its folder is cut no later)
            for i in everything:
                if res[i][0] == OK and z.entries[i].size:
                    alone, _ = _check(form, ctx, z, bad, [i], 1)
                    assert alone[0] == res[i], (name, z.names[i])
            if name == "behind every cut of the solid folder":
                # damage behind a folder's cut is not seen: the first four files alone are good, the set says otherwise for
                # what lies behind the damage
                early, _ = _check(form, ctx, z, bad, [z.index("f0_%d" % i) for i in range(4)], 1)
                assert [r[0] for r in early] == [OK] * 4 and res[z.index("f0_4")][0] != OK
            if name == "in the last unit":
                early, cover = _check(form, ctx, z, bad, [z.index("f2_0"), z.index("f2_2")], 1)
                assert [r[0] for r in early] == [OK, OK] and cover[0][1] < z.folders[2]["unpack_len"] and res[z.index("f2_3")][0] != OK


@pytest.mark.parametrize("form", ["host", "device"])
def test_windows(ctx, built, modes, form):
    """(d): a short window is that entry's XLZ_ERR_OUT_CAP and asks nothing of its folder; nothing is written outside the
    windows or behind out_len; the same entry twice"""
    arc, content = built
    modes(0)
    with lzma_amd.SevenZipFile(arc) as z:
        big, small, mid = z.index("f0_4"), z.index("f0_1"), z.index("f2_1")
        _check(form, ctx, z, arc, [small, mid, small, z.index("f3_0"), z.index("f3_0")], 0, slack=5)
        wants = [(big, 0, 70000), (small, 70000, 15), (mid, 70100, 5002), (z.index("a dir"), 1 << 62, 1 << 62)]
        want, cover = _model(z, arc, wants, 0)
        assert [w[0] for w in want] == [OUT_CAP, OK, OUT_CAP, OK] and cover == [(0, 16, z.folders[0]["pack_len"])]
        res, dest = _run(form, ctx, z, wants, 80000)
        assert [r[0] for r in res] == [OUT_CAP, OK, OUT_CAP, OK]
        assert dest == bytes([FILL]) * 70000 + SOLID[1] + bytes([FILL]) * (80000 - 70015)
        stats = ctx.last_7z_extract_stats()
        assert (stats["folders"], stats["decoded_bytes"], stats["failed_entries"], stats["copied_bytes"]) == (1, 16, 2, 15)
        # nothing but entries without bytes: no destination is needed
        assert _run(form, ctx, z, [(z.index("a dir"), 5, 0), (z.index("nothing in it"), 9, 9)], 0)[0] == [(OK, 0, 0), (OK, 0, 0)]
        assert ctx.last_7z_extract_stats()["folders"] == 0 and ctx.last_pack_stats()["launches"] == 0


def test_a_refused_call_leaves_the_statistics_alone(ctx, built, modes):
    """(g): XLZ_ERR_BAD_ARG -- overlapping windows, a window outside the destination, an entry outside the table, a host
    pointer as the device destination -- launches nothing, writes nothing and leaves every statistic as it was"""
    arc, _ = built
    modes(1)
    with lzma_amd.SevenZipFile(arc) as z:
        a, b = z.index("f0_1"), z.index("f4_1")
        _check("device", ctx, z, arc, [a, b], 1)
        before = (ctx.last_7z_extract_stats(), ctx.last_pack_stats(), ctx.last_check_stats(), ctx.last_filter_stats())
        assert before[1]["launches"] == 1 and before[3]["launches"] >= 1
        t = _device(4096)
        host = ctypes.create_string_buffer(bytes([FILL]) * 4096, 4096)
        refused = [("xlz_7z_extract_device", [(a, 0, 15), (b, 14, 1234)], t.data_ptr()), ("xlz_7z_extract_device", [(a, 4090, 15)], t.data_ptr()),
                   ("xlz_7z_extract_device", [(len(z.entries), 0, 15)], t.data_ptr()), ("xlz_7z_extract_device", [(a, 0, 15)], ctypes.addressof(host)),
                   ("xlz_7z_extract", [(a, 0, 15), (a, 7, 15)], ctypes.addressof(host))]
        for name, wants, dst in refused:
            with pytest.raises(lzma_amd.LzmaError) as ei:
                z._extract(name, ctx, wants, ctypes.c_void_p(dst), 4096, True)
            assert ei.value.status == BAD_ARG, (name, wants)
            assert (ctx.last_7z_extract_stats(), ctx.last_pack_stats(), ctx.last_check_stats(), ctx.last_filter_stats()) == before
        assert t.cpu().numpy().tobytes() == bytes([FILL]) * 4096 and host.raw == bytes([FILL]) * 4096


def test_an_archive_written_by_libarchive(ctx, tmp_path):
    """(f): names, bytes, and the encoded header opened on the device"""
    if not shutil.which("cmake"):
        pytest.skip("no cmake on this box: nothing here writes a .7z archive")
    files = [("first.txt", b"the first file\n" * 300), ("second.bin", _noise(40000, 9)), ("empty", b""), ("third", b"3")]
    d = tmp_path / "in"
    d.mkdir()
    for n, b in files:
        (d / n).write_bytes(b)
    out = tmp_path / "written.7z"
    subprocess.check_call(["cmake", "-E", "tar", "cf", str(out), "--format=7zip"] + [n for n, _ in files], cwd=str(d))
    arc = out.read_bytes()
    with pytest.raises(lzma_amd.LzmaError) as ei:  # (the header is encoded: without a context it cannot be read)
        lzma_amd.SevenZipFile(arc)
    assert ei.value.status == N.ERR_DEVICE
    with lzma_amd.SevenZipFile(arc, ctx) as z:
        listing = subprocess.run(["cmake", "-E", "tar", "tf", str(out)], capture_output=True, text=True, check=True).stdout.splitlines()
        assert z.names == listing and sorted(z.names) == sorted(n for n, _ in files)
        want = dict(files)
        got = z.extract(ctx, list(range(len(z.entries))))
        assert {n: g for n, g in zip(z.names, got)} == want
        assert z.read(ctx, "third") == b"3" and z.cover("first.txt")[0][1] < z.folders[0]["unpack_len"]



def test_a_crafted_archive_behind_an_encoded_header(ctx, built, modes):
    """the same table and bytes when the header -- FilesInfo with names, times and an empty file among it -- is LZMA-encoded
    and decoded on the device at open: the parser then reads FilesInfo out of the decoded header"""
    rec, pk = C.lzma_folder(b"".join(SOLID))
    rec2, pk2 = F.lzma2_units_folder(UNITS)
    folders = [B.plain_folder(rec, pk, SOLID), B.plain_folder(rec2, pk2, UNITS)]
    entries = [F.entry("d\u00e9j\u00e0/vu", "dir", attr=0x10), F.entry("s0", mtime=F.filetime(1_234_567_890)), F.entry("s1"), F.entry("gone", "anti"),
               F.entry("s2", attr=0x20), F.entry("s3"), F.entry("lone-\ud800", "empty"), F.entry("s4", mtime=F.filetime(7))] + \
              [F.entry("u%d" % i) for i in range(len(UNITS))]
    plain, enc = F.archive(folders, entries), F.archive(folders, entries, encoded_header=True)
    assert plain != enc
    with pytest.raises(lzma_amd.LzmaError) as ei:
        lzma_amd.SevenZipFile(enc)
    assert ei.value.status == N.ERR_DEVICE
    modes(0)
    with lzma_amd.SevenZipFile(plain) as a, lzma_amd.SevenZipFile(enc, ctx) as b:
        assert a.entries == b.entries and a.names == [F.as_utf8(e["name"]) for e in entries]
        assert [f["unpack_len"] for f in a.folders] == [f["unpack_len"] for f in b.folders]
        assert b.entries[1].mtime == 1_234_567_890 and b.entries[3].is_anti and b.entries[0].is_dir and not b.entries[6].is_dir
        for form in ("host", "device"):
            _check(form, ctx, b, enc, list(range(len(b.entries))), 0)
            _, cover = _check(form, ctx, b, enc, [b.index("s1"), b.index("u1")], 0)
            assert [(c[0], c[1]) for c in cover] == [(0, 16), (1, 3001 + 5003)]
        assert b.read(ctx, "s4") == SOLID[4] and b.read(ctx, "u3") == UNITS[3]
