"""GPU: the deflate (method 8) entries of a .zip archive through ZipFile in the context's deflate modes -- 0 refuses them
as ever, 1 inflates them on the device (lzma_amd/csrc/xlz_inflate_dev.hip), 2 on host threads -- in the same call as the
LZMA batch and the stored scatter.  The judges: Python's zipfile for the archive zipfile writes, the recipe of
tests/golden/infozip.zip for the one Info-ZIP wrote, Python's zlib for what a damaged payload is."""
import io
import os
import struct
import sys
import zipfile

import pytest
import torch   # (before libxlz.so is loaded: torch brings its own HIP runtime, which must be the one that initialises the device)

import inflate_edges as E
import lzma_amd
import zip_files as Z
from lzma_amd import _native as N

pytestmark = pytest.mark.gpu

OK, UNSUPPORTED, RESULT, EOF, OUT_CAP = N.OK, N.ERR_UNSUPPORTED, N.ERR_RESULT, N.ERR_UNEXPECTED_EOF, N.ERR_OUT_CAP


def _archive():
    """deflate at levels 0, 1 and 9, LZMA, stored, directories, a deflate entry of no bytes"""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w") as z:
        def put(name, data, method, level=None):
            z.writestr(zipfile.ZipInfo(name, (2024, 2, 29, 13, 37, 42)), data, compress_type=method, compresslevel=level)
        put("dir/", b"", zipfile.ZIP_STORED)
        put("d0.txt", Z.text(11, 5000), zipfile.ZIP_DEFLATED, 0)
        put("d1.txt", Z.text(12, 70000), zipfile.ZIP_DEFLATED, 1)
        put("lzma.txt", Z.text(13, 4000), zipfile.ZIP_LZMA)
        put("stored.bin", Z.noise(14, 1000), zipfile.ZIP_STORED)
        put("d9.txt", Z.text(15, 33000), zipfile.ZIP_DEFLATED, 9)
        put("dir/noise.bin", Z.noise(16, 3000), zipfile.ZIP_DEFLATED, 6)
        put("empty.txt", b"", zipfile.ZIP_DEFLATED, 6)
        put("dir/sub/", b"", zipfile.ZIP_STORED)
        put("d6.txt", Z.text(17, 257) * 40, zipfile.ZIP_DEFLATED, 6)
        put("lzma2.txt", Z.text(18, 9000), zipfile.ZIP_LZMA)
    return buf.getvalue()


@pytest.fixture(scope="module")
def archive():
    arc = _archive()
    with zipfile.ZipFile(io.BytesIO(arc)) as ref:
        plain = [ref.read(i) for i in ref.infolist()]
        methods = [i.compress_type for i in ref.infolist()]
    assert methods.count(zipfile.ZIP_DEFLATED) == 6 and plain[methods.index(8, 7)] == b""
    return arc, plain, methods


@pytest.fixture()
def modes(ctx):
    def set_mode(m):
        ctx.set_deflate_mode(m)
        assert ctx.deflate_mode() == m
    yield set_mode
    ctx.set_deflate_mode(0)


def _tensor_results(z, ctx, which, **kw):
    tensor, table = z.extract_tensor(ctx, which, **kw)
    got = tensor.cpu().numpy().tobytes()
    return [(st, got[off:off + n] if st == OK else b"") for _, off, n, st in table]


def test_the_mode_of_a_context(ctx):
    assert lzma_amd.Context(torch.cuda.current_device()).deflate_mode() == 0   # a new context refuses
    assert ctx.deflate_mode() == 0
    for m in (1, 2, 0):
        ctx.set_deflate_mode(m)
        assert ctx.deflate_mode() == m
    for m in (3, -1, 256):
        with pytest.raises(lzma_amd.LzmaError) as e:
            ctx.set_deflate_mode(m)
        assert e.value.status == N.ERR_BAD_ARG and ctx.deflate_mode() == 0


def test_mode_0_refuses_every_deflate_entry_as_ever(ctx, archive, modes):
    arc, plain, methods = archive
    modes(0)
    with lzma_amd.ZipFile(arc) as z:
        assert [e["deflate"] for e in z.entries] == [m == 8 for m in methods] and not any(e["supported"] for e in z.entries if e["deflate"])
        want = [(UNSUPPORTED, b"") if m == 8 and p else (OK, p) for m, p in zip(methods, plain)]
        assert z.extract(ctx, range(len(plain))) == want
        assert _tensor_results(z, ctx, range(len(plain))) == want
        s = ctx.last_zip_extract_stats()
        assert (s["entries"], s["failed_entries"], s["lzma_entries"], s["stored_entries"]) == (len(plain), 5, 2, 1)
        assert s["comp_bytes"] == sum(e["comp_size"] for e in z.entries if e["method"] != 8 and e["size"])


@pytest.mark.parametrize("mode", [1, 2])
def test_modes_1_and_2_give_what_zipfile_reads(ctx, archive, modes, mode):
    arc, plain, methods = archive
    modes(mode)
    with lzma_amd.ZipFile(arc) as z:
        everything = [(OK, p) for p in plain]
        for verify in (True, False):
            assert z.extract(ctx, range(len(plain)), verify=verify) == everything
            s, x = ctx.last_inflate_stats(), ctx.last_zip_extract_stats()
            inflated = sum(len(p) for m, p in zip(methods, plain) if m == 8)
            if mode == 1:
                assert s == {"device_items": 5, "device_bytes": inflated, "host_items": 0, "host_bytes": 0, "failed_items": 0, "uploads": 1,
                             "launches": 1}
            else:
                assert s == {"device_items": 0, "device_bytes": 0, "host_items": 5, "host_bytes": inflated, "failed_items": 0, "uploads": 0,
                             "launches": 0}
            assert (x["entries"], x["failed_entries"], x["lzma_entries"], x["stored_entries"], x["stored_uploads"]) == (len(plain), 0, 2, 1, 1)
            assert x["comp_bytes"] == sum(e["comp_size"] for e in z.entries if e["size"]) and x["copied_bytes"] == sum(map(len, plain))
            for align in (1, 256):
                assert _tensor_results(z, ctx, range(len(plain)), verify=verify, align=align) == everything
        # the INVARIANT: each entry alone gives what it gives among all; and the same entry twice, into two windows
        for i, p in enumerate(plain):
            assert z.extract(ctx, [i]) == [(OK, p)] == _tensor_results(z, ctx, [i])
        twice = [5, 1, 5, 3, 1]
        assert z.extract(ctx, twice) == [(OK, plain[i]) for i in twice] == _tensor_results(z, ctx, twice)
        assert z.read(ctx, "d9.txt") == plain[5] and z.read(ctx, "empty.txt") == b""


@pytest.mark.parametrize("mode", [1, 2])
def test_the_info_zip_archive(ctx, modes, mode):
    sys.path.insert(0, Z.GOLDEN)
    import make_infozip_zip as R
    modes(mode)
    with lzma_amd.ZipFile(Z.infozip()) as z:
        for res in (dict(zip(z.names, z.extract(ctx, range(len(z.entries))))), dict(zip(z.names, _tensor_results(z, ctx, range(len(z.entries)))))):
            for name, data in {**R.STORED, **R.DEFLATED}.items():
                assert res[name] == (OK, data), name
            assert res["sub/"] == (OK, b"")
        assert ctx.last_inflate_stats()["device_items" if mode == 1 else "host_items"] == 2


def _central(arc, name):
    """where the central record of `name` begins"""
    at = arc.rfind(b"PK\x05\x06")
    pos = struct.unpack_from("<I", arc, at + 16)[0]
    while arc[pos:pos + 4] == b"PK\x01\x02":
        n, m, k = struct.unpack_from("<HHH", arc, pos + 28)
        if arc[pos + 46:pos + 46 + n] == name.encode():
            return pos
        pos += 46 + n + m + k
    raise KeyError(name)


@pytest.mark.parametrize("mode", [1, 2])
def test_three_damaged_entries_fail_alone(ctx, archive, modes, mode):
    arc, plain, methods = archive
    bad = bytearray(arc)
    with lzma_amd.ZipFile(arc) as z:
        ent = {e["name"]: e for e in z.entries}
    flip = ent["d9.txt"]["data_off"] + ent["d9.txt"]["comp_size"] // 2
    bad[flip] ^= 0x10                                                               # one payload byte
    struct.pack_into("<I", bad, _central(arc, "d1.txt") + 16, ent["d1.txt"]["crc"] ^ 1)   # the CRC field of another
    cut = ent["d6.txt"]["comp_size"] - 3
    struct.pack_into("<I", bad, _central(arc, "d6.txt") + 20, cut)                  # a third payload, cut
    bad = bytes(bad)
    # what zlib makes of the two damaged payloads
    e9, e6 = ent["d9.txt"], ent["d6.txt"]
    cls9, out9, _ = E.judge(bad[e9["data_off"]:e9["data_off"] + e9["comp_size"]], e9["size"])
    want9 = {E.RESULT: RESULT, E.OUT_CAP: RESULT, E.EOF: EOF, E.OK: RESULT}[cls9]   # (OK: another size, or another CRC)
    assert cls9 != E.OK or out9 != plain[5]
    assert E.judge(bad[e6["data_off"]:e6["data_off"] + cut], e6["size"])[0] == E.EOF
    want = [(OK, p) for p in plain]
    names = [e["name"] for e in sorted(ent.values(), key=lambda e: e["header_off"])]
    want[names.index("d9.txt")] = (want9, b"")
    want[names.index("d1.txt")] = (RESULT, b"")
    want[names.index("d6.txt")] = (EOF, b"")
    modes(mode)
    with lzma_amd.ZipFile(bad) as z:
        assert z.names == names
        assert z.extract(ctx, range(len(plain))) == want
        assert ctx.last_zip_extract_stats()["failed_entries"] == 3
        assert _tensor_results(z, ctx, range(len(plain))) == want
        for i in range(len(plain)):
            assert z.extract(ctx, [i]) == [want[i]] == _tensor_results(z, ctx, [i])
        unverified = list(want)
        unverified[names.index("d1.txt")] = (OK, plain[names.index("d1.txt")])     # only its CRC field is wrong
        if cls9 == E.OK and len(out9) == e9["size"]:
            unverified[names.index("d9.txt")] = (OK, out9)
        assert z.extract(ctx, range(len(plain)), verify=False) == unverified


@pytest.mark.parametrize("mode", [1, 2])
def test_windows_too_small_are_out_cap(ctx, archive, modes, mode):
    arc, plain, methods = archive
    modes(mode)
    with lzma_amd.ZipFile(arc) as z:
        wants, total = z.layout(range(len(plain)), align=16)
        short = [(e, off, cap - 1 if methods[e] == 8 and cap and e % 2 else cap) for e, off, cap in wants]
        want = [(OUT_CAP, 0) if w[2] != s[2] else (OK, len(plain[w[0]])) for w, s in zip(wants, short)]
        assert sum(st == OUT_CAP for st, _ in want) == 3
        out = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert z.extract_device(ctx, short, out.data_ptr(), total) == want
        got = out.cpu().numpy().tobytes()
        host = bytearray(b"\xA5" * total)
        assert z.extract_into(ctx, short, host) == want
        for (e, off, cap), (st, n) in zip(wants, want):
            for image in (got, bytes(host)):
                assert image[off:off + cap] == (plain[e] if st == OK else b"\xA5" * cap), e
