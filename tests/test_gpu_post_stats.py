"""GPU: what the post-decode stage reports, call by call -- the characterisation of the host code between a decoded batch
and the caller (the check-kernel table, the digest sequence, the statistics' publishing, the device-destination form and
the .7z / .xz front-ends on top of them).  Every call is pinned by its status, its bytes against Python's own decode,
*unverified and all five last_*_stats of a fresh context; the call is then made again on the same context, which must
report the same (statistics are a call's, not a context's history).  The counters are computed here from what the
inputs hold, by the definitions in include/xlz.h; the `launches` are literals that describe the library as it was before
this file existed -- read off its launch counting (one per run of the check kernels' table, one per round of SHA-256 lanes,
two per round of x86 steps, one per pack, one per merge), since no GPU could be had to take them from a run: marked
"parent" below.  kernel_ms is only asked to be positive exactly where something was launched."""
import ctypes
import hashlib
import lzma
import struct
import zlib

import pytest

import bcj2_ref
import check_ref
import filter_ref as R
import lzma_amd
import sevenzip_bcj2 as Z
import sevenzip_chains
import sevenzip_craft as C
from lzma_amd import _native as N
from lzma_amd import CHECK_CRC32, CHECK_CRC64, CHECK_SHA256, FMT_LZMA2_RAW

pytestmark = pytest.mark.gpu

FILL = 0xA5
MIS = 5  # the device destinations start 5 bytes behind a multiple of 16
KINDS = ("check", "sha256", "filter", "pack", "bcj2")


# ---- the statistics ----
def _zero(struct_type):
    return {k: 0 for k, _ in struct_type._fields_ if k not in ("reserved", "kernel_ms")}


def _want(**given):
    """the five dicts (without kernel_ms), zero where nothing is given"""
    types = {"check": N.CheckStats, "sha256": N.Sha256Stats, "filter": N.FilterStats, "pack": N.PackStats, "bcj2": N.Bcj2Stats}
    out = {}
    for kind in KINDS:
        out[kind] = _zero(types[kind])
        extra = given.get(kind, {})
        assert set(extra) <= set(out[kind]), (kind, extra)
        out[kind].update(extra)
    return out


def _stats(ctx):
    return {"check": ctx.last_check_stats(), "sha256": ctx.last_sha256_stats(), "filter": ctx.last_filter_stats(),
            "pack": ctx.last_pack_stats(), "bcj2": ctx.last_bcj2_stats()}


def _assert_stats(ctx, want, what):
    got = _stats(ctx)
    print(what, got)
    for kind in KINDS:
        ms = got[kind].pop("kernel_ms")
        assert (ms > 0) == (got[kind]["launches"] > 0), (what, kind, ms, got[kind])
        assert got[kind] == want[kind], (what, kind)


def _pack_want(dst_offs, lens, mis):
    """the streams' regions of the arena begin at multiples of 256: an item is congruent when its destination is"""
    return {"items": len(lens), "bytes": sum(lens), "congruent_items": sum((o + mis) % 16 == 0 for o in dst_offs), "launches": 1}


# ---- the .7z archive ----
def _digests(values, defined):
    """a Digests record: not all defined -> a bit vector, MSB first, then the CRCs that are"""
    if all(defined):
        bits = b"\x01"
    else:
        v = bytearray((len(defined) + 7) // 8)
        for i, d in enumerate(defined):
            if d:
                v[i // 8] |= 0x80 >> (i % 8)
        bits = b"\x00" + bytes(v)
    return bytes([C.K_CRC]) + bits + b"".join(struct.pack("<I", c) for c, d in zip(values, defined) if d)


def _archive(folders, crc_of_folder=None):
    """folders: dicts as tests/sevenzip_bcj2.py makes them, each with "file_crc" (one flag per file) and "folder_crc";
    crc_of_folder: {folder index: the CRC32 to write instead of the right one}.  The FilesInfo lists one more file than the
    folders hold: an empty one (kEmptyStream)."""
    packed = b"".join(p for f in folders for p in f["packs"])
    si = bytes([C.K_PACK_INFO]) + C.number(0) + C.number(sum(len(f["packs"]) for f in folders)) + bytes([C.K_SIZE])
    si += b"".join(C.number(len(p)) for f in folders for p in f["packs"]) + bytes([C.K_END])
    si += bytes([C.K_UNPACK_INFO, C.K_FOLDER]) + C.number(len(folders)) + b"\x00" + b"".join(f["rec"] for f in folders)
    si += bytes([C.K_CODERS_UNPACK_SIZE]) + b"".join(C.number(v) for f in folders for v in f["sizes"])
    si += _digests([(crc_of_folder or {}).get(k, zlib.crc32(b"".join(f["files"]))) for k, f in enumerate(folders)],
                   [f["folder_crc"] for f in folders])
    si += bytes([C.K_END])
    si += bytes([C.K_SUBSTREAMS, C.K_NUM_UNPACK_STREAM]) + b"".join(C.number(len(f["files"])) for f in folders)
    sizes = b"".join(C.number(len(x)) for f in folders for x in f["files"][:-1])
    if sizes:
        si += bytes([C.K_SIZE]) + sizes
    need = [(zlib.crc32(x), d) for f in folders if not (len(f["files"]) == 1 and f["folder_crc"]) for x, d in zip(f["files"], f["file_crc"])]
    si += _digests([c for c, _ in need], [d for _, d in need])
    si += bytes([C.K_END]) + bytes([C.K_END])
    nfiles = sum(len(f["files"]) for f in folders) + 1
    empty = bytearray((nfiles + 7) // 8)
    empty[(nfiles - 1) // 8] |= 0x80 >> ((nfiles - 1) % 8)  # the last file has no stream
    header = bytes([C.K_HEADER, C.K_MAIN_STREAMS]) + si
    header += bytes([C.K_FILES]) + C.number(nfiles) + bytes([0x0E]) + C.number(len(empty)) + bytes(empty) + bytes([C.K_END]) + bytes([C.K_END])
    start = struct.pack("<QQI", len(packed), len(header), zlib.crc32(header))
    return b"7z\xbc\xaf\x27\x1c" + bytes([0, 4]) + struct.pack("<I", zlib.crc32(start)) + start + packed + header


def _folder(kind, folder, file_crc, folder_crc):
    return dict(folder, kind=kind, file_crc=file_crc, folder_crc=folder_crc)


class Archive:
    def __init__(self, folders):
        self.folders = folders
        self.data = _archive(folders)
        self.want = b"".join(x for f in folders for x in f["files"])
        self.offs, at = [], 0
        for f in folders:
            self.offs.append(at)
            at += sum(len(x) for x in f["files"])

    def lens(self, kinds):
        return [sum(len(x) for x in f["files"]) for f in self.folders if f["kind"] in kinds]

    def ranges(self, kinds):
        """the lengths of the CRC ranges of the folders of these kinds: every file that carries a CRC (the single file of a
        folder with a CRC carries the folder's), then the folder"""
        out = []
        for f in self.folders:
            if f["kind"] not in kinds:
                continue
            single = len(f["files"]) == 1 and f["folder_crc"]
            out += [len(x) for x, d in zip(f["files"], f["file_crc"]) if d or single]
            if f["folder_crc"]:
                out.append(sum(len(x) for x in f["files"]))
        return out

    def unverified(self):
        return sum(1 for f in self.folders if not f["folder_crc"] and not any(f["file_crc"]))


DECODED = ("lzma2", "chain", "lzma")  # the folders that are one stream of the batch each, packed into a device destination


@pytest.fixture(scope="module")
def archives():
    """-> (the archive of the issue, the same without its BCJ2 folder): a solid LZMA2 folder of three files of which two
    carry a CRC; a Copy folder with a CRC; an x86 BCJ + LZMA chain folder with a CRC; a BCJ2 folder of 3001 bytes (no multiple
    of 16) whose call and jump streams are stored, with a CRC; an LZMA folder that carries no CRC at all; one empty file"""
    text, code = R.text(3200 + 1234 + 600), R.machine_code(300_000 + 4000 + 3001)[300_000:]  # (calls and jumps to convert)
    solid = [text[:1000], text[1000:2500], text[2500:3200]]
    rec, packed, nc = sevenzip_chains.chain_folder(code[:4000], [{"id": lzma.FILTER_X86}])
    folders = [_folder("lzma2", Z.plain_folder(*C.lzma2_folder(b"".join(solid)), solid), [True, False, True], False),
               _folder("copy", Z.plain_folder(*C.copy_folder(text[3200:4434]), [text[3200:4434]]), [False], True),
               _folder("chain", Z.plain_folder(rec, packed, [code[:4000]], nc), [False], True),
               _folder("bcj2", Z.bcj2_folder([code[4000:]], 2, False), [False], True),
               _folder("lzma", Z.plain_folder(*C.lzma_folder(text[4434:]), [text[4434:]]), [False], False)]
    # Python's own decode of what the folders hold
    assert lzma.decompress(folders[0]["packs"][0], lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA2, "dict_size": 1 << 16}]) == b"".join(solid)
    assert lzma.decompress(packed, lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_X86}, {"id": lzma.FILTER_LZMA1, "dict_size": 1 << 16}]) == code[:4000]
    main, call, jump, rc = folders[3]["streams"]
    assert folders[3]["packs"][1:] == [call, jump, rc] and call and jump and bcj2_ref.decode(main, call, jump, rc, 3001) == (bcj2_ref.OK, code[4000:])
    return Archive(folders), Archive(folders[:3] + folders[4:])


def _sz(ctx, data, total, dptr=None):
    """xlz_7z_decode / xlz_7z_decode_device as the C ABI has them -> (status, out_len, *unverified, the host form's bytes)"""
    buf = ctypes.create_string_buffer(data, len(data))
    out_len, unverified = ctypes.c_uint64(77), ctypes.c_size_t(77)
    if dptr is not None:
        st = N.lib().xlz_7z_decode_device(ctx._h, ctypes.cast(buf, ctypes.c_void_p), len(data), ctypes.c_void_p(dptr), total,
                                          ctypes.byref(out_len), 1, ctypes.byref(unverified))
        return st, out_len.value, unverified.value, None
    out = ctypes.create_string_buffer(total + 1)
    st = N.lib().xlz_7z_decode(ctx._h, ctypes.cast(buf, ctypes.c_void_p), len(data), ctypes.cast(out, ctypes.c_void_p), total,
                               ctypes.byref(out_len), 1, ctypes.byref(unverified))
    return st, out_len.value, unverified.value, out.raw[:total]


def _filled(n):
    import torch
    t = torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def _twice(make_ctx, call, want, what):
    """call(ctx) on a fresh context, then again: the same statistics both times"""
    ctx = make_ctx()
    try:
        for k in range(2):
            call(ctx)
            _assert_stats(ctx, want, "%s, call %d" % (what, k))
    finally:
        ctx.close()


def _sz_want(a, check_mode, device, bcj2_mode):
    """what a successful front-end call on archive `a` in filter mode 1 leaves behind"""
    merged = bool(a.lens(("bcj2",)))  # a BCJ2 folder: the device-destination form, whatever the caller's destination is
    on_dev = device or merged or check_mode >= 1
    want = {"filter": {"device_steps": 1, "device_bytes": a.lens(("chain",))[0], "launches": 2}}  # (launches: parent)
    if on_dev:
        dev, host = a.ranges(DECODED + ("bcj2",)), a.ranges(("copy",))
        want["check"] = {"device_ranges": len(dev), "device_bytes": sum(dev), "host_ranges": len(host), "host_bytes": sum(host),
                         "launches": 2 if merged else 1}  # (launches: parent -- the arena's ranges, the destination's)
    if device or merged:
        offs = [o for o, f in zip(a.offs, a.folders) if f["kind"] in DECODED]
        want["pack"] = _pack_want(offs, a.lens(DECODED), MIS if device else 0)
    if merged:
        n = a.lens(("bcj2",))[0]
        want["bcj2"] = {"device_items": 1, "device_bytes": n, "launches": 1} if bcj2_mode == 1 else {"host_items": 1, "host_bytes": n}
    return _want(**want)


def _sz_call(a, data, device, status, unverified):
    total = len(a.want)

    def call(ctx):
        if device:
            dst = _filled(total + 40)
            st, n, nu, _ = _sz(ctx, data, total, dst.data_ptr() + MIS)
            got = dst.cpu().numpy().tobytes()
            assert got[:MIS] == bytes([FILL]) * MIS and got[MIS + total:] == bytes([FILL]) * (40 - MIS)
            got = got[MIS:MIS + total]
        else:
            st, n, nu, got = _sz(ctx, data, total)
        assert st == status
        if status == lzma_amd.OK:
            assert (n, nu) == (total, unverified) and got == a.want
        else:
            assert nu == 0 and (n == 0 or not device)
    return call


def _modes(check_mode, filter_mode, bcj2_mode):
    def make():
        ctx = lzma_amd.Context(0)
        ctx.set_check_mode(check_mode), ctx.set_filter_mode(filter_mode), ctx.set_bcj2_mode(bcj2_mode)
        return ctx
    return make


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("check_mode", [0, 1])
@pytest.mark.parametrize("bcj2_mode", [0, 1, 2])
def test_sevenzip_calls(archives, device, check_mode, bcj2_mode):
    full, plain = archives
    what = "7z %s, check mode %d, bcj2 mode %d" % ("device" if device else "host", check_mode, bcj2_mode)
    if bcj2_mode == 0:  # the BCJ2 folder is refused, before anything ran; the archive without it decodes as ever
        _twice(_modes(check_mode, 1, 0), _sz_call(full, full.data, device, lzma_amd.ERR_UNSUPPORTED, 0), _want(), what + ", refused")
        a = plain
    else:
        a = full
    _twice(_modes(check_mode, 1, bcj2_mode), _sz_call(a, a.data, device, lzma_amd.OK, a.unverified()), _sz_want(a, check_mode, device, bcj2_mode), what)


@pytest.mark.parametrize("device", [False, True])
def test_sevenzip_chain_refused_in_filter_mode_0(archives, device):
    _, plain = archives
    _twice(_modes(1, 0, 0), _sz_call(plain, plain.data, device, lzma_amd.ERR_UNSUPPORTED, 0), _want(), "7z filter mode 0")


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("bcj2_mode", [1, 2])
def test_sevenzip_flipped_crc_of_the_bcj2_folder(archives, device, bcj2_mode):
    full, _ = archives
    right = zlib.crc32(full.folders[3]["files"][0])
    bad = _archive(full.folders, crc_of_folder={3: right ^ 0x00010000})
    assert len(bad) == len(full.data) and 1 <= sum(x != y for x, y in zip(bad, full.data)) <= 1 + 4 + 4  # (and the two header CRCs)
    # everything ran, the comparison at the end failed: the statistics are the good archive's
    _twice(_modes(1, 1, bcj2_mode), _sz_call(full, bad, device, lzma_amd.ERR_RESULT, 0), _sz_want(full, 1, device, bcj2_mode),
           "7z flipped CRC, %s, bcj2 mode %d" % ("device" if device else "host", bcj2_mode))


# ---- the .xz file ----
@pytest.fixture(scope="module")
def xz_file():
    """four concatenated streams, checks none / CRC32 / CRC64 / SHA-256 -> (the file, the decoded bytes, the blocks' lengths)"""
    text = R.text(1500 + 3000 + 5000 + 8000)
    parts = [text[:1500], text[1500:4500], text[4500:9500], text[9500:]]
    data = b"".join(lzma.compress(p, format=lzma.FORMAT_XZ, check=c, preset=1)
                    for p, c in zip(parts, (lzma.CHECK_NONE, lzma.CHECK_CRC32, lzma.CHECK_CRC64, lzma.CHECK_SHA256)))
    assert lzma.decompress(data) == text
    return data, text, [len(p) for p in parts]


def _xz_digest_form_want(lens):
    """check mode 2 and the device form: CRC32 and CRC64 by the check kernels, the SHA-256 block where xlz_sha256_plan puts it"""
    on = int(lzma_amd.sha256_plan([lens[3]])[0])
    sha = {"device_ranges": on, "device_bytes": on * lens[3], "host_ranges": 1 - on, "host_bytes": (1 - on) * lens[3],
           "threshold": on * lens[3], "launches": on}
    check = {"device_ranges": 2 + on, "device_bytes": lens[1] + lens[2] + on * lens[3], "host_ranges": 1 - on,
             "host_bytes": (1 - on) * lens[3], "launches": 1 + on}  # (launches: parent; the SHA-256 launches count too)
    return check, sha


@pytest.mark.parametrize("check_mode", [0, 1, 2])
def test_xz_decode(xz_file, check_mode):
    data, text, lens = xz_file
    if check_mode == 0:
        want = _want()
    elif check_mode == 1:  # (the SHA-256 block stays with the host threads; launches: parent)
        want = _want(check={"device_ranges": 2, "device_bytes": lens[1] + lens[2], "host_ranges": 1, "host_bytes": lens[3], "launches": 1})
    else:
        check, sha = _xz_digest_form_want(lens)
        want = _want(check=check, sha256=sha)

    def call(ctx):
        out = ctypes.create_string_buffer(len(text) + 1)
        out_len, unverified = ctypes.c_uint64(77), ctypes.c_size_t(77)
        st = N.lib().xlz_xz_decode(ctx._h, ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p), len(data), ctypes.cast(out, ctypes.c_void_p),
                                   len(text), ctypes.byref(out_len), 1, ctypes.byref(unverified))
        assert (st, out_len.value, unverified.value) == (lzma_amd.OK, len(text), 0) and out.raw[:len(text)] == text
    _twice(_modes(check_mode, 0, 0), call, want, "xz check mode %d" % check_mode)


def test_xz_decode_device(xz_file):
    data, text, lens = xz_file
    check, sha = _xz_digest_form_want(lens)
    offs = [sum(lens[:k]) for k in range(4)]

    def call(ctx):
        dst = _filled(len(text) + 40)
        out_len, unverified = ctypes.c_uint64(77), ctypes.c_size_t(77)
        st = N.lib().xlz_xz_decode_device(ctx._h, ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p), len(data),
                                          ctypes.c_void_p(dst.data_ptr() + MIS), len(text), ctypes.byref(out_len), 1, ctypes.byref(unverified))
        assert (st, out_len.value, unverified.value) == (lzma_amd.OK, len(text), 0)
        got = dst.cpu().numpy().tobytes()
        assert got[MIS:MIS + len(text)] == text and got[:MIS] == bytes([FILL]) * MIS and got[MIS + len(text):] == bytes([FILL]) * (40 - MIS)
    _twice(_modes(0, 0, 0), call, _want(check=check, sha256=sha, pack=_pack_want(offs, lens, MIS)), "xz device")


# ---- Batch.digests ----
def test_batch_digests_mixed_kinds():
    """CRC32, CRC64 and SHA-256 ranges over two streams in one call: an empty range of each kind, ranges that begin behind a
    stream's end or reach past it, and enough short SHA-256 ranges that xlz_sha256_plan gives some to the device"""
    plain = [R.text(4000), R.machine_code(3001)]
    raw = [lzma.compress(p, format=lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA2, "dict_size": 1 << 16, "preset": 1}]) for p in plain]
    ranges = [(0, 0, 4000, CHECK_CRC32), (1, 0, 3001, CHECK_CRC64), (0, 7, 1000, CHECK_SHA256), (1, 0, 1 << 62, CHECK_SHA256),
              (0, 100, 0, CHECK_CRC32), (1, 100, 0, CHECK_CRC64), (0, 100, 0, CHECK_SHA256),           # empty as given
              (0, 4000, 5, CHECK_CRC32), (1, 5000, 5, CHECK_CRC64), (1, 3001, 5, CHECK_SHA256),        # behind the end
              (0, 3990, 100, CHECK_CRC32), (1, 2999, (1 << 64) - 1, CHECK_CRC64), (0, 3999, 9, CHECK_SHA256)]  # past the end
    ranges += [(k % 2, 3 * k, 64 + k % 5, CHECK_SHA256) for k in range(300)]
    clipped = [plain[s][off:off + n] for s, off, n, _ in ranges]
    sha_lens = [len(c) for c, r in zip(clipped, ranges) if r[3] == CHECK_SHA256 and c]
    on = lzma_amd.sha256_plan(sha_lens)
    assert any(on) and not all(on)
    dev_lens, host_lens = [n for n, d in zip(sha_lens, on) if d], [n for n, d in zip(sha_lens, on) if not d]
    sha_empty = sum(1 for c, r in zip(clipped, ranges) if r[3] == CHECK_SHA256 and not c)
    crc = [len(c) for c, r in zip(clipped, ranges) if r[3] != CHECK_SHA256]
    sha = {"device_ranges": len(dev_lens), "device_bytes": sum(dev_lens), "host_ranges": len(host_lens), "host_bytes": sum(host_lens),
           "empty_ranges": sha_empty, "threshold": max(dev_lens), "launches": 1}  # (launches: parent)
    check = {"device_ranges": sum(1 for n in crc if n) + len(dev_lens), "device_bytes": sum(crc) + sum(dev_lens), "host_ranges": len(host_lens),
             "host_bytes": sum(host_lens), "empty_ranges": sum(1 for n in crc if not n) + sha_empty, "launches": 2}  # (launches: parent)

    def call(ctx):
        b = lzma_amd.Batch(ctx, [lzma_amd.Stream(r, FMT_LZMA2_RAW, out_cap=len(p), dict_size=1 << 16) for r, p in zip(raw, plain)])
        try:
            b.run()
            got = b.digests(ranges)
            for q, (c, r) in enumerate(zip(clipped, ranges)):
                ref = {CHECK_CRC32: lambda: zlib.crc32(c) if c else 0, CHECK_CRC64: lambda: check_ref.crc64(c) if c else 0,
                       CHECK_SHA256: lambda: hashlib.sha256(c).digest()}[r[3]]()
                assert got[q] == ref, (q, r)
        finally:
            b.close()
    _twice(_modes(0, 0, 0), call, _want(check=check, sha256=sha), "Batch.digests")
