"""GPU: gzip files, BGZF files and zlib streams as one batch (lzma_amd/csrc/xlz_gz.hip) through lzma_amd.gz.  ONE call over
some 300 files -- the header, member, BGZF and defect cases of the CPU test, again with room to spare, a few of them with a window that is one
byte short or empty, 64 small .gz files, 64 zlib streams, one BGZF file of 203 blocks, one ordinary file of three members --
into a destination of 0xA5 with guard bytes between the windows.  Every status, every byte, out_len and in_consumed is
compared with gz.decode_host (the serial twin) and with the judges of tests/gz_files.py (Python's gzip and zlib).  Then:
every failing file alone; the statistics; deflate mode 2; the host form; a destination that is 5 modulo 16; the tensor
form.  Every stream is bounds-checked data: a damaged one is a status, nothing here reads or writes out of range."""
import pytest
import torch   # (before libxlz.so is loaded: torch brings its own HIP runtime, which must be the one that initialises the device)

import gz_files as G
import lzma_amd
from lzma_amd import gz

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xA5, 48


@pytest.fixture(scope="module")
def crowd():
    """-> [(case, cap, judged)]: judged = the case's cap is its own, so the judges apply; otherwise only the twin does"""
    named = G.header_cases() + G.member_cases() + G.bulk_cases()
    out = [(c, c.cap, True) for c in named]
    out += [(c, c.cap + 37, True) for c in G.header_cases() + G.member_cases()]   # (room to spare changes nothing)
    by = {c.name: c for c in named}
    for name in ("one_member", "three_members", "bgzf_5_blocks_eof", "zlib_one"):
        out += [(by[name], by[name].cap - 1, False), (by[name], 0, False)]
    return out


@pytest.fixture(scope="module")
def twin(crowd, xlz_so):
    """what gz.decode_host says of every file: computed once, never changed"""
    return [gz.decode_host(c.data, out_cap=cap) for c, cap, _ in crowd]


def _windows(crowd, shift=0):
    windows, at = [], GUARD + shift
    for k, (_, cap, _) in enumerate(crowd):
        at += (5 * k) % 16   # (every residue modulo 16)
        windows.append((at, cap))
        at += cap + GUARD
    return windows, at


def _compare(crowd, twin, windows, res, image, what, failed_untouched=False):
    covered = bytearray(len(image))
    for k, ((c, cap, judged), (off, _), r) in enumerate(zip(crowd, windows, res)):
        status, out_len, used, members = r
        out = bytes(image[off:off + out_len]) if status == G.OK else None
        assert (out, status, used, members) == twin[k], (what, c.name, cap, r, twin[k][1:])
        if judged:
            G.check(c, (out, status, used))
        else:
            assert status == G.ERR_OUT_CAP, (what, c.name, cap)
        if status != G.OK:
            assert out_len == 0 and used == 0
        if not (failed_untouched and status != G.OK):
            covered[off:off + cap] = b"\1" * cap
    outside = bytes(b for b, m in zip(image, covered) if not m)
    assert outside == bytes([FILL]) * len(outside), what   # the guards (and, in the host form, the failed files' windows)


def _device_call(ctx, crowd, shift=0, verify=True):
    windows, total = _windows(crowd)
    dst = torch.full((total + 16,), FILL, dtype=torch.uint8, device="cuda")
    res = gz.decode_many_device(ctx, [c.data for c, _, _ in crowd], dst.data_ptr() + shift, total, windows, verify=verify)
    return windows, res, dst.cpu().numpy().tobytes()[shift:shift + total]


def test_one_call_over_the_whole_crowd(ctx, crowd, twin):
    assert len(crowd) >= 290
    windows, res, image = _device_call(ctx, crowd)
    _compare(crowd, twin, windows, res, image, "device")
    s = gz.last_stats(ctx)
    zl = [k for k, (c, _, _) in enumerate(crowd) if G.is_zlib(c)]
    # a zlib stream reaches verification when its deflate stream ended well and four bytes follow it
    verified = sum(1 for k in zl if twin[k][1] == G.OK or crowd[k][0].name == "zlib_flipped_adler")
    bgzf = sum(1 for c, _, _ in crowd if c.name.startswith("bgzf_") and gz.probe(c.data)["bgzf"])
    assert s["files"] == len(crowd) and s["failed_files"] == sum(1 for t in twin if t[1] != G.OK)
    assert s["rounds"] == 3 and s["uploads"] == s["rounds"]
    assert s["adler_ranges"] == verified > 64
    assert s["bgzf_files"] == bgzf >= 10 and s["host_items"] == 0 and s["device_items"] >= s["members"] > 400
    assert s["members"] == sum(t[3] for t in twin)
    # every failing file alone: the same result
    for k, (c, cap, _) in enumerate(crowd):
        if twin[k][1] == G.OK:
            continue
        w, r, image = _device_call(ctx, [crowd[k]])
        _compare([crowd[k]], [twin[k]], w, r, image, "alone: " + c.name)


def test_the_bulk_alone_has_one_bgzf_file_and_verify_off_accepts_wrong_checks(ctx, crowd):
    bulk = [x for x in crowd if x[0].name.startswith(("small_gz_", "zlib_small_", "bgzf_203", "ordinary_three"))]
    assert len(bulk) == 130
    windows, res, image = _device_call(ctx, bulk)
    for (c, cap, _), (off, _), r in zip(bulk, windows, res):
        G.check(c, (bytes(image[off:off + r[1]]), r[0], r[2]))
    s = gz.last_stats(ctx)
    assert s["bgzf_files"] == 1 and s["rounds"] == 3 == s["uploads"] and s["adler_ranges"] == 64 and s["crc_ranges"] == 64 + 204 + 3
    assert s["failed_files"] == 0 and s["members"] == 64 + 64 + 204 + 3
    flipped = [x for x in crowd if x[0].check_only]
    assert len(flipped) >= 4
    windows, res, image = _device_call(ctx, flipped, verify=False)
    for (c, cap, _), (off, _), r in zip(flipped, windows, res):
        G.check(c, (bytes(image[off:off + r[1]]), r[0], r[2]), verify=False)
        assert r[0] == G.OK
    s = gz.last_stats(ctx)
    assert s["adler_ranges"] == 0 == s["crc_ranges"]


def test_deflate_mode_2_gives_identical_results(ctx, crowd, twin):
    ctx.set_deflate_mode(2)
    try:
        windows, res, image = _device_call(ctx, crowd)
    finally:
        ctx.set_deflate_mode(0)
    _compare(crowd, twin, windows, res, image, "host threads")
    s = gz.last_stats(ctx)
    assert s["device_items"] == 0 and s["uploads"] == 0 and s["host_items"] >= s["members"] > 400 and s["rounds"] == 3


def test_the_host_form_and_a_destination_that_is_5_modulo_16(ctx, crowd, twin):
    windows, total = _windows(crowd)
    out = bytearray([FILL]) * total
    res = gz.decode_many_into(ctx, [c.data for c, _, _ in crowd], out, windows)
    _compare(crowd, twin, windows, res, bytes(out), "host form", failed_untouched=True)
    w, res5, image5 = _device_call(ctx, crowd, shift=5)
    assert res5 == res
    _compare(crowd, twin, w, res5, image5, "5 modulo 16")
    # decode_many: the same files, windows from the size hints and the given caps
    some = [x for x in crowd if x[2]][::7]
    got = gz.decode_many(ctx, [c.data for c, _, _ in some], caps=[cap for _, cap, _ in some])
    for (c, _, _), g in zip(some, got):
        G.check(c, g)
    one = next(c for c, _, _ in crowd if c.name == "bgzf_203_blocks")
    assert gz.decompress(ctx, one.data) == G.judge_gzip(one.data)[1]
    cut = next(c for c, _, _ in crowd if c.name == "cut_second_member")
    with pytest.raises(lzma_amd.LzmaError) as e:
        gz.decompress(ctx, cut.data, out_cap=cut.cap)
    assert e.value.status == G.ERR_UNEXPECTED_EOF


def test_the_tensor_form_returns_views_of_the_judges_bytes(ctx, crowd):
    some = [x for x in crowd if x[2] and x[0].name.startswith(("small_gz_0", "zlib_small_0", "bgzf_", "three_members", "junk"))]
    tensor, views, res = gz.decode_many_tensor(ctx, [c.data for c, _, _ in some], caps=[cap for _, cap, _ in some], align=64)
    assert tensor.is_cuda and len(views) == len(some)
    for (c, _, _), v, r in zip(some, views, res):
        G.check(c, (None if v is None else v.cpu().numpy().tobytes(), r[0], r[2]))
        assert v is None or v.data_ptr() % 64 == tensor.data_ptr() % 64


def test_argument_rules(ctx, crowd):
    c = crowd[0][0]
    dst = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda")

    def bad(datas, ptr, cap, windows, **kw):
        with pytest.raises(lzma_amd.LzmaError) as e:
            gz.decode_many_device(ctx, datas, ptr, cap, windows, **kw)
        assert e.value.status == lzma_amd.ERR_BAD_ARG

    bad([c.data], dst.data_ptr(), 4096, [(4000, 700)])                          # a window that leaves the destination
    bad([c.data, c.data], dst.data_ptr(), 4096, [(0, 700), (699, 700)])         # two windows that share a byte
    bad([c.data], dst.data_ptr(), 4096, [(0, 700)], format=3)                   # an unknown format
    bad([c.data], 0, 4096, [(0, 700)])                                          # no destination
    host = bytearray(4096)
    import ctypes
    bad([c.data], ctypes.addressof((ctypes.c_char * 4096).from_buffer(host)), 4096, [(0, 700)])   # a host pointer
    assert dst.cpu().numpy().tobytes() == bytes([FILL]) * 4096                  # nothing was written
    assert gz.decode_many_device(ctx, [], dst.data_ptr(), 4096, []) == []
    # no room at all: the empty member is sound, the other wants more than its window
    assert gz.decode_many_device(ctx, [G.member(b""), c.data], dst.data_ptr(), 0, [(0, 0), (0, 0)]) == [(G.OK, 0, 20, 1), (G.ERR_OUT_CAP, 0, 0, 0)]
    assert gz.decode_many_device(ctx, [c.data], dst.data_ptr(), 4096, [(0, 700)])[0][:2] == (G.OK, 700)
