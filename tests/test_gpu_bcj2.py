"""GPU: BCJ2 folders merged on the device (lzma_amd/csrc/xlz_bcj2_dev.hip) -- Batch.bcj2 on a device-resident batch against
tests/bcj2_ref.py, and sevenzip_decode / sevenzip_decode_device in bcj2 mode 1 (the kernel) and 2 (host threads).
Everything is bit-exact.  Damaged inputs are data errors the merge must report: every read is bounds-checked, nothing here
reads or writes out of range."""
import lzma
import random

import numpy as np
import pytest

import bcj2_ref as B
import filter_ref as R
import lzma_amd
import sevenzip_bcj2 as Z
import sevenzip_chains
import sevenzip_craft
from lzma_amd import FMT_LZMA2_RAW, LzmaError

pytestmark = pytest.mark.gpu

DICT = 1 << 16
FILL = 0xA5
LENS = (0, 1, 4, 5, 15, 16, 17, 1023, 1024, 1025, 65_539)
MODS = (0, 1, 7, 13)


def _filled(n):
    import torch
    t = torch.full((max(n, 1),), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _soup(n, seed, density=4):
    """random bytes with E8 / E9 / 0F 8x sprinkled in, operands with top byte 00 / FF / 0F / anything"""
    rnd = random.Random(seed)
    v = bytearray(rnd.randbytes(n))
    i = 0
    while i + 6 < n:
        if rnd.randrange(100) < density:
            r = rnd.randrange(4)
            if r == 3:
                v[i], v[i + 1] = 0x0F, 0x80 | rnd.randrange(16)
                i += 1
            else:
                v[i] = 0xE9 if r == 0 else 0xE8
            v[i + 4] = rnd.choice((0x00, 0xFF, 0x0F, rnd.randrange(256)))
        i += 1
    return bytes(v)


def _plain(n):
    return bytes((7 * k + 1) % 0xE0 for k in range(n))  # no candidate in it


def _cases():
    """-> [(data, convert, out_len)]: what the issue lists, then random ones up to about 300"""
    out = []
    for k, n in enumerate(LENS):
        for d in (0, 5, 40):
            out.append((_soup(n, 100 * k + d, d), None, n))
        out.append((_soup(n, 77 + k, 20), B.convert_0f_too, n))
    out.append((_plain(1023) + b"\xE8\x10\x00\x00\x00" + _plain(300), None, None))  # opcode ends a window, operand in the next
    out.append((_plain(1024 + 1023) + b"\xE9\x10\x00\x00\xFF" + _plain(30), None, None))
    for lead in (5, 15, 1023, 1024, 2047):  # the prev trap: inside a lane, across lanes, across windows
        out.append((B.trap_data(lead)[0], B.convert_0f_too, None))
    out.append((_soup(1024, 1, 30) + _plain(1024) + _soup(700, 2, 30), None, None))  # a window without candidates
    out.append((b"\xE8\x00\x00\x00\x00" * 1100, None, None))  # a window of 1024 candidates, all taken
    out.append((b"\xE8" * 2100, None, None))                  # ... none taken (the operand's top byte is E8)
    out.append((b"".join(bytes([0x0F, 0x80 | (k & 15)]) for k in range(1100)), None, None))
    end = _plain(2000) + b"\xE8\x10\x00\x00\x00"  # a conversion that ends exactly at out_len, and less room than that
    for cut in range(0, 7):
        out.append((end, None, len(end) - cut))
    rnd = random.Random(2024)
    while len(out) < 300:
        n = rnd.choice((rnd.randrange(1, 200), rnd.randrange(900, 1200), rnd.randrange(1, 6000)))
        out.append((_soup(n, rnd.randrange(1 << 30), rnd.randrange(50)), rnd.choice((None, None, B.convert_0f_too)), None))
    return out


def _lzma2(data):
    return lzma.compress(data, format=lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA2, "dict_size": DICT, "preset": 0}])


class Plan:
    """items for Batch.bcj2 over a list of (streams, out_len): every third item reads main / call / jump from the batch
    (streams decoded by the same batch), the next one only its main stream, the next one nothing; destinations at MODS
    modulo 16 with guard bytes between them"""

    def __init__(self, specs, broken=()):
        self.streams, self.items, self.ranges = [], [], []
        at = 0
        for q, (st4, out_len) in enumerate(specs):
            src = []
            for j in range(3):
                from_batch = st4[j] and (q % 3 == 0 or (q % 3 == 1 and j == 0))
                if from_batch:
                    comp = _lzma2(st4[j])
                    if (q, j) in broken:  # a stream that does not decode: its last bytes are missing
                        comp = comp[: len(comp) // 2]
                    src.append(len(self.streams))
                    self.streams.append(lzma_amd.Stream(comp, FMT_LZMA2_RAW, out_cap=len(st4[j]), dict_size=DICT))
                else:
                    src.append(st4[j])
            at += 19
            at += (MODS[q % 4] - at) % 16
            self.items.append((src[0], src[1], src[2], st4[3], out_len, at))
            self.ranges.append((at, out_len))
            at += out_len
        self.cap = at + 64
        if not self.streams:
            self.streams.append(lzma_amd.Stream(_lzma2(b"x"), FMT_LZMA2_RAW, out_cap=1, dict_size=DICT))


@pytest.fixture(scope="module")
def cases300():
    """-> [(the four streams, out_len, expected bytes)], judged by tests/bcj2_ref.py"""
    out = []
    for data, convert, out_len in _cases():
        st4 = B.encode(data, convert)
        n = len(data) if out_len is None else out_len
        st, ref = B.decode(*st4, n)
        assert st == B.OK and ref == data[:n]
        out.append((st4, n, ref))
    return out


def test_merge_of_300_items_in_one_launch(ctx, cases300):
    plan = Plan([(s, n) for s, n, _ in cases300])
    assert any(isinstance(it[1], int) for it in plan.items) and any(not isinstance(it[0], int) for it in plan.items)
    assert {at % 16 for at, _ in plan.ranges} == set(MODS)
    b = lzma_amd.Batch(ctx, plan.streams)
    b.run()
    dst = _filled(plan.cap)
    res = b.bcj2(plan.items, dst.data_ptr(), plan.cap)
    want = np.full(plan.cap, FILL, dtype=np.uint8)
    for (at, n), (_, _, ref) in zip(plan.ranges, cases300):
        want[at:at + n] = np.frombuffer(ref, dtype=np.uint8)
    assert res == [(lzma_amd.OK, n) for _, n, _ in cases300]
    assert _bytes(dst) == want.tobytes()  # the merged bytes, and every guard byte between and around them
    st = ctx.last_bcj2_stats()
    assert st["device_items"] == len(cases300) and st["device_bytes"] == sum(n for _, n, _ in cases300)
    assert st["host_items"] == 0 and st["failed_items"] == 0 and st["launches"] == 1 and st["kernel_ms"] > 0
    b.close()


def _damaged_specs():
    code = R.machine_code(30_000)
    good = B.encode(code)
    main, call, jump, rc = good
    assert len(call) >= 8 and len(jump) >= 8
    specs = [(good, len(code)), ((main, call[:-1], jump, rc), len(code)), (good, len(code)), ((main, call, jump[:-4], rc), len(code)),
             ((main, call, jump, rc[:len(rc) // 2]), len(code)), (good, len(code) - 3), ((main[:-1], call, jump, rc), len(code)),
             ((main, call, jump, rc[:4]), len(code)), (good, len(code)), (good, len(code)), (good, len(code) + 1), (good, len(code))]
    bad = {1, 3, 4, 6, 7, 9, 10}  # (9: its main stream, a stream of the batch, does not decode)
    return code, specs, bad


@pytest.mark.parametrize("mode", [1, 2])
def test_damaged_items_among_good_ones(ctx, mode):
    code, specs, bad = _damaged_specs()
    for st4, n in specs[:9]:
        assert (B.decode(*st4, n)[0] != B.OK) == (specs.index((st4, n)) in bad)
    plan = Plan(specs, broken={(9, 0)})
    assert isinstance(plan.items[9][0], int)
    b = lzma_amd.Batch(ctx, plan.streams)
    b.run()
    assert b.results()[plan.items[9][0]][1] < 0
    dst = _filled(plan.cap)
    ctx.set_bcj2_mode(mode)
    try:
        res = b.bcj2(plan.items, dst.data_ptr(), plan.cap)
    finally:
        ctx.set_bcj2_mode(0)
    got = np.frombuffer(_bytes(dst), dtype=np.uint8)
    inside = np.zeros(plan.cap, dtype=bool)
    for q, ((at, n), (st4, _)) in enumerate(zip(plan.ranges, specs)):
        inside[at:at + n] = True
        if q in bad:
            assert res[q] == (lzma_amd.ERR_RESULT, 0), q
        else:
            assert res[q] == (lzma_amd.OK, n), q
            assert got[at:at + n].tobytes() == code[:n], q
    assert (got[~inside] == FILL).all()  # nothing outside the items' ranges, whatever a failed item left inside its own
    st = ctx.last_bcj2_stats()
    assert st["failed_items"] == len(bad)
    assert (st["device_items"], st["host_items"]) == ((len(specs) - 1, 0) if mode == 1 else (0, len(specs) - 1))  # (9 never ran)
    b.close()


def test_bad_arguments_write_nothing(ctx):
    code = R.machine_code(5000)
    st4 = B.encode(code)
    plan = Plan([(st4, len(code)), (st4, len(code))])
    b = lzma_amd.Batch(ctx, plan.streams)
    b.run()
    dst = _filled(plan.cap)
    a, c = plan.items
    for items, cap in (([a, c[:5] + (a[5] + 10,)], plan.cap),           # the destination ranges overlap
                       ([a, c], plan.cap - 65),                         # ... reach past dst_cap
                       ([a, (len(plan.streams),) + c[1:]], plan.cap)):  # a stream the batch does not have
        with pytest.raises(LzmaError) as e:
            b.bcj2(items, dst.data_ptr(), cap)
        assert e.value.status == lzma_amd.ERR_BAD_ARG
    host = np.zeros(plan.cap, dtype=np.uint8)
    with pytest.raises(LzmaError) as e:  # host memory is no destination
        b.bcj2([a], host.ctypes.data, plan.cap)
    assert e.value.status == lzma_amd.ERR_BAD_ARG
    assert _bytes(dst) == bytes([FILL]) * plan.cap
    for mode in (-1, 3):
        with pytest.raises(LzmaError) as e:
            ctx.set_bcj2_mode(mode)
        assert e.value.status == lzma_amd.ERR_BAD_ARG
    assert ctx.bcj2_mode() == 0
    b.close()


@pytest.fixture(scope="module")
def mixed_archive():
    """BCJ2 folders of both forms (LZMA and LZMA2, solid with per-file CRCs), a plain LZMA folder, an x86 chain folder and a
    Copy folder -> (folders, the files back to back)"""
    code, text = R.machine_code(400_000), R.text(30_000)
    c = [code[k * 90_000:(k + 1) * 90_000] for k in range(4)]
    rec, packed, nc = sevenzip_chains.chain_folder(code[:50_000], [{"id": lzma.FILTER_X86}], lzma_first=True)
    folders = [Z.bcj2_folder([c[0][:1001], c[0][1001:]], 4, False, "libarchive"),
               Z.plain_folder(*sevenzip_craft.lzma_folder(text), [text[:77], text[77:]]),
               Z.bcj2_folder([c[1]], 4, True, "7zip"),
               Z.plain_folder(rec, packed, [code[:50_000]], nc),
               Z.bcj2_folder([c[2][:5], c[2][5:70_000], c[2][70_000:]], 2, False),
               Z.plain_folder(*sevenzip_craft.copy_folder(text[:1234]), [text[:1234]]),
               Z.bcj2_folder([c[3]], 2, True)]
    return folders, b"".join(x for f in folders for x in f["files"])


@pytest.mark.parametrize("mode", [1, 2])
def test_front_ends_decode_bcj2_folders(ctx, mixed_archive, mode):
    folders, want = mixed_archive
    arch = Z.archive(folders)
    n_bcj2, bcj2_bytes = 4, sum(len(x) for f in folders if "streams" in f for x in f["files"])
    ctx.set_filter_mode(1)
    ctx.set_bcj2_mode(mode)
    try:
        assert lzma_amd.sevenzip_decode(ctx, arch, verify=True) == want  # (mode 1: THE test that fails without the feature)
        st = ctx.last_bcj2_stats()
        assert (st["device_items"], st["host_items"]) == ((n_bcj2, 0) if mode == 1 else (0, n_bcj2)) and st["failed_items"] == 0
        assert st["device_bytes"] + st["host_bytes"] == bcj2_bytes
        dst = _filled(len(want) + 40)
        assert lzma_amd.sevenzip_decode_device(ctx, arch, dst.data_ptr() + 7, len(want), verify=True) == len(want)
        got = _bytes(dst)
        assert got[7:7 + len(want)] == want and got[:7] == bytes([FILL]) * 7 and got[7 + len(want):] == bytes([FILL]) * 33
        assert bytes(lzma_amd.sevenzip_decode_tensor(ctx, arch).cpu().numpy().tobytes()) == want
        # the CRCs are looked at: a flipped one of a file inside a solid BCJ2 folder, and of a BCJ2 folder with one file
        for at in (1, 2):
            bad = Z.archive(folders, crc_override={1: 0x12345678}) if at == 1 else Z.archive(folders, folder_crc_override={2: 0x12345678})
            assert bad != arch and len(bad) == len(arch)
            for call in (lambda: lzma_amd.sevenzip_decode(ctx, bad), lambda: lzma_amd.sevenzip_decode_device(ctx, bad, dst.data_ptr(), len(want))):
                with pytest.raises(LzmaError) as e:
                    call()
                assert e.value.status == lzma_amd.ERR_RESULT
            assert lzma_amd.sevenzip_decode(ctx, bad, verify=False) == want
        # a folder whose streams do not merge to its size
        main, call_s, jump, rc = folders[6]["streams"]
        short = folders[:6] + [Z.bcj2_folder(folders[6]["files"], 2, True, streams=(main, call_s, jump[:-4], rc))]
        with pytest.raises(LzmaError) as e:
            lzma_amd.sevenzip_decode(ctx, Z.archive(short), verify=False)
        assert e.value.status == lzma_amd.ERR_RESULT
        assert ctx.last_bcj2_stats()["failed_items"] == 1
    finally:
        ctx.set_bcj2_mode(0)
        ctx.set_filter_mode(0)


def test_mode_0_refuses_bcj2_folders_as_ever(ctx, mixed_archive):
    folders, want = mixed_archive
    arch = Z.archive([folders[0], folders[1]])
    assert ctx.bcj2_mode() == 0
    dst = _filled(len(want))
    for call in (lambda: lzma_amd.sevenzip_decode(ctx, arch), lambda: lzma_amd.sevenzip_decode_device(ctx, arch, dst.data_ptr(), len(want))):
        with pytest.raises(LzmaError) as e:
            call()
        assert e.value.status == lzma_amd.ERR_UNSUPPORTED
    # an archive without a BCJ2 folder takes the path it always took, whatever the mode
    plain = Z.archive([folders[1], folders[5]])
    ctx.set_bcj2_mode(1)
    try:
        assert lzma_amd.sevenzip_decode(ctx, plain) == b"".join(folders[1]["files"] + folders[5]["files"])
        assert ctx.last_bcj2_stats()["device_items"] == 0
    finally:
        ctx.set_bcj2_mode(0)
