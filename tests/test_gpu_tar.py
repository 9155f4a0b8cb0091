"""GPU: the members of a .tar image in device memory (xlz_tar_scan_device, xlz_xz_tar_list).  The
classify kernel against the serial classifier, byte for byte; the device listing against the host walk (tar_parse) and
Python's tarfile on the archives of tests/tar_archives.py, the damaged and cut ones included; member views of a decoded
.tar.xz against tarfile's extractfile; TarXzFile on a 12-block .xz whose block edges are no multiples of 512."""
import ctypes
import io
import lzma
import os
import random
import sys
import tarfile
import time

import pytest
import torch   # (before libxlz.so is loaded: torch brings its own HIP runtime, which must be the one that initialises the device)

import lzma_amd
from lzma_amd import LzmaError
from lzma_amd import _native as N

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tar_archives as T  # noqa: E402
import xz_chains  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 512


def _upload(data, shift=0):
    """data at a 512-aligned device address + shift, with GUARD bytes of 0xA5 in front and behind -> (tensor, address)"""
    import torch
    host = bytes([0xA5]) * (GUARD + shift) + data + bytes([0xA5]) * GUARD
    t = torch.frombuffer(bytearray(host), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert t.data_ptr() % 512 == 0
    return t, t.data_ptr() + GUARD + shift


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _field_forms(rng):
    """a header block with each form of the checksum field, right and off by one, with and without high bytes"""
    out = []
    for high in (False, True):
        good = T.header((b"\xc8" * 30 if high else b"") + bytes(rng.randrange(97, 123) for _ in range(40)))
        body = good[:148] + b" " * 8 + good[156:]
        for total in (sum(body), sum(b - 256 if b >= 128 else b for b in body), sum(body) + 1, sum(body) - 1):
            for field in (b"%07o\0" % total, b"%06o\0 " % total, b"%6o \0" % total, b" %07o" % total, b" " * 8, bytes(8),
                          (b"%07o\0" % total).replace(b"0", b"8", 1), b"%06o\0x" % total, b"%08o" % total):
                out.append(good[:148] + field + good[156:])
    only_field = bytearray(512)
    only_field[148:156] = b"0000400\0"
    return out + [bytes(only_field)]


@pytest.fixture(scope="module")
def mixed_image():
    """8191 blocks and 511 bytes: the archives back to back, every field form, random blocks, zero runs -- shuffled by
    block, so that headers fall into both halves of a wave's pair -- and the serial classifier's flags for them"""
    rng = random.Random(512)
    blocks = []
    for image in list(T.everything().values()) + [v[0] for k, v in sorted(T.damaged().items()) if k != "meta_2mib"]:
        blocks += [image[i:i + 512] for i in range(0, len(image) - 511, 512)]
    blocks += _field_forms(rng)
    while len(blocks) < 8191:
        kind = rng.randrange(4)
        if kind == 0:
            blocks += [bytes(512)] * rng.randrange(1, 9)
        elif kind == 1:
            one = bytearray(512)
            one[rng.randrange(512)] = rng.randrange(1, 256)
            blocks.append(bytes(one))
        else:
            blocks.append(rng.randbytes(512))
    blocks = blocks[:8191]
    rng.shuffle(blocks)
    data = b"".join(blocks) + rng.randbytes(511)
    flags = bytes(T.serial_flag(b) for b in blocks)
    assert flags.count(1) > 100 and flags.count(2) > 300 and flags.count(0) > 300
    return data, flags


def _classify(ctx, ptr, n):
    flags = ctypes.create_string_buffer(bytes([0xEE]) * (n // 512 + 1), n // 512 + 1)
    ms = ctypes.c_double(-1)
    st = N.lib().xlz_internal_tar_classify_device(ctx._h, ctypes.c_void_p(ptr), n, flags, ctypes.byref(ms))
    return st, flags.raw, ms.value


@pytest.mark.parametrize("blocks", [1, 63, 64, 65, 8191])
@pytest.mark.parametrize("tail", [0, 1, 511])
def test_classify_kernel_equals_the_serial_classifier(ctx, mixed_image, blocks, tail):
    data, want = mixed_image
    # the last `blocks` blocks of the image and `tail` bytes of what follows them: the image ends where the allocation's
    # payload ends, the guard behind it is not part of it
    cut = data[512 * (8191 - blocks):512 * 8191 + tail]
    t, ptr = _upload(cut)
    st, flags, ms = _classify(ctx, ptr, len(cut))
    assert st == N.OK and ms >= 0
    assert flags[:blocks] == want[8191 - blocks:]
    assert flags[blocks] == 0xEE  # no flag for the partial block
    assert _bytes(t) == bytes([0xA5]) * GUARD + cut + bytes([0xA5]) * GUARD


def test_short_images_launch_nothing(ctx):
    for n in (0, 1, 511):
        t, ptr = _upload(b"\1" * n)
        assert _classify(ctx, ptr, n) == (N.OK, b"\xee", 0.0)
        table = lzma_amd.tar_scan_device(ctx, ptr, n)
        assert (table.entries, table.end_status, table.end_off) == ([], N.OK if n == 0 else N.ERR_UNEXPECTED_EOF, 0)
    assert lzma_amd.tar_scan_device(ctx, 0, 0) == ([], N.OK, 0)


def test_alignment_and_memory_kind(ctx):
    image = T.standard("ustar")
    t, ptr = _upload(image, shift=8)
    h = ctypes.c_void_p(7)
    assert ptr % 16 == 8
    assert N.lib().xlz_tar_scan_device(ctx._h, ctypes.c_void_p(ptr), len(image), ctypes.byref(h)) == N.ERR_BAD_ARG and not h.value
    assert _classify(ctx, ptr, len(image))[0] == N.ERR_BAD_ARG
    host = ctypes.create_string_buffer(image, len(image) + 64)
    aligned = (ctypes.addressof(host) + 15) & ~15
    assert N.lib().xlz_tar_scan_device(ctx._h, ctypes.c_void_p(aligned), 1024, ctypes.byref(h)) == N.ERR_BAD_ARG  # host memory
    t, ptr = _upload(image, shift=16)
    assert T.rows(lzma_amd.tar_scan_device(ctx, ptr, len(image)).entries) == T.judge(image)


@pytest.mark.parametrize("name", sorted(T.everything()))
def test_scan_device_equals_the_host_walk_and_tarfile(ctx, name):
    image = T.everything()[name]
    t, ptr = _upload(image)
    table = lzma_amd.tar_scan_device(ctx, ptr, len(image))
    assert table == lzma_amd.tar_parse(image) and table.end_status == N.OK
    assert T.rows(table.entries) == T.judge(image)
    assert _bytes(t) == bytes([0xA5]) * GUARD + image + bytes([0xA5]) * GUARD  # the image is only read
    s = ctx.last_tar_stats()
    flags = [T.serial_flag(image[i:i + 512]) for i in range(0, len(image), 512)]
    assert (s["blocks"], s["zero_blocks"], s["candidate_blocks"]) == (len(flags), flags.count(2), flags.count(1))
    metas, meta = _meta_entries(image)
    assert s["meta_bytes"] == meta and s["downloaded_bytes"] == len(flags) + 512 * flags.count(1) + meta
    assert s["header_blocks"] == len(table.entries) + metas
    if name in ("ustar", "gnu", "pax"):
        assert s["header_blocks"] < s["candidate_blocks"]  # the headers of the tar stored as a member are never reached
    assert s["launches"] == 1 + (flags.count(1) > 0) + (meta > 0) and s["kernel_ms"] >= 0


def _meta_entries(image):
    """(number, padded data bytes) of the 'L', 'K', 'x' and 'g' entries of a well-formed archive: whatever lies between the
    end of one member and the header of the next"""
    def pad(n):
        return -(-n // 512) * 512
    count = data = at = 0
    for m in T.judge(image):
        while at < m[9] - 512:
            size = int(image[at + 124:at + 136].strip(b" \0"), 8)
            count, data, at = count + 1, data + pad(size), at + 512 + pad(size)
        at = m[9] + (0 if b"1" <= m[3] <= b"6" else pad(m[2]))
    return count, data


@pytest.mark.parametrize("name", sorted(T.damaged()))
def test_damaged_archives_end_as_on_the_host(ctx, name):
    image, status, listed = T.damaged()[name]
    t, ptr = _upload(image)
    table = lzma_amd.tar_scan_device(ctx, ptr, len(image))
    assert table == lzma_amd.tar_parse(image)
    assert (table.end_status, len(table.entries)) == (getattr(N, status), listed)


def test_xz_tar_tensor_member_views(ctx):
    import torch
    image = T.standard("gnu")
    t, entries, end = lzma_amd.xz_tar_tensor(ctx, lzma.compress(image))
    assert end == N.OK and isinstance(t, torch.Tensor) and t.numel() == len(image)
    with tarfile.open(fileobj=io.BytesIO(image)) as tf:
        members = tf.getmembers()
        assert [e.name for e in entries] == [m.name for m in members]
        for e, m in zip(entries, members):
            if m.isreg():
                view = t[e.data_off:e.data_off + e.size]
                assert view.numel() == 0 or view.data_ptr() == t.data_ptr() + e.data_off  # a view, no copy (torch gives an empty one no address)
                assert _bytes(view) == tf.extractfile(m).read()
    t, entries, end = lzma_amd.xz_tar_tensor(ctx, lzma.compress(b""))
    assert (t.numel(), entries, end) == (0, [], N.OK)


@pytest.fixture(scope="module")
def twelve_blocks():
    """a tar of 40 members of 1-4000 bytes as a 12-block .xz with CRC64 checks; no block edge is a multiple of 512"""
    rng = random.Random(12)
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w", format=tarfile.GNU_FORMAT) as tf:
        for i in range(40):
            body = bytes(rng.randrange(32, 127) for _ in range(rng.randrange(1, 4000)))
            name = "sample-%04d.txt" % i if i % 7 else "long/" + "n" * 120 + "-%04d.txt" % i
            ti = tarfile.TarInfo(name)
            ti.size, ti.mtime = len(body), T.MTIME + i
            tf.addfile(ti, io.BytesIO(body))
    image = buf.getvalue()
    edges = [0] + [len(image) * k // 12 // 512 * 512 + 37 + 16 * k for k in range(1, 12)] + [len(image)]
    assert all(e % 512 for e in edges[1:-1]) and edges == sorted(set(edges))
    blocks = [(image[a:b], [xz_chains.LZMA2]) for a, b in zip(edges, edges[1:])]
    return image, xz_chains.stream(blocks, check=lzma.CHECK_CRC64), edges


def test_tar_xz_file_lists_and_reads_chosen_members(ctx, twelve_blocks):
    image, data, edges = twelve_blocks
    assert lzma.decompress(data) == image
    with tarfile.open(fileobj=io.BytesIO(image)) as tf:
        bodies = {m.name: tf.extractfile(m).read() for m in tf.getmembers()}
    with lzma_amd.TarXzFile(data) as f:
        assert len(f.xz.blocks) == 12 and f.entries is None
        entries = f.list(ctx)
        assert T.rows(entries) == T.judge(image) and f.end_status == N.OK and f.names == [e.name for e in entries]
        assert ctx.last_xz_read_stats()["blocks"] == 12 and ctx.last_tar_stats()["header_blocks"] == 40 + 6
        # three members whose bytes lie in two .xz blocks: only those are decoded
        for i in range(len(entries) - 2):
            spans = [f.span(k) for k in (i, i + 1, i + 2)]
            if len(f.xz.cover(spans)) == 2:
                break
        else:
            raise AssertionError("no three members in two blocks")
        want = [i + 2, i, i + 1]
        got = f.read_many(ctx, want)
        assert got == [bodies[entries[k].name] for k in want]
        assert ctx.last_xz_read_stats()["blocks"] == len(f.xz.cover([f.span(k) for k in want])) == 2 < 12
        assert f.read(ctx, entries[7].name) == bodies[entries[7].name]
        assert _bytes(f.read_tensor(ctx, 39)) == bodies[entries[39].name]
        with pytest.raises(KeyError):
            f.index("no such member")


def test_tar_xz_file_on_a_damaged_block_and_an_empty_archive(ctx, twelve_blocks):
    image, data, edges = twelve_blocks
    with lzma_amd.XzFile(data) as x:
        third = x.blocks[2]
    bad = bytearray(data)
    bad[third["comp_off"] + third["comp_len"] // 2] ^= 0x10
    bad = bytes(bad)
    with pytest.raises(LzmaError) as whole:
        lzma_amd.xz_decode(ctx, bad)
    with lzma_amd.TarXzFile(bad) as f:
        with pytest.raises(LzmaError) as e:
            f.list(ctx)
        assert e.value.status == whole.value.status and f.entries is None
    with lzma_amd.TarXzFile(lzma.compress(bytes(1024))) as f:
        assert f.list(ctx) == [] and f.end_status == N.OK and f.end_off == 0
        assert ctx.last_tar_stats()["zero_blocks"] == 2
    cut = T.damaged()["cut_in_data"][0]
    with lzma_amd.TarXzFile(lzma.compress(cut)) as f:
        with pytest.raises(LzmaError) as e:
            f.list(ctx)
        assert e.value.status == N.ERR_UNEXPECTED_EOF and len(f.entries) == 2
        assert len(f.list(ctx, strict=False)) == 2


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_classify_kernel_over_many_rounds(ctx, mixed_image):
    """an image of three times as many blocks as one round of the grid takes (8 workgroups per CU x 8 pairs x 2 blocks), and
    more: the fixture's 8191 blocks tiled -- an odd number, so every repetition shifts which half of a pair a header falls
    in -- and 511 trailing bytes.  The flags are the fixture's flags tiled: no block is judged again"""
    t_start = time.time()
    data, want = mixed_image
    cus = _cus()
    reps = -(-(3 * 128 * cus + 1) // 8191)
    blocks = 8191 * reps
    assert blocks >= 3 * 128 * cus + 1
    image = data[:512 * 8191] * reps + data[512 * 8191:]
    assert len(image) == 512 * blocks + 511
    t, ptr = _upload(image)
    st, flags, ms = _classify(ctx, ptr, len(image))
    print("classify: %d blocks = %d pairs on %d CUs, %d pairs per round: %.2f rounds; kernel %.3f ms"
          % (blocks, -(-blocks // 2), cus, 64 * cus, -(-blocks // 2) / (64.0 * cus), ms))
    assert st == N.OK and ms > 0
    assert flags[:blocks] == want * reps
    assert flags[blocks] == 0xEE  # no flag for the partial block
    assert _bytes(t) == bytes([0xA5]) * GUARD + image + bytes([0xA5]) * GUARD  # the image and its guards are only read
    print("test_classify_kernel_over_many_rounds: %.1f s wall" % (time.time() - t_start))


def test_gather_kernel_over_many_rounds(ctx):
    """an archive of three times as many header blocks as one round of the gather's grid takes (8 workgroups per CU x 256
    threads, a thread per 16 bytes: 64 blocks per CU), and one more: empty members, every block a candidate"""
    t_start = time.time()
    cus = _cus()
    members = 3 * 64 * cus + 1
    assert members >= 3 * 64 * cus + 1
    image = b"".join(T.header(b"many/%07d.txt" % i, mtime=T.MTIME + i, mode=0o600 + i % 64) for i in range(members)) + bytes(1024)
    t, ptr = _upload(image)
    table = lzma_amd.tar_scan_device(ctx, ptr, len(image))
    s = ctx.last_tar_stats()
    print("gather: %d candidate blocks on %d CUs, %d blocks per round: %.2f rounds; stats %s" % (members, cus, 64 * cus, members / (64.0 * cus), s))
    assert table == lzma_amd.tar_parse(image) and table.end_status == N.OK and len(table.entries) == members
    assert T.rows(table.entries) == T.judge(image)
    assert s["candidate_blocks"] == members == s["header_blocks"] and (s["blocks"], s["zero_blocks"]) == (members + 2, 2)
    assert s["launches"] == 2 and s["meta_bytes"] == 0
    assert _bytes(t) == bytes([0xA5]) * GUARD + image + bytes([0xA5]) * GUARD
    print("test_gather_kernel_over_many_rounds: %.1f s wall" % (time.time() - t_start))
