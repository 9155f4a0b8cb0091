"""Dev tool (GPU box): what listing a .tar.xz on the device costs (lzma_amd/csrc/xlz_tar_dev.hip),
in one process.
    python tools/tar_bench.py [--image-mib 1024] [--members 4096] [--member-kib 64] [--calls 7] > profiles/device_tar.txt

(a) The classify kernel alone on an image of --image-mib MiB in device memory (a 16 MiB mix of headers, text, random and
    zero blocks, repeated), by HIP events through xlz_internal_tar_classify_device, medians of --calls after a warm-up.
    Beside it, same box and same run, the project's other read-only HBM kernel: CRC32 of 1024 x 1 MiB ranges of a
    device-resident batch (xlz_check_dev.hip; Context.last_check_stats).
(b) TarXzFile.list (xlz_xz_tar_list) of a tarball of --members members of --member-kib KiB, one .xz block per MiB, against
    the by-hand form -- xz_decode_device, then a serial chain of one 512-byte hipMemcpy per member, each depending on the
    size field of the one before -- and against tarfile over liblzma on the host.
(c) TarXzFile.read_many of 1 % of the members against xz_decode of the whole file.
Every GPU step runs in this process under the caller's time limit."""
import ctypes
import io
import lzma
import os
import random
import statistics
import sys
import tarfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _hip():
    H = ctypes.CDLL("libamdhip64.so")
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    H.hipMalloc.argtypes = [ctypes.POINTER(vp), sz]
    H.hipFree.argtypes = [vp]
    H.hipMemcpy.argtypes = [vp, vp, sz, ctypes.c_int]
    return H


def _ok(st):
    assert st == 0, "HIP call failed: %d" % st


def _med(label, ms, n_bytes=None):
    med = statistics.median(ms)
    txt = "    %-58s median %9.3f ms (min %.3f, max %.3f, %d calls)" % (label, med, min(ms), max(ms), len(ms))
    if n_bytes:
        txt += "  %8.1f GB/s" % (n_bytes / (med * 1e-3) / 1e9)
    print(txt, flush=True)
    return med


def mixed_image(n_bytes):
    """headers, printable text, random and zero blocks: 16 MiB, repeated"""
    import tar_archives as T
    rng = random.Random(18)
    blocks = []
    while len(blocks) < (16 << 20) // 512:
        kind = rng.randrange(8)
        if kind == 0:
            blocks.append(T.header(b"member-%06d" % len(blocks), size=rng.randrange(1 << 20)))
        elif kind == 1:
            blocks += [bytes(512)] * 4
        elif kind < 5:
            blocks.append(bytes(rng.randrange(32, 127) for _ in range(512)))
        else:
            blocks.append(rng.randbytes(512))
    piece = b"".join(blocks)[:16 << 20]
    return piece * (n_bytes // len(piece)) + piece[:n_bytes % len(piece)]


def kernel_alone(ctx, H, image, cs, calls):
    from lzma_amd import _native as N
    import lzma_amd
    n_bytes = len(image)
    d = ctypes.c_void_p()
    _ok(H.hipMalloc(ctypes.byref(d), n_bytes))
    _ok(H.hipMemcpy(d, ctypes.cast(ctypes.c_char_p(image), ctypes.c_void_p), n_bytes, 1))
    flags = ctypes.create_string_buffer(n_bytes // 512 + 1)
    ms = []
    for k in range(calls + 1):
        t = ctypes.c_double()
        st = N.lib().xlz_internal_tar_classify_device(ctx._h, d, n_bytes, flags, ctypes.byref(t))
        assert st == 0, st
        if k:
            ms.append(t.value)
    raw = flags.raw[:n_bytes // 512]
    print("image of %d MiB in device memory: %d blocks, %d zero, %d header candidates" % (n_bytes >> 20, len(raw), raw.count(2), raw.count(1)), flush=True)
    _med("classify kernel (reads every byte once)", ms, n_bytes)
    _ok(H.hipFree(d))
    # the CRC32 kernel over as many bytes as fit 1024 ranges of 1 MiB, on a device-resident batch
    size, n = 1 << 20, 1024
    b = lzma_amd.Batch(ctx, [lzma_amd.Stream(cs[i % 64], out_cap=size) for i in range(n)])
    b.run()
    assert all(r[0] == size and r[1] == 0 for r in b.results())
    ms = []
    for k in range(calls + 1):
        b.checks([(i, 0, size, lzma_amd.CHECK_CRC32) for i in range(n)])
        if k:
            ms.append(ctx.last_check_stats()["kernel_ms"])
    _med("CRC32 check kernel, %d ranges of 1 MiB (xlz_check_dev)" % n, ms, n * size)
    b.close()


def tarball(members, member_bytes):
    """-> (the .tar image, the .xz file with a block per MiB)"""
    import xz_chains
    rng = random.Random(4096)
    words = [bytes(rng.randrange(97, 123) for _ in range(rng.randrange(2, 10))) for _ in range(2000)]
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w", format=tarfile.GNU_FORMAT) as tf:
        for i in range(members):
            body = b" ".join(rng.choice(words) for _ in range(member_bytes // 6))[:member_bytes].ljust(member_bytes, b".")
            ti = tarfile.TarInfo("shard/sample-%06d.txt" % i)
            ti.size, ti.mtime = len(body), 1_700_000_000
            tf.addfile(ti, io.BytesIO(body))
    image = buf.getvalue()
    filt = [{"id": lzma.FILTER_LZMA2, "preset": 0, "dict_size": 1 << 20}]
    blocks = [(image[a:a + (1 << 20)], filt) for a in range(0, len(image), 1 << 20)]
    return image, xz_chains.stream(blocks, check=lzma.CHECK_CRC64)


def by_hand(ctx, H, data, d, cap):
    """xz_decode_device, then the header chain with one small copy per member -> the member count"""
    import lzma_amd
    n = lzma_amd.xz_decode_device(ctx, data, d.value, cap)
    block = ctypes.create_string_buffer(512)
    off = count = 0
    while off + 512 <= n:
        _ok(H.hipMemcpy(ctypes.cast(block, ctypes.c_void_p), ctypes.c_void_p(d.value + off), 512, 2))
        if block.raw == bytes(512):
            break
        size = int(block.raw[124:136].strip(b" \0") or b"0", 8)
        off += 512 + -(-size // 512) * 512
        count += 1
    return count


def listing(ctx, H, image, data, members, member_bytes, calls):
    import lzma_amd
    print("tarball of %d members of %d KiB: %.1f MiB, %.1f MiB as .xz with a block per MiB" %
          (members, member_bytes >> 10, len(image) / 2**20, len(data) / 2**20), flush=True)
    d = ctypes.c_void_p()
    _ok(H.hipMalloc(ctypes.byref(d), len(image)))
    ms = {"list": [], "hand": [], "host": [], "read": [], "whole": []}
    rng = random.Random(1)
    chosen = sorted(rng.sample(range(members), max(members // 100, 1)))
    with lzma_amd.TarXzFile(data) as f:
        for k in range(calls + 1):
            t0 = time.perf_counter()
            entries = f.list(ctx)
            t1 = time.perf_counter()
            count = by_hand(ctx, H, data, d, len(image))
            t2 = time.perf_counter()
            got = f.read_many(ctx, chosen)
            t3 = time.perf_counter()
            whole = lzma_amd.xz_decode(ctx, data)
            t4 = time.perf_counter()
            assert len(entries) == count == members and whole == image
            assert all(g == image[entries[i].data_off:entries[i].data_off + entries[i].size] for g, i in zip(got, chosen))
            if k:
                ms["list"].append((t1 - t0) * 1e3), ms["hand"].append((t2 - t1) * 1e3), ms["read"].append((t3 - t2) * 1e3), ms["whole"].append((t4 - t3) * 1e3)
            elif k == 0:
                print("    statistics of the listing: %s" % ctx.last_tar_stats(), flush=True)
                f.read_many(ctx, chosen)
                print("    statistics of the read of %d members: %s" % (len(chosen), ctx.last_xz_read_stats()), flush=True)
        for k in range(3):
            t0 = time.perf_counter()
            with tarfile.open(fileobj=io.BytesIO(lzma.decompress(data))) as tf:
                assert len(tf.getmembers()) == members
            ms["host"].append((time.perf_counter() - t0) * 1e3)
    _ok(H.hipFree(d))
    a = _med("TarXzFile.list (decode into scratch, classify, gather, walk)", ms["list"])
    b = _med("by hand: xz_decode_device + one 512-byte copy per member", ms["hand"])
    c = _med("host: tarfile over lzma.decompress (one thread)", ms["host"])
    print("    list / by hand: %.2f x; list / host: %.2f x" % (a / b, a / c), flush=True)
    r = _med("TarXzFile.read_many of %d members (1 %%)" % len(chosen), ms["read"])
    w = _med("xz_decode of the whole file (host to host)", ms["whole"])
    print("    read of 1 %% / whole file: %.2f x" % (r / w), flush=True)


def main():
    args = sys.argv[1:]
    image_mib, members, member_kib, calls = 1024, 4096, 64, 7
    while args:
        a = args.pop(0)
        if a == "--image-mib":
            image_mib = int(args.pop(0))
        elif a == "--members":
            members = int(args.pop(0))
        elif a == "--member-kib":
            member_kib = int(args.pop(0))
        elif a == "--calls":
            calls = int(args.pop(0))
        else:
            raise SystemExit("unknown argument " + a)
    import lzma_amd
    from lzma_amd import _native as N
    info = N.library_info()
    print("library build %s, decode kernels %s; classify kernel: a wave per pair of 512-byte blocks, 16 bytes per lane, at most 8 workgroups "
          "of 256 per CU" % (info["build_id"], info["kernel_id"]), flush=True)
    # (everything the host makes, worker processes included, is done before this process opens the device)
    import corpus
    cs, _ = corpus.make_alone_batch("T", 64, 1 << 20, base_seed=801, workers=16, preset=0)
    mixed = mixed_image(image_mib << 20)
    image, data = tarball(members, member_kib << 10)
    H = _hip()
    ctx = lzma_amd.Context(0)
    kernel_alone(ctx, H, mixed, cs, calls)
    del mixed
    listing(ctx, H, image, data, members, member_kib << 10, calls)


if __name__ == "__main__":
    main()
