"""Dev tool (GPU box): what the extraction of chosen files of a .7z archive (SevenZipFile: xlz_7z_open /
xlz_7z_extract_device) costs, in one process.
    python tools/sevenzip_extract_bench.py [--folders 64] [--files 16] [--size 65536] [--calls 7] > profiles/sevenzip_extract.txt

Two archives written by tests/sevenzip_files.py, payloads from liblzma: FOLDERS solid LZMA folders of FILES files of SIZE
bytes, and the same as LZMA2 folders of one unit per file.  Per archive, each against xlz_7z_decode_device of the whole
archive on the same context -- without the extraction the only way to those bytes --: the first file of one folder, the
last file of one folder, one file per folder, every file.  The five calls alternate; medians of 7 after a warm-up round
that also compares the bytes.  Beside each time: decoded_bytes / folder_bytes of the call (xlz_7z_extract_stats) -- what the
batch was asked to decode of the covering folders' sizes.  Every GPU step runs in this process under the caller's time limit."""
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

D2H = 2  # hipMemcpyDeviceToHost


def _hip():
    """the HIP runtime libxlz.so has loaded (and no second one)"""
    path = "libamdhip64.so"
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                path = line.split()[-1]
                break
    H = ctypes.CDLL(path)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    H.hipMalloc.argtypes = [ctypes.POINTER(vp), sz]
    H.hipFree.argtypes = [vp]
    H.hipMemcpy.argtypes = [vp, vp, sz, ctypes.c_int]
    return H


def _ok(st):
    assert st == 0, "HIP call failed: %d" % st


def _spread(label, ms):
    print("    %-52s median %9.3f ms  min %9.3f  max %9.3f  (%d calls)" % (label, statistics.median(ms), min(ms), max(ms), len(ms)), flush=True)
    return statistics.median(ms)


def _file(folder, k, size):
    """compressible and different from its neighbours: a line of text per 64 bytes"""
    line = ("folder %05d file %03d " % (folder, k)).encode()
    out = bytearray()
    i = 0
    while len(out) < size:
        out += line + b"%09d " % (i * 2654435761 % 1000000007) + b"lorem ipsum dolor sit amet\n"
        i += 1
    return bytes(out[:size])


def archives(n_folders, n_files, size):
    import sevenzip_bcj2 as B
    import sevenzip_craft as C
    import sevenzip_files as F
    groups = [[_file(f, k, size) for k in range(n_files)] for f in range(n_folders)]
    entries = [F.entry("d%03d/f%03d.txt" % (f, k)) for f in range(n_folders) for k in range(n_files)]
    solid, units = [], []
    for g in groups:
        rec, pk = C.lzma_folder(b"".join(g), dict_size=1 << 20)
        solid.append(B.plain_folder(rec, pk, g))
        rec, pk = F.lzma2_units_folder(g, dict_byte=18)
        units.append(B.plain_folder(rec, pk, g))
    return groups, [("solid LZMA folders", F.archive(solid, entries)), ("LZMA2 folders, one unit per file", F.archive(units, entries))]


def run(ctx, H, name, arc, groups, calls):
    import lzma_amd
    n_folders, n_files = len(groups), len(groups[0])
    total = sum(len(x) for g in groups for x in g)
    print("%s: %d folders x %d files x %d bytes (%.1f MiB, %.1f MiB compressed), verify on:"
          % (name, n_folders, n_files, len(groups[0][0]), total / 2**20, len(arc) / 2**20), flush=True)
    z = lzma_amd.SevenZipFile(arc)
    mid = n_folders // 2
    cases = [
        ("the first file of one folder", [mid * n_files]),
        ("the last file of one folder", [mid * n_files + n_files - 1]),
        ("one file per folder", [f * n_files + (f * 7) % n_files for f in range(n_folders)]),
        ("every file", list(range(n_folders * n_files))),
    ]
    whole, dst = ctypes.c_void_p(), ctypes.c_void_p()
    _ok(H.hipMalloc(ctypes.byref(whole), total))
    _ok(H.hipMalloc(ctypes.byref(dst), total))
    ms = {c[0]: [] for c in cases}
    ms["whole"] = []
    stats = {}
    for k in range(calls + 1):
        t0 = time.perf_counter()
        n = lzma_amd.sevenzip_decode_device(ctx, arc, whole.value, total)
        dt = (time.perf_counter() - t0) * 1e3
        assert n == total
        if k:
            ms["whole"].append(dt)
        for label, idx in cases:
            wants, need = z.layout(idx)
            t0 = time.perf_counter()
            res = z.extract_device(ctx, wants, dst.value, total)
            dt = (time.perf_counter() - t0) * 1e3
            assert all(st == 0 for st, _, _ in res), label
            if k:
                ms[label].append(dt)
                continue
            stats[label] = ctx.last_7z_extract_stats()
            got = (ctypes.c_char * need)()
            _ok(H.hipMemcpy(ctypes.cast(got, ctypes.c_void_p), dst, need, D2H))
            want = b"".join(groups[i // n_files][i % n_files] for i in idx)
            assert got.raw == want, "wrong bytes: " + label
    w = _spread("sevenzip_decode_device of the whole archive", ms["whole"])
    for label, idx in cases:
        m = _spread("extract_device of " + label, ms[label])
        s = stats[label]
        print("        %d folders in the batch, decoded_bytes / folder_bytes = %d / %d (%.3f), %d bytes copied; whole archive / extraction: %.2f x"
              % (s["folders"], s["decoded_bytes"], s["folder_bytes"], s["decoded_bytes"] / max(s["folder_bytes"], 1), s["copied_bytes"], w / m), flush=True)
    _ok(H.hipFree(whole))
    _ok(H.hipFree(dst))
    z.close()


def main():
    args = sys.argv[1:]
    n_folders, n_files, size, calls = 64, 16, 65536, 7
    while args:
        a = args.pop(0)
        if a == "--folders":
            n_folders = int(args.pop(0))
        elif a == "--files":
            n_files = int(args.pop(0))
        elif a == "--size":
            size = int(args.pop(0))
        elif a == "--calls":
            calls = int(args.pop(0))
        else:
            raise SystemExit("unknown argument " + a)
    import lzma_amd
    from lzma_amd import _native as N
    info = N.library_info()
    print("library build %s, decode kernels %s" % (info["build_id"], info["kernel_id"]), flush=True)
    groups, arcs = archives(n_folders, n_files, size)
    ctx = lzma_amd.Context(0)
    H = _hip()
    for name, arc in arcs:
        run(ctx, H, name, arc, groups, calls)


if __name__ == "__main__":
    main()
