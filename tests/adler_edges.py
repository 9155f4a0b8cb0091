"""The edge list of the device Adler-32 (lzma_amd/csrc/xlz_adler_dev.h), shared by tests/test_adler_dev.py (the lane-by-lane
scheme on the CPU) and tests/test_gpu_adler.py (the kernels): ONE buffer of 4 MiB and ranges of it, every one with the
names of the edges it sits on.  The judge is zlib.adler32."""
import random
import zlib

SEG = 128 * 1024          # xlzchk::kSegBytes: one wave's share
ROW = 1024                # 64 lanes x 16 bytes
MAX_LANE_ROWS = 1451      # xlzadl::kMaxLaneRows: rows of 0xFF bytes a lane's sums hold before a reduction is due
DEFERRAL = MAX_LANE_ROWS * ROW

LENGTHS = {"len_0": 0, "len_1": 1, "len_15": 15, "len_16": 16, "len_17": 17, "len_1023": 1023, "len_1024": 1024, "len_1025": 1025,
           "nmax_minus_1": 5551, "nmax": 5552, "nmax_plus_1": 5553, "seg_minus_1": SEG - 1, "seg": SEG, "seg_plus_1": SEG + 1,
           "three_segs_plus_1": 3 * SEG + 1}
OFFSETS = {"residue16_%d" % k: k for k in range(16)}
OFFSETS.update({"residue128_0": 0, "residue128_127": 127, "residue128_128": 128})
REGIONS = {"content_random": (0, 512 * 1024), "content_zero": (512 * 1024, 512 * 1024), "content_ff": (1024 * 1024, 3 * 1024 * 1024)}
BUF_LEN = 4 * 1024 * 1024
EDGES = sorted(list(LENGTHS) + list(OFFSETS) + list(REGIONS) + ["deferral_bound_twice"])


def buffer():
    r = random.Random("adler-edges")
    buf = bytearray(BUF_LEN)
    lo, n = REGIONS["content_random"]
    buf[lo:lo + n] = r.randbytes(n)
    lo, n = REGIONS["content_ff"]
    buf[lo:lo + n] = b"\xff" * n
    return bytes(buf)


def ranges():
    """-> [(off, len, {edge names})]"""
    out = []
    for ln_name, ln in LENGTHS.items():
        for off_name, off in OFFSETS.items():
            out.append((REGIONS["content_random"][0] + 256 + off, ln, {ln_name, off_name, "content_random"}))
        for region in ("content_zero", "content_ff"):
            for off_name in ("residue128_0", "residue16_5", "residue128_127"):
                out.append((REGIONS[region][0] + 256 + OFFSETS[off_name], ln, {ln_name, off_name, region}))
    # 0xFF bytes past the deferral bound twice over: every sum that is reduced too late wraps here
    out.append((REGIONS["content_ff"][0] + 3, 2 * DEFERRAL + 1, {"deferral_bound_twice", "content_ff", "residue16_3"}))
    for off, ln, _ in out:
        assert off + ln <= BUF_LEN
    return out


def expected(buf, rs):
    view = memoryview(buf)
    return [zlib.adler32(view[off:off + ln]) for off, ln, _ in rs]
