"""CPU: .bz2 files (lzma_amd/csrc/xlz_bz2_dev.h, xlz_bz2.h) -- the serial twin through bzip2.decode_host and the LANE SCHEME
of the kernels through tests/c/bz2_dev_selftest.cpp (g++, lane by lane, once more under -fsanitize=address,undefined), on the
cases of tests/bz2_files.py.  The judge is Python's bz2: every case agrees with it on accept / reject, on the class of a
reject (a defect against input that merely ends) and, where accepted, on every byte and on where the last good stream ended."""
import bz2
import collections
import ctypes
import os
import subprocess

import pytest

import bz2_craft as craft
import bz2_files as F
from lzma_amd import _native as N
from lzma_amd import bzip2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_class(got, want):
    """a randomised block is ERR_UNSUPPORTED here and a defect to the yardstick"""
    return got == want or (want == F.ERR_RESULT and got == F.ERR_UNSUPPORTED)


def test_the_new_symbols_and_struct_sizes(xlz_so):
    L = N.lib()
    for name in ("xlz_bz2_probe", "xlz_bz2_decode_host", "xlz_bz2_decode_many_device", "xlz_bz2_decode_many", "xlz_ctx_last_bz2_stats",
                 "xlz_ctx_set_bz2_mode", "xlz_ctx_bz2_mode", "xlz_ctx_set_bz2_scratch", "xlz_crc32_bzip2_host"):
        assert name in N.EXPORTS and hasattr(L, name), name
    sizes = {N.Bz2Info: 40, N.Bz2File: 32, N.Bz2Result: 32, N.Bz2Stats: 112}
    for struct_, size in sizes.items():
        assert ctypes.sizeof(struct_) == size, struct_
        assert sum(ctypes.sizeof(t) for _, t in struct_._fields_) == size, struct_   # (no implicit padding)


def test_the_yardstick_mirror_is_bz2_decompress():
    """bz2_files.yardstick re-runs bz2.decompress's loop to learn in_consumed: the two must agree on every case"""
    for (name, f), (st, data, used) in zip(F.cases(), F.expected()):
        try:
            want = (F.OK, bz2.decompress(f))
        except OSError:
            want = (F.ERR_RESULT, None)
        except ValueError:
            want = (F.ERR_UNEXPECTED_EOF, None)
        assert (st, data) == want, name
        assert st != F.OK or 0 <= used <= len(f), name


def test_the_case_list_bites_by_the_yardstick_alone():
    ex = dict(zip((n for n, _ in F.cases()), F.expected()))
    # every crafted or compressed shape and file decodes under bz2 (to what the writer meant: bz2_craft puts the CRC of the
    # intended bytes into the block, and bz2 compares it) ...
    for name, _ in F.shape_cases():
        assert ex[name][0] == F.OK, name
    assert ex["zero_run_full"][1] == craft.long_run_block(0, 100000)[1] and len(ex["full_level9"][1]) == 899900
    assert ex["fours_of_4"][1] == b"\x04" * 1800 and ex["fours_of_255"][1] == craft.unrle1(b"\xff" * 322)
    # ... every defect is refused by it, as a defect ...
    for name, _ in F.defect_cases():
        assert ex[name][0] == F.ERR_RESULT, name
    # ... and the files are of the classes their names say
    for name in ("then_junk", "then_junk_magic", "then_junk_magic_bits", "then_damaged", "then_bad_level"):
        assert ex[name][0] == F.OK and ex[name][2] == len(F.file_cases()[2][1]), name
    assert ex["then_cut"][0] == ex["then_cut_header"][0] == F.ERR_UNEXPECTED_EOF
    assert ex["damaged_first"][0] == ex["bad_header"][0] == F.ERR_RESULT
    assert ex["empty_stream"] == (F.OK, b"", 14) and ex["no_bytes"] == (F.OK, b"", 0)
    seen = collections.Counter(st for (n, _), (st, _, _) in zip(F.cases(), F.expected()) if n.startswith("mut"))
    assert min(seen[F.OK], seen[F.ERR_RESULT]) >= 100 and seen[F.ERR_UNEXPECTED_EOF] >= 5, seen


def test_the_files_cover_all_eight_bit_offsets_of_a_block_start(xlz_so):
    offsets, blocks = set(), 0
    for name, f in F.file_cases():
        if not name.startswith("blocks15"):
            continue
        info = bzip2.probe(f)
        assert info["level"] == 1 and info["streams"] == 1 and info["candidates"] >= 14, (name, info)
        blocks += info["candidates"]
        at = 0
        for s in range(8):   # the magic at bit s of a byte: its 48 bits lie in seven bytes, of which the inner five are fixed
            field = craft.BLOCK_MAGIC << (8 - s)
            inner, j = field.to_bytes(7, "big")[1:6], -1
            while (j := f.find(inner, j + 1)) >= 1:
                if j + 6 <= len(f) and (int.from_bytes(f[j - 1:j + 6], "big") >> (8 - s)) & 0xFFFFFFFFFFFF == craft.BLOCK_MAGIC:
                    offsets.add(s)
                    at += 1
        assert at == info["candidates"], name   # the probe's scan against a search of its own
    assert offsets == set(range(8)), offsets


def test_probe(xlz_so):
    info = bzip2.probe(dict(F.cases())["then_junk_magic"])
    assert info["candidates"] == 2 and info["streams"] == 1 and info["level"] == 1
    info = bzip2.probe(dict(F.cases())["three_streams_one_empty"])
    assert info["candidates"] == 2 and info["streams"] == 3
    assert info["size_hint"] == 2 * 100000 and info["size_bound"] >= 2 * 900000 * 51
    for bad, st in ((b"", F.ERR_UNEXPECTED_EOF), (b"BZh", F.ERR_UNEXPECTED_EOF), (b"BZh0....", F.ERR_RESULT), (b"XZh9....", F.ERR_RESULT)):
        with pytest.raises(Exception) as e:
            bzip2.probe(bad)
        assert e.value.status == st


def test_the_twin_equals_bz2_on_every_case(xlz_so):
    for (name, f), (st, data, used) in zip(F.cases(), F.expected()):
        got = bzip2.decode_host(f, len(data) if data is not None else 5000)
        assert same_class(got[1], st), (name, got[1:], st)
        if st == F.OK:
            assert got[0] == data and got[2] == len(data) and got[3] == used, name
        else:
            assert got[0] is None and got[2] == 0 and got[3] == 0, name
    d = dict(F.cases())
    assert bzip2.decode_host(d["defect_random"], 5000)[1] == F.ERR_UNSUPPORTED
    assert bzip2.decode_host(d["three_streams_one_empty"], 5000)[4:] == (2, 3)
    assert bzip2.decode_host(d["then_damaged"], 5000)[4:] == (1, 1)


@pytest.mark.parametrize("name", ["one_block", "blocks15_seed31", "two_streams", "then_damaged", "x260", "empty_stream"])
def test_out_cap_short_and_zero_report_the_true_size(xlz_so, name):
    f = dict(F.cases())[name]
    data = bz2.decompress(f)
    for cap in sorted({0, max(len(data) - 1, 0)}):
        got = bzip2.decode_host(f, cap)
        if cap >= len(data):
            assert got[:3] == (data, F.OK, len(data))
        else:
            assert got[:4] == (None, F.ERR_OUT_CAP, len(data), 0), (name, cap)
    assert bzip2.decode_host(f, len(data) + 7)[:3] == (data, F.OK, len(data))


def test_verify_off_skips_the_crcs_only(xlz_so):
    d = dict(F.cases())
    assert bzip2.decode_host(d["defect_crc"], 5000, verify=False)[1] == F.OK
    assert bzip2.decode_host(d["defect_combined"], 5000, verify=False)[1] == F.OK
    assert bzip2.decode_host(d["defect_orig"], 5000, verify=False)[1] == F.ERR_RESULT


def test_crc32_bzip2_against_the_bitwise_definition(xlz_so):
    assert bzip2.crc32_bzip2(b"123456789") == 0xFC891918 == craft.crc32_bzip2(b"123456789")
    data = F.noise(3000, 5)
    for n in (0, 1, 2, 3, 4, 5, 255, 256, 257, 3000):
        assert bzip2.crc32_bzip2(data[:n]) == craft.crc32_bzip2(data[:n]), n
    assert bzip2.crc32_bzip2(data[1000:], bzip2.crc32_bzip2(data[:1000])) == craft.crc32_bzip2(data)


def test_arguments_are_refused_before_the_context_is_used(xlz_so):
    L = N.lib()
    bad = -7
    assert L.xlz_bz2_probe(None, 0, None) == bad and L.xlz_bz2_probe(None, 5, ctypes.byref(N.Bz2Info())) == bad
    assert L.xlz_bz2_decode_host(None, 0, None, 0, 1, None) == bad
    assert L.xlz_bz2_decode_host(None, 3, None, 0, 1, ctypes.byref(N.Bz2Result())) == bad
    assert L.xlz_bz2_decode_many(None, None, 0, None, 0, 1, None) == bad and L.xlz_bz2_decode_many_device(None, None, 0, None, 0, 1, None) == bad
    assert L.xlz_ctx_last_bz2_stats(None, ctypes.byref(N.Bz2Stats())) == bad
    assert L.xlz_ctx_set_bz2_mode(None, 1) == bad and L.xlz_ctx_set_bz2_scratch(None, 0) == bad and L.xlz_ctx_bz2_mode(None) == bad
    # the windows and the pointers, with a context that must not be looked at: it is no context at all
    not_a_ctx = ctypes.c_void_p(16)
    data = ctypes.create_string_buffer(bz2.compress(b"abc"))
    out = ctypes.create_string_buffer(100)
    res = (N.Bz2Result * 2)()

    def call(files, n, dst, cap, device=False):
        arr = (N.Bz2File * 2)()
        for i, (p, ln, off, c) in enumerate(files):
            arr[i].inp, arr[i].in_len, arr[i].dst_off, arr[i].dst_cap = p, ln, off, c
        f = L.xlz_bz2_decode_many_device if device else L.xlz_bz2_decode_many
        return f(not_a_ctx, arr, n, dst, cap, 1, res)

    p, ln = ctypes.addressof(data), len(data) - 1
    for device in (False, True):
        assert call([(p, ln, 0, 60), (p, ln, 59, 10)], 2, out, 100, device) == bad   # two windows share a byte
        assert call([(p, ln, 0, 60), (p, ln, 60, 41)], 2, out, 100, device) == bad   # a window past the capacity
        assert call([(p, ln, 101, 0)], 1, out, 100, device) == bad                   # an empty window past the capacity
        assert call([(None, 5, 0, 10)], 1, out, 100, device) == bad                  # a length without a pointer
        assert call([(p, ln, 0, 10)], 1, None, 100, device) == bad                   # a capacity without a destination
        assert L.xlz_bz2_decode_many(not_a_ctx, None, 1, out, 100, 1, res) == bad and L.xlz_bz2_decode_many(not_a_ctx, (N.Bz2File * 2)(), 1, out, 100, 1, None) == bad
        assert (L.xlz_bz2_decode_many_device if device else L.xlz_bz2_decode_many)(not_a_ctx, None, 0, None, 0, 1, None) == 0   # n = 0


def _build(tmp, src, flags, tag):
    exe = str(tmp / (src + tag))
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-Wall"] + flags + ["-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", src + ".cpp"), "-o", exe])
    return exe


SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _run_list(exe, tmp, jobs):
    """jobs: [(name, file, out_cap)] through --list in one run -> [(status, out_len, in_consumed, blocks, streams, bytes or None)]"""
    with open(tmp / "list.txt", "w") as lst, open(tmp / "in.bin", "wb") as blob:
        for _, f, cap in jobs:
            lst.write("%d %d\n" % (len(f), cap))
            blob.write(f)
    run = subprocess.run([exe, "--list", str(tmp / "list.txt"), str(tmp / "in.bin"), str(tmp / "out.bin"), str(tmp / "res.txt")],
                         capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    _run_list.stdout = run.stdout
    res = [tuple(int(x) for x in line.split()) for line in open(tmp / "res.txt")]
    assert len(res) == len(jobs)
    out = []
    with open(tmp / "out.bin", "rb") as got:
        for r in res:
            out.append(r + (got.read(r[1]) if r[0] == F.OK else None,))
        assert got.read(1) == b""
    return out


def _lane_jobs(mutations):
    jobs = []
    for (name, f), (st, data, used) in zip(F.cases(), F.expected()):
        if name.startswith("mut") and int(name[3:]) >= mutations:
            continue
        jobs.append((name, f, len(data) if data is not None else 5000))
    return jobs


def _check_lanes(exe, tmp, jobs):
    ex = dict(zip((n for n, _ in F.cases()), F.expected()))
    for (name, f, cap), got in zip(jobs, _run_list(exe, tmp, jobs)):
        st, data, used = ex[name]
        assert same_class(got[0], st), (name, got[:5], st)
        if st == F.OK:
            assert got[5] == data and got[2] == used, name
        assert got[:5] == bzip2.decode_host(f, cap)[1:], name   # and status, sizes and counts are the twin's exactly


def test_the_lane_scheme_equals_bz2_on_every_case(xlz_so, tmp_path):
    exe = _build(tmp_path, "bz2_dev_selftest", ["-O2"], "")
    assert subprocess.run([exe], capture_output=True, text=True).stdout.strip() == "ok"
    _check_lanes(exe, tmp_path, _lane_jobs(F.MUTATION_SEEDS))
    # marks_avoided and marks_avoided_small, and they alone, exceed a lane's share of the walk: the twin decodes them instead
    assert _run_list.stdout.strip() == "gave up 2"


def test_the_lane_scheme_under_sanitizers(xlz_so, tmp_path):
    """the same program built with -fsanitize=address,undefined, stand-alone: the shapes, files, defects, cuts and 300 mutations"""
    exe = _build(tmp_path, "bz2_dev_selftest", SANITIZE, "_san")
    assert subprocess.run([exe], capture_output=True, text=True).stdout.strip() == "ok"
    _check_lanes(exe, tmp_path, _lane_jobs(300))


def test_the_lane_scheme_out_cap(xlz_so, tmp_path):
    exe = _build(tmp_path, "bz2_dev_selftest", ["-O2"], "")
    d = dict(F.cases())
    jobs = [(n, d[n], cap) for n in ("one_block", "two_streams", "then_damaged", "x260") for cap in (0, len(bz2.decompress(d[n])) - 1)]
    for (name, f, cap), got in zip(jobs, _run_list(exe, tmp_path, jobs)):
        assert got[:5] == (F.ERR_OUT_CAP, len(bz2.decompress(f)), 0, 0, 0), (name, cap)


def test_fuzz_under_sanitizers(xlz_so, tmp_path):
    exe = _build(tmp_path, "bz2_fuzz", SANITIZE, "_san")
    d = dict(F.cases())
    paths = []
    for name in ("one_block", "two_streams", "groups3_deep", "then_junk_magic", "x260_fours", "all256"):
        paths.append(str(tmp_path / name))
        with open(paths[-1], "wb") as fh:
            fh.write(d[name])
    run = subprocess.run([exe, "3000"] + paths, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout[-2000:] + run.stderr[-4000:]
