"""CPU: the shared window header (lzma_amd/csrc/xlz_windows.h) -- "disjoint windows inside a capacity" and "windows back
to back at an alignment" as every container front end asks them -- in a g++ program of its own
(tests/c/windows_selftest.cpp) against brute-force byte-map models, plain and under the host sanitizers; and that it is
host code of the library's build, over the standard library alone."""
import os
import re
import subprocess

import pytest

from lzma_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lzma_amd", "csrc")


def test_windows_header_is_host_code():
    assert "xlz_windows.h" in build.HEADERS and "xlz_windows.h" not in build.KERNEL_FILES
    text = open(os.path.join(CSRC, "xlz_windows.h")).read()
    assert "hip" not in text.lower()  # plain C++: nothing of the runtime, not even a file's name
    includes = re.findall(r"#include\s+(\S+)", text)
    assert includes and all(i.startswith("<") for i in includes)  # the standard library alone: usable wherever xlz_zip.h is
    for user in ("xlz_zip.h", "xlz_7z_files.h", "xlz_xz_many.h", "xlz_post.h"):
        assert '#include "xlz_windows.h"' in open(os.path.join(CSRC, user)).read(), user


def _selftest(tmp_path, flags):
    exe = str(tmp_path / "windows_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "c", "windows_selftest.cpp"), "-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_predicate_and_layout_against_byte_map_models(tmp_path, flags):
    out = _selftest(tmp_path, flags)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")
