"""CPU: the public Python surface of lzma_amd against the fixture recorded before the container classes were put on
common base classes (tests/golden/api_surface.json, made by tests/api_surface.py): the public names, and the
inspect.signature string and the docstring of every public function, class and method.  The surface is taken in a fresh
interpreter that imports the package alone, so that neither the names nor "importing lzma_amd does not import torch"
depend on what the test session has loaded."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_public_surface_is_the_recorded_one():
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "api_surface.py")], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert run.returncode == 0, run.stderr  # (the program itself fails where the import pulled torch in)
    got = json.loads(run.stdout)
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "api_surface.json")))
    assert sorted(got) == sorted(want)
    for name in want:
        if want[name]["kind"] == "class":
            assert sorted(got[name]["members"]) == sorted(want[name]["members"]), name
            for m in want[name]["members"]:
                assert got[name]["members"][m] == want[name]["members"][m], "%s.%s" % (name, m)
        assert got[name] == want[name], name
    for cls in ("XzFile", "SevenZipFile", "ZipFile", "Context"):
        assert want[cls]["kind"] == "class" and want[cls]["members"]["close"]["kind"] == "function"
    assert want["ZipFile"]["members"]["extract"]["doc"] != want["SevenZipFile"]["members"]["extract"]["doc"]
