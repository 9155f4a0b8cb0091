"""The recipe of tests/golden/infozip.zip: a few KiB written once by Info-ZIP's `zip` 3.0 with -fz (force ZIP64 extra
fields) and -fd (force data descriptors): the stored entries in a first run (-0), the deflate entries added in a second
one (-9 -fz; zip cannot update an archive it wrote with -fz itself, so the first run goes without).  The second run
rewrites every entry with ZIP64 extra fields, and leaves an all-ones directory offset in the end record WITHOUT a ZIP64
end record, so Python's zipfile refuses the archive; the parser takes the directory where it finds it.  An independent
writer for the .zip parser.  The tests read the committed bytes; this script needs the `zip` program and is
run by hand:  python tests/golden/make_infozip_zip.py"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import zip_files as Z  # noqa: E402

STORED = {"stored_1.bin": Z.noise(900, 1), "stored_17.bin": Z.noise(901, 17), "sub/stored_1000.bin": Z.noise(902, 1000),
          "stored_empty.bin": b""}
DEFLATED = {"deflated_3000.txt": Z.text(903, 3000), "sub/deflated_257.txt": Z.text(904, 257)}


def main():
    out = os.path.join(HERE, "infozip.zip")
    with tempfile.TemporaryDirectory() as d:
        os.mkdir(os.path.join(d, "sub"))
        for name, data in {**STORED, **DEFLATED}.items():
            with open(os.path.join(d, name), "wb") as f:
                f.write(data)
            os.utime(os.path.join(d, name), (1709213862, 1709213862))
        os.utime(os.path.join(d, "sub"), (1709213862, 1709213862))
        tmp = os.path.join(d, "out.zip")
        env = dict(os.environ, TZ="UTC")
        subprocess.check_call(["zip", "-X", "-fd", "-0", tmp, "sub/"] + sorted(STORED), cwd=d, env=env)
        subprocess.check_call(["zip", "-X", "-fz", "-fd", "-9", tmp] + sorted(DEFLATED), cwd=d, env=env)
        with open(tmp, "rb") as f:
            data = f.read()
    with open(out, "wb") as f:
        f.write(data)
    print(out, len(data))


if __name__ == "__main__":
    main()
