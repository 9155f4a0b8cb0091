"""Generates tests/golden/libarchive_gnutar.tar and libarchive_pax.tar: archives written by an INDEPENDENT writer --
libarchive's tar writers, through `cmake -E tar cf x.tar --format=gnutar|pax` -- of a small tree with a file, an empty
file, a symbolic link and a file whose path is longer than a ustar header holds (208 bytes, one of them not ASCII), so
that the gnutar archive carries an 'L' entry and the pax one an 'x' entry.  The tests compare the library's table with
tarfile's over these bytes; nothing else is recorded.
    python tests/golden/make_libarchive_tar.py"""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))


def write_archive(fmt):
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "tree", "sub" * 40))
        with open(os.path.join(d, "tree", "a.txt"), "wb") as f:
            f.write(b"alpha" * 300)
        with open(os.path.join(d, "tree", "sub" * 40, "n" * 80 + "é.bin"), "wb") as f:
            f.write(bytes(range(256)) * 9)
        open(os.path.join(d, "tree", "empty"), "wb").close()
        os.symlink("a.txt", os.path.join(d, "tree", "link"))
        out = os.path.join(d, "x.tar")
        subprocess.check_call(["cmake", "-E", "tar", "cf", out, "--format=" + fmt, "tree"], cwd=d)
        with open(out, "rb") as f:
            return f.read()


def main():
    for fmt in ("gnutar", "pax"):
        data = write_archive(fmt)
        with open(os.path.join(HERE, "libarchive_%s.tar" % fmt), "wb") as f:
            f.write(data)
        print("wrote libarchive_%s.tar (%d bytes)" % (fmt, len(data)))


if __name__ == "__main__":
    main()
