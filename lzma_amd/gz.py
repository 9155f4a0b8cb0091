"""gzip files, BGZF files and zlib streams as one batch, and Adler-32 of device ranges (include/xlz.h: xlz_gz_* and
xlz_adler32_*).  Use as `from lzma_amd import gz`: the package does not import this module.

Every deflate stream is inflated by ONE wave, and a lone wave is slower than a host core.  What this makes fast is BGZF
files (bgzip, BAM, tabix: every block of at most 64 KiB is a member of its own, known in advance) and batches of many
files or streams.  One ordinary single-member .gz of a large file is the host's job and stays so.

A file's outcome is a status of its own, never an exception: (status, out_len, in_consumed, members)."""
import ctypes

from . import _native as N
from . import LzmaError, OK, ERR_OUT_CAP, _ManyFiles, _PyBuffer, _cbuf, _tensor_out

AUTO, GZIP, ZLIB = N.GZ_AUTO, N.GZ_GZIP, N.GZ_ZLIB
F_BGZF, F_NAME, F_COMMENT, F_HCRC = N.GZ_F_BGZF, N.GZ_F_NAME, N.GZ_F_COMMENT, N.GZ_F_HCRC


def _formats(n, format):
    fmts = [int(format)] * n if isinstance(format, int) else [int(x) for x in format]
    if len(fmts) != n:
        raise ValueError("one format per file")
    return fmts


class _GzFiles(_ManyFiles):
    """an xlz_gz_file array over `datas` (bytes or contiguous buffers), every one borrowed through the buffer protocol --
    never copied -- and held until release()"""

    def __init__(self, datas, windows, format):
        self.n = len(datas)
        if len(windows) != self.n:
            raise ValueError("one window per file")
        fmts = _formats(self.n, format)
        self.arr = (N.GzFile * max(self.n, 1))()
        self.res = (N.GzResult * max(self.n, 1))()
        self._views = (_PyBuffer * max(self.n, 1))()
        self._held = 0
        try:
            for i, d in enumerate(datas):
                ctypes.pythonapi.PyObject_GetBuffer(ctypes.py_object(d), ctypes.byref(self._views[i]), 0)  # (raises: no buffer, not contiguous)
                self._held = i + 1
                self.arr[i].inp, self.arr[i].in_len = self._views[i].buf, self._views[i].len
                self.arr[i].dst_off, self.arr[i].dst_cap, self.arr[i].format = int(windows[i][0]), int(windows[i][1]), fmts[i]
        except Exception:
            self.release()
            raise

    def decode(self, name, ctx, dst, cap, verify):
        st = getattr(N.lib(), name)(ctx._h, self.arr, self.n, dst, int(cap), 1 if verify else 0, self.res)
        if st != OK:
            raise LzmaError(st, name)
        return [(r.status, r.out_len, r.in_consumed, r.members) for r in self.res[: self.n]]


def probe(data, format=AUTO):
    """xlz_gz_probe: what the headers say, nothing inflated -> a dict: format (GZIP / ZLIB), flags (F_*), bgzf, members
    (BGZF: blocks; otherwise 0 = not known), size_hint (BGZF: the sum of the blocks' sizes; gzip: the last four bytes, what
    gzip -l prints; zlib: 0), mtime, name (bytes or None).  Raises LzmaError with the header's status.  Host only."""
    data = bytes(data)
    buf, p = _cbuf(data)
    info = N.GzInfo()
    st = N.lib().xlz_gz_probe(p, len(data), int(format), ctypes.byref(info))
    if st != OK:
        raise LzmaError(st, "xlz_gz_probe")
    return {"format": info.format, "flags": info.flags, "bgzf": bool(info.flags & F_BGZF), "members": info.members, "size_hint": info.size_hint,
            "mtime": info.mtime, "name": data[info.name_off:info.name_off + info.name_len] if info.flags & F_NAME else None}


def layout(datas, caps=None, align=1, format=AUTO):
    """windows for `datas` back to back, each offset a multiple of `align` -> ([(dst_off, dst_cap)], total).  A window's
    size is caps[i] where that is given and not None, else the file's size hint -- exact for BGZF and for a gzip file of ONE
    member below 4 GiB; a zlib stream has no hint and NEEDS a cap (ValueError).  A file whose header is refused gets an
    empty window: decoding reports its status.  Host only."""
    fmts = _formats(len(datas), format)
    if align < 1:
        raise ValueError("align must be at least 1")
    windows, at = [], 0
    for i, d in enumerate(datas):
        cap = caps[i] if caps is not None else None
        if cap is None:
            try:
                info = probe(d, fmts[i])
            except LzmaError:
                info = {"format": GZIP, "size_hint": 0}
            if info["format"] == ZLIB:
                raise ValueError("file %d is a zlib stream: it announces no size, give a cap" % i)
            cap = info["size_hint"]
        at = (at + align - 1) // align * align
        windows.append((at, int(cap)))
        at += int(cap)
    return windows, at


def decode_host(data, out_cap=None, format=AUTO, verify=True):
    """xlz_gz_decode_host, the serial twin: one file on the host -> (bytes or None, status, in_consumed, members).
    out_cap: the room (None: the size hint).  No device needed."""
    data = bytes(data)
    if out_cap is None:
        out_cap = layout([data], format=format)[1]
    buf, p = _cbuf(data)
    out = ctypes.create_string_buffer(max(int(out_cap), 1))
    r = N.GzResult()
    st = N.lib().xlz_gz_decode_host(p, len(data), int(format), ctypes.cast(out, ctypes.c_void_p), int(out_cap), 1 if verify else 0, ctypes.byref(r))
    if st != OK:
        raise LzmaError(st, "xlz_gz_decode_host")
    return (out.raw[: r.out_len] if r.status == OK else None), r.status, r.in_consumed, r.members


def decode_many(ctx, datas, caps=None, format=AUTO, verify=True, max_size=None):
    """xlz_gz_decode_many: many files as ONE batch into one host buffer laid out by layout() -> a list of (bytes or None,
    status, in_consumed, members), one per file.  max_size: refuse (ERR_OUT_CAP) a set whose windows take more in all."""
    windows, total = layout(datas, caps, 1, format)
    if max_size is not None and total > max_size:
        raise LzmaError(ERR_OUT_CAP, "xlz_gz_decode_many: the windows take %d bytes, max_size is %d" % (total, max_size))
    out = ctypes.create_string_buffer(max(total, 1))
    with _GzFiles(datas, windows, format) as m:
        res = m.decode("xlz_gz_decode_many", ctx, ctypes.cast(out, ctypes.c_void_p), total, verify)
    base = ctypes.addressof(out)
    return [(ctypes.string_at(base + windows[i][0], n) if st == OK else None, st, used, mem) for i, (st, n, used, mem) in enumerate(res)]


def decode_many_into(ctx, datas, out, windows, format=AUTO, verify=True):
    """xlz_gz_decode_many with the caller's buffer: file i goes to its window (dst_off, dst_cap) = windows[i] of `out` (a
    writable buffer); windows must not overlap -> [(status, out_len, in_consumed, members)]"""
    dst = out if isinstance(out, ctypes.Array) else (ctypes.c_char * memoryview(out).nbytes).from_buffer(out)
    with _GzFiles(datas, windows, format) as m:
        return m.decode("xlz_gz_decode_many", ctx, ctypes.cast(dst, ctypes.c_void_p), ctypes.sizeof(dst), verify)


def decode_many_device(ctx, datas, dptr, cap, windows, format=AUTO, verify=True):
    """xlz_gz_decode_many_device: the same into `cap` bytes of device memory at the address `dptr` (on the context's
    device): the rounds of inflate launches and the checks run there, only digests come back
    -> [(status, out_len, in_consumed, members)]"""
    with _GzFiles(datas, windows, format) as m:
        return m.decode("xlz_gz_decode_many_device", ctx, ctypes.c_void_p(int(dptr)), cap, verify)


def decode_many_tensor(ctx, datas, caps=None, format=AUTO, verify=True, align=1, out=None):
    """decode_many_device into a torch.uint8 tensor on the context's device: `out` (one-dimensional, contiguous, at least
    the layout's total; ERR_OUT_CAP if smaller) or a new one -> (tensor, [view or None], [(status, out_len, in_consumed,
    members)]): view i is tensor[off:off + out_len] where file i's status is OK"""
    windows, total = layout(datas, caps, align, format)
    out = _tensor_out(ctx, total, out, "the windows take")
    with _GzFiles(datas, windows, format) as m:
        res = m.decode("xlz_gz_decode_many_device", ctx, ctypes.c_void_p(out.data_ptr()), out.numel(), verify)
    return out, [out[windows[i][0]:windows[i][0] + r[1]] if r[0] == OK else None for i, r in enumerate(res)], res


def decompress(ctx, data, out_cap=None, format=AUTO, verify=True):
    """one file through decode_many -> bytes; raises LzmaError with the file's status.  (One ordinary .gz is one wave, or the
    host's threads above the launch-length cap: the batch calls are what the device is for.)"""
    out, st, _, _ = decode_many(ctx, [data], None if out_cap is None else [out_cap], format, verify)[0]
    if st != OK:
        raise LzmaError(st, "gz.decompress")
    return out


def adler32_device(ctx, dptr, buf_len, ranges):
    """xlz_adler32_device: Adler-32 of ranges [(off, len), ...] of `buf_len` bytes of device memory at `dptr` -> [digest];
    ranges may overlap, in any order; an empty one is 1"""
    ranges = list(ranges)
    n = len(ranges)
    arr = (N.AdlerRange * max(n, 1))()
    for i, (off, ln) in enumerate(ranges):
        arr[i].off, arr[i].len = int(off), int(ln)
    dig = (ctypes.c_uint32 * max(n, 1))()
    st = N.lib().xlz_adler32_device(ctx._h, ctypes.c_void_p(int(dptr)), int(buf_len), arr, n, dig)
    if st != OK:
        raise LzmaError(st, "xlz_adler32_device")
    return list(dig[:n])


def adler32_host(data, adler=1):
    """xlz_adler32_host: the digest of `adler`'s bytes followed by data.  Host only."""
    buf, p = _cbuf(data)
    return N.lib().xlz_adler32_host(int(adler), p, len(data))


def adler32_combine(a, b, len_b):
    """xlz_adler32_combine: adler32(A + B) from a = adler32(A), b = adler32(B) and len_b = len(B).  Host only."""
    return N.lib().xlz_adler32_combine(int(a), int(b), int(len_b))


def last_stats(ctx):
    """xlz_ctx_last_gz_stats: of the most recent decode_many* on ctx that ran -> a dict"""
    s = N.GzStats()
    st = N.lib().xlz_ctx_last_gz_stats(ctx._h, ctypes.byref(s))
    if st != OK:
        raise LzmaError(st, "xlz_ctx_last_gz_stats")
    return {name: getattr(s, name) for name, _ in N.GzStats._fields_}
