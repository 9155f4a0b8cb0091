""".bz2 files as one batch (include/xlz.h: xlz_bz2_*).  Use as `from lzma_amd import bzip2`: the
package does not import this module.

A .bz2 file is a chain of independent blocks of at most 900 000 bytes, each found by its 48-bit magic at any bit offset, so
ONE large file is a batch of blocks, as many files are.  Every block is decoded by one wave, and a lone wave is much
slower than a host core: files of many blocks and batches of many files are what the device is for; a call of fewer than
some 300 blocks in all is the host's job (set_mode(ctx, HOST_THREADS), decode_host, or Python's bz2; profiles/device_bz2.txt).

A file's outcome is a status of its own, never an exception: (status, out_len, in_consumed, blocks, streams).  A .bz2 file
does not state its decoded size: a window that is too small gives ERR_OUT_CAP with out_len = the true size, and the
caller retries once with exact room (decompress does).  OK with in_consumed < len(data) means that, behind at least one
complete stream, a damaged stream was ignored together with everything behind it, as Python's bz2.decompress does."""
import ctypes

from . import _native as N
from . import LzmaError, OK, ERR_OUT_CAP, _ManyFiles, _PyBuffer, _cbuf, _tensor_out

DEVICE, HOST_THREADS = 1, 2  # set_mode


class _Bz2Files(_ManyFiles):
    """an xlz_bz2_file array over `datas` (bytes or contiguous buffers), every one borrowed through the buffer protocol --
    never copied -- and held until release()"""

    def __init__(self, datas, windows):
        self.n = len(datas)
        if len(windows) != self.n:
            raise ValueError("one window per file")
        self.arr = (N.Bz2File * max(self.n, 1))()
        self.res = (N.Bz2Result * max(self.n, 1))()
        self._views = (_PyBuffer * max(self.n, 1))()
        self._held = 0
        try:
            for i, d in enumerate(datas):
                ctypes.pythonapi.PyObject_GetBuffer(ctypes.py_object(d), ctypes.byref(self._views[i]), 0)  # (raises: no buffer, not contiguous)
                self._held = i + 1
                self.arr[i].inp, self.arr[i].in_len = self._views[i].buf, self._views[i].len
                self.arr[i].dst_off, self.arr[i].dst_cap = int(windows[i][0]), int(windows[i][1])
        except Exception:
            self.release()
            raise

    def decode(self, name, ctx, dst, cap, verify):
        st = getattr(N.lib(), name)(ctx._h, self.arr, self.n, dst, int(cap), 1 if verify else 0, self.res)
        if st != OK:
            raise LzmaError(st, name)
        return [(r.status, r.out_len, r.in_consumed, r.blocks, r.streams) for r in self.res[: self.n]]


def probe(data):
    """xlz_bz2_probe: the first header and the scan for the two magics, nothing decoded -> a dict: level, candidates (block
    magics at any bit offset: an upper bound of the blocks), streams (end magics), size_hint (candidates x level x 100 000:
    the decoded size at most, unless the encoder folded runs), size_bound (what the file can decode to at all).  Raises
    LzmaError with the header's status.  Host only."""
    data = bytes(data)
    buf, p = _cbuf(data)
    info = N.Bz2Info()
    st = N.lib().xlz_bz2_probe(p, len(data), ctypes.byref(info))
    if st != OK:
        raise LzmaError(st, "xlz_bz2_probe")
    return {"level": info.level, "candidates": info.candidates, "streams": info.streams, "size_hint": info.size_hint, "size_bound": info.size_bound}


def layout(datas, caps=None, align=1):
    """windows for `datas` back to back, each offset a multiple of `align` -> ([(dst_off, dst_cap)], total).  A window's
    size is caps[i] where that is given and not None, else the probe's size_hint (a file whose header is refused gets an
    empty window: decoding reports its status).  Host only."""
    if align < 1:
        raise ValueError("align must be at least 1")
    windows, at = [], 0
    for i, d in enumerate(datas):
        cap = caps[i] if caps is not None else None
        if cap is None:
            try:
                cap = probe(d)["size_hint"]
            except LzmaError:
                cap = 0
        at = (at + align - 1) // align * align
        windows.append((at, int(cap)))
        at += int(cap)
    return windows, at


def decode_host(data, out_cap=None, verify=True):
    """xlz_bz2_decode_host, the serial twin: one file on the host -> (bytes or None, status, out_len, in_consumed, blocks,
    streams).  out_cap: the room (None: the size hint).  No device needed."""
    data = bytes(data)
    if out_cap is None:
        out_cap = layout([data])[1]
    buf, p = _cbuf(data)
    out = ctypes.create_string_buffer(max(int(out_cap), 1))
    r = N.Bz2Result()
    st = N.lib().xlz_bz2_decode_host(p, len(data), ctypes.cast(out, ctypes.c_void_p), int(out_cap), 1 if verify else 0, ctypes.byref(r))
    if st != OK:
        raise LzmaError(st, "xlz_bz2_decode_host")
    return (out.raw[: r.out_len] if r.status == OK else None), r.status, r.out_len, r.in_consumed, r.blocks, r.streams


def decode_many(ctx, datas, caps=None, verify=True, max_size=None):
    """xlz_bz2_decode_many: many files as ONE batch into one host buffer laid out by layout() -> a list of (bytes or None,
    status, out_len, in_consumed, blocks, streams), one per file.  max_size: refuse (ERR_OUT_CAP) a set whose windows
    take more in all."""
    windows, total = layout(datas, caps, 1)
    if max_size is not None and total > max_size:
        raise LzmaError(ERR_OUT_CAP, "xlz_bz2_decode_many: the windows take %d bytes, max_size is %d" % (total, max_size))
    out = ctypes.create_string_buffer(max(total, 1))
    with _Bz2Files(datas, windows) as m:
        res = m.decode("xlz_bz2_decode_many", ctx, ctypes.cast(out, ctypes.c_void_p), total, verify)
    base = ctypes.addressof(out)
    return [(ctypes.string_at(base + windows[i][0], r[1]) if r[0] == OK else None,) + r for i, r in enumerate(res)]


def decode_many_into(ctx, datas, out, windows, verify=True):
    """xlz_bz2_decode_many with the caller's buffer: file i goes to its window (dst_off, dst_cap) = windows[i] of `out` (a
    writable buffer); windows must not overlap -> [(status, out_len, in_consumed, blocks, streams)]"""
    dst = out if isinstance(out, ctypes.Array) else (ctypes.c_char * memoryview(out).nbytes).from_buffer(out)
    with _Bz2Files(datas, windows) as m:
        return m.decode("xlz_bz2_decode_many", ctx, ctypes.cast(dst, ctypes.c_void_p), ctypes.sizeof(dst), verify)


def decode_many_device(ctx, datas, dptr, cap, windows, verify=True):
    """xlz_bz2_decode_many_device: the same into `cap` bytes of device memory at the address `dptr` (on the context's
    device): only statuses, lengths and digests come back -> [(status, out_len, in_consumed, blocks, streams)]"""
    with _Bz2Files(datas, windows) as m:
        return m.decode("xlz_bz2_decode_many_device", ctx, ctypes.c_void_p(int(dptr)), cap, verify)


def decode_many_tensor(ctx, datas, caps=None, verify=True, align=1, out=None):
    """decode_many_device into a torch.uint8 tensor on the context's device: `out` (one-dimensional, contiguous, at least
    the layout's total; ERR_OUT_CAP if smaller) or a new one -> (tensor, [view or None], [(status, out_len, in_consumed,
    blocks, streams)]): view i is tensor[off:off + out_len] where file i's status is OK"""
    windows, total = layout(datas, caps, align)
    out = _tensor_out(ctx, total, out, "the windows take")
    with _Bz2Files(datas, windows) as m:
        res = m.decode("xlz_bz2_decode_many_device", ctx, ctypes.c_void_p(out.data_ptr()), out.numel(), verify)
    return out, [out[windows[i][0]:windows[i][0] + r[1]] if r[0] == OK else None for i, r in enumerate(res)], res


def decompress(ctx, data, out_cap=None, verify=True):
    """one file through decode_many -> bytes, retrying ONCE on ERR_OUT_CAP with the size that the first call reported;
    raises LzmaError with the file's status"""
    r = decode_many(ctx, [data], None if out_cap is None else [out_cap], verify)[0]
    if r[1] == ERR_OUT_CAP:
        r = decode_many(ctx, [data], [r[2]], verify)[0]
    if r[1] != OK:
        raise LzmaError(r[1], "bzip2.decompress")
    return r[0]


def crc32_bzip2(data, crc=0):
    """xlz_crc32_bzip2_host: CRC-32/BZIP2 (polynomial 0x04C11DB7, not reflected) of `crc`'s bytes followed by data.  Host only."""
    buf, p = _cbuf(data)
    return N.lib().xlz_crc32_bzip2_host(int(crc), p, len(data))


def set_mode(ctx, mode):
    """xlz_ctx_set_bz2_mode: DEVICE (1, the default) or HOST_THREADS (2: every block on host threads, uploaded)"""
    st = N.lib().xlz_ctx_set_bz2_mode(ctx._h, int(mode))
    if st != OK:
        raise LzmaError(st, "xlz_ctx_set_bz2_mode")


def set_scratch(ctx, nbytes):
    """xlz_ctx_set_bz2_scratch: the scratch one round of block candidates may take (0: the default, 6 GiB)"""
    st = N.lib().xlz_ctx_set_bz2_scratch(ctx._h, int(nbytes))
    if st != OK:
        raise LzmaError(st, "xlz_ctx_set_bz2_scratch")


def last_stats(ctx):
    """xlz_ctx_last_bz2_stats: of the most recent decode_many* on ctx that ran -> a dict"""
    s = N.Bz2Stats()
    st = N.lib().xlz_ctx_last_bz2_stats(ctx._h, ctypes.byref(s))
    if st != OK:
        raise LzmaError(st, "xlz_ctx_last_bz2_stats")
    return {name: getattr(s, name) for name, _ in N.Bz2Stats._fields_}
