"""lzma_amd -- MI355X-native batched LZMA / LZMA2 decoder.

Host-side mirror of the reference's Go surface (kulaginds/lzma: NewReader1,
NewReader2, the bodgit/sevenzip decompressor constructors and the exported
Decode* helpers) on top of the C ABI in include/xlz.h.  All decoding happens in
hand-written HIP kernels (lzma_amd/csrc); this package only marshals buffers.
It fails loudly when libxlz.so or a GPU is missing -- there is no CPU fallback.
"""
import collections
import ctypes

from . import _native as N
from ._native import (EOF, ERR_BAD_ARG, ERR_CLOSED, ERR_DEVICE, ERR_HEADER_EOF,  # noqa: F401
                      ERR_INSUFFICIENT_PROPS, ERR_NEED_ONE_READER, ERR_OUT_CAP, ERR_PROPS,
                      ERR_RC_INIT, ERR_RESULT, ERR_UNEXPECTED_EOF, ERR_UNSUPPORTED,
                      FMT_LZMA2_RAW, FMT_LZMA_ALONE, FMT_LZMA_RAW, NEED_INPUT, OK, OK_INPUT_EOF, UNKNOWN_SIZE,
                      CHECK_CRC32, CHECK_CRC64, CHECK_NONE, CHECK_SHA256)

# the .xz filter ids (include/xlz.h: XLZ_FILTER_*)
FILTER_DELTA, FILTER_X86, FILTER_POWERPC, FILTER_IA64, FILTER_ARM, FILTER_ARMTHUMB, FILTER_SPARC = 3, 4, 5, 6, 7, 8, 9
ZIP_ENTRY_DEFLATE = N.ZIP_ENTRY_DEFLATE  # xlz_zip_entry.flags: a method-8 entry that deflate mode 1 / 2 inflates


class LzmaError(Exception):
    """A reference error value (errors.go:5-12 and friends) carried as a status code."""

    def __init__(self, status, where=""):
        self.status = status
        msg = N.strerror(status)
        super().__init__("%s%s" % (where + ": " if where else "", msg))


# the reference's sentinels, as statuses
ErrResultError = ERR_RESULT                  # errors.go:8
ErrIncorrectProperties = ERR_PROPS           # errors.go:7
ErrUnexpectedEOF = ERR_UNEXPECTED_EOF        # io.ErrUnexpectedEOF (reader2.go:104-127)


class Stream:
    """One compressed stream of a batch (xlz_stream_desc)."""

    def __init__(self, data, fmt=FMT_LZMA_ALONE, out_cap=None, dict_size=0, unpack_size=UNKNOWN_SIZE,
                 props=0):
        self.data = bytes(data)
        self.fmt = fmt
        self.dict_size = dict_size
        self.unpack_size = unpack_size
        self.props = props
        if out_cap is None:
            out_cap = self._guess_cap()
        self.out_cap = out_cap

    def _guess_cap(self):
        if self.fmt == FMT_LZMA_ALONE and len(self.data) >= 13:
            u = int.from_bytes(self.data[5:13], "little")
            if u != UNKNOWN_SIZE:
                return u
        if self.fmt == FMT_LZMA_RAW and self.unpack_size != UNKNOWN_SIZE:
            return self.unpack_size
        raise ValueError("out_cap is required when the stream does not carry its size")


class Context:
    """One HIP device + stream (xlz_ctx).  One per host thread and GPU."""

    def __init__(self, device=0):
        self._h = ctypes.c_void_p()
        self.last_xz_unverified = 0
        st = N.lib().xlz_ctx_create(device, ctypes.byref(self._h))
        if st != OK:
            raise LzmaError(st, "xlz_ctx_create(device=%d)" % device)

    def enable_batching(self, window_us=500, max_streams=4096):
        """Readers created on this context from now on are decoded together (xlz_ctx_enable_batching)."""
        st = N.lib().xlz_ctx_enable_batching(self._h, window_us, max_streams)
        if st != OK:
            raise LzmaError(st, "xlz_ctx_enable_batching")

    def batching_stats(self):
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        st = N.lib().xlz_ctx_batching_stats(self._h, ctypes.byref(a), ctypes.byref(b))
        if st != OK:
            raise LzmaError(st, "xlz_ctx_batching_stats")
        return a.value, b.value

    def _stats(self, struct, name):
        """the context's `struct` as the library call `name` fills it in -> dict of its fields (but `reserved`)"""
        s = struct()
        st = getattr(N.lib(), name)(self._h, ctypes.byref(s))
        if st != OK:
            raise LzmaError(st, name)
        return {k: getattr(s, k) for k, _ in struct._fields_ if k != "reserved"}

    def last_call_stats(self):
        """phase times and slot occupancy of the last decode_batch on this context (xlz_ctx_last_call_stats) -> dict"""
        return self._stats(N.CallStats, "xlz_ctx_last_call_stats")

    def set_slicing(self, min_call_bytes=0, slice_bytes=0, max_slices=0):
        """when a decode_batch of one wave round runs as a sequence of launches whose downloads overlap the decode
        (xlz_ctx_set_slicing; 0 = default, max_slices=1: never)"""
        st = N.lib().xlz_ctx_set_slicing(self._h, min_call_bytes, slice_bytes, max_slices)
        if st != OK:
            raise LzmaError(st, "xlz_ctx_set_slicing")

    def trim(self):
        """release the device / pinned memory decode_batch keeps between calls (xlz_ctx_trim) -> bytes released"""
        n = ctypes.c_uint64()
        st = N.lib().xlz_ctx_trim(self._h, ctypes.byref(n))
        if st != OK:
            raise LzmaError(st, "xlz_ctx_trim")
        return n.value

    def set_check_mode(self, mode):
        """where xz_decode / sevenzip_decode verify (xlz_ctx_set_check_mode): 0 on host threads behind the download
        (default); 1 CRC32 / CRC64 on the device next to the decode; 2 as 1, and the SHA-256 blocks of an .xz file on the
        device too, where sha256_plan gives them to it"""
        st = N.lib().xlz_ctx_set_check_mode(self._h, int(mode))
        if st != OK:
            raise LzmaError(st, "xlz_ctx_set_check_mode")

    def check_mode(self):
        return N.lib().xlz_ctx_check_mode(self._h)

    def last_check_stats(self):
        """who checked what in the last Batch.checks / decode_batch_checked / front-end call in check mode 1 on this
        context (xlz_ctx_last_check_stats) -> dict"""
        return self._stats(N.CheckStats, "xlz_ctx_last_check_stats")

    def last_sha256_stats(self):
        """who hashed the SHA-256 ranges of the last Batch.digests / decode_batch_digests / xz_decode in check mode 2 on this
        context, and the threshold the plan chose (xlz_ctx_last_sha256_stats) -> dict"""
        return self._stats(N.Sha256Stats, "xlz_ctx_last_sha256_stats")

    def set_filter_mode(self, mode):
        """what xz_decode / sevenzip_decode do with Delta / BCJ filter chains (xlz_ctx_set_filter_mode): 0 refuse them
        (default), 1 decode them and undo the filters on the device"""
        st = N.lib().xlz_ctx_set_filter_mode(self._h, int(mode))
        if st != OK:
            raise LzmaError(st, "xlz_ctx_set_filter_mode")

    def filter_mode(self):
        L = N.lib()
        if not hasattr(L, "xlz_ctx_filter_mode"):  # (an older library loaded through XLZ_SO: it refuses every chain)
            return 0
        return L.xlz_ctx_filter_mode(self._h)

    def last_filter_stats(self):
        """what ran where in the last Batch.filter / decode_batch_filtered / front-end call in filter mode 1 on this context
        (xlz_ctx_last_filter_stats) -> dict"""
        return self._stats(N.FilterStats, "xlz_ctx_last_filter_stats")

    def last_pack_stats(self):
        """what the pack kernel copied in the last Batch.pack / xz_decode_device / sevenzip_decode_device on this context
        (xlz_ctx_last_pack_stats) -> dict"""
        return self._stats(N.PackStats, "xlz_ctx_last_pack_stats")

    def last_xz_read_stats(self):
        """what the last XzFile.read / read_ranges / read_device / read_tensor on this context decoded and copied
        (xlz_ctx_last_xz_read_stats) -> dict: blocks, comp_bytes and decoded_bytes are those of the covering blocks.  Such a
        read also leaves its *unverified -- covering blocks with a reserved check type -- in self.last_xz_unverified."""
        return self._stats(N.XzReadStats, "xlz_ctx_last_xz_read_stats")

    def last_xz_many_stats(self):
        """what the last xz_decode_many / xz_decode_many_into / xz_decode_many_device / xz_decode_many_tensor on this context
        was made of (xlz_ctx_last_xz_many_stats) -> dict: files and failed_files, the blocks and comp_bytes of the one batch,
        decoded_bytes = the sum over the good files"""
        return self._stats(N.XzManyStats, "xlz_ctx_last_xz_many_stats")

    def set_bcj2_mode(self, mode):
        """what sevenzip_decode / sevenzip_decode_device do with BCJ2 folders (xlz_ctx_set_bcj2_mode): 0 refuse them (default),
        1 decode them and merge their streams on the device, 2 the same with the merge on host threads"""
        st = N.lib().xlz_ctx_set_bcj2_mode(self._h, int(mode))
        if st != OK:
            raise LzmaError(st, "xlz_ctx_set_bcj2_mode")

    def set_deflate_mode(self, mode):
        """what ZipFile extractions do with deflate (method 8) entries (xlz_ctx_set_deflate_mode): 0 refuse them (default),
        1 inflate them on the device, 2 the same on host threads"""
        st = N.lib().xlz_ctx_set_deflate_mode(self._h, int(mode))
        if st != OK:
            raise LzmaError(st, "xlz_ctx_set_deflate_mode")

    def deflate_mode(self):
        L = N.lib()
        if not hasattr(L, "xlz_ctx_deflate_mode"):  # (an older library loaded through XLZ_SO: it refuses every deflate entry)
            return 0
        return L.xlz_ctx_deflate_mode(self._h)

    def last_inflate_stats(self):
        """what was inflated where in the last inflate_batch, or in the last ZipFile extraction in deflate mode 1 / 2 that had
        a deflate entry, on this context (xlz_ctx_last_inflate_stats) -> dict: device_items, device_bytes, host_items,
        host_bytes, failed_items, uploads, launches"""
        return self._stats(N.InflateStats, "xlz_ctx_last_inflate_stats")

    def last_7z_extract_stats(self):
        """of the most recent SevenZipFile extraction on this context that ran: entries, empty_entries, failed_entries,
        folders, comp_bytes, decoded_bytes (what the batch was asked to decode), folder_bytes (the covering folders' full
        sizes: the difference is what the cuts saved), copied_bytes"""
        return self._stats(N.SzExtractStats, "xlz_ctx_last_7z_extract_stats")

    def last_zip_extract_stats(self):
        """of the most recent ZipFile extraction on this context that ran: entries, empty_entries, failed_entries,
        lzma_entries (streams of the batch), stored_entries, comp_bytes, copied_bytes, stored_uploads (host-to-device
        transfers made for the stored entries: 1 however many there are, as long as they fit one staging block)"""
        return self._stats(N.ZipExtractStats, "xlz_ctx_last_zip_extract_stats")

    def last_tar_stats(self):
        """of the most recent tar_scan_device / TarXzFile.list on this context whose scan ran: blocks, zero_blocks,
        candidate_blocks (downloaded), header_blocks (reached by the walk), meta_bytes, downloaded_bytes, kernel_ms, launches"""
        return self._stats(N.TarStats, "xlz_ctx_last_tar_stats")

    def bcj2_mode(self):
        L = N.lib()
        if not hasattr(L, "xlz_ctx_bcj2_mode"):  # (an older library loaded through XLZ_SO: it refuses every BCJ2 folder)
            return 0
        return L.xlz_ctx_bcj2_mode(self._h)

    def last_bcj2_stats(self):
        """what merged where in the last Batch.bcj2 / sevenzip_decode / sevenzip_decode_device in bcj2 mode 1 / 2 on this
        context (xlz_ctx_last_bcj2_stats) -> dict"""
        return self._stats(N.Bcj2Stats, "xlz_ctx_last_bcj2_stats")

    def event_record(self, slot):
        st = N.lib().xlz_ctx_event_record(self._h, slot)
        if st != OK:
            raise LzmaError(st, "xlz_ctx_event_record")

    def event_elapsed_ms(self, a, b):
        ms = ctypes.c_float()
        st = N.lib().xlz_ctx_event_elapsed_ms(self._h, a, b, ctypes.byref(ms))
        if st != OK:
            raise LzmaError(st, "xlz_ctx_event_elapsed_ms")
        return ms.value

    def close(self):
        if self._h:
            N.lib().xlz_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _make_descs(streams, with_out=True):
    n = len(streams)
    descs = (N.StreamDesc * n)()
    keep_in, outs = [], []
    for i, s in enumerate(streams):
        ib = ctypes.create_string_buffer(s.data, len(s.data)) if len(s.data) else ctypes.create_string_buffer(1)
        keep_in.append(ib)
        descs[i].inp = ctypes.cast(ib, ctypes.c_void_p)
        descs[i].in_len = len(s.data)
        if with_out:
            ob = ctypes.create_string_buffer(max(int(s.out_cap), 1))
            outs.append(ob)
            descs[i].out = ctypes.cast(ob, ctypes.c_void_p)
        descs[i].out_cap = int(s.out_cap)
        descs[i].format = s.fmt
        descs[i].dict_size = s.dict_size & 0xFFFFFFFF
        descs[i].unpack_size = s.unpack_size
        descs[i].props = s.props
    return descs, keep_in, outs


def decode_batch(ctx, streams):
    """Decode independent streams on the GPU.

    Returns a list of (output bytes, status, in_consumed).  A bad stream never
    fails the batch; the call raises only if it could not run at all.
    """
    streams = list(streams)
    n = len(streams)
    if n == 0:
        return []
    descs, keep, outs = _make_descs(streams)
    res = (N.Result * n)()
    st = N.lib().xlz_decode_batch(ctx._h, descs, n, res)
    if st != OK:
        raise LzmaError(st, "xlz_decode_batch")
    del keep
    return [(outs[i].raw[: res[i].out_len], res[i].status, res[i].in_consumed) for i in range(n)]


def _make_ranges(ranges):
    """[(stream, off, len, kind), ...] -> (xlz_check_range array, digest array)"""
    n = len(ranges)
    arr = (N.CheckRange * max(n, 1))()
    for q, (stream, off, length, kind) in enumerate(ranges):
        arr[q].stream, arr[q].off, arr[q].len, arr[q].kind = int(stream), int(off), int(length), int(kind)
    return arr, (ctypes.c_uint64 * max(n, 1))()


def decode_batch_checked(ctx, streams, checks):
    """decode_batch plus the CRC32 / CRC64 of ranges of the outputs, computed on the GPU before the call's device memory is
    released (xlz_decode_batch_checked).  checks: [(stream index, off, len, CHECK_CRC32 | CHECK_CRC64), ...]; a range
    covers what the decoder produced of it.  -> (list of (output bytes, status, in_consumed), list of digests)"""
    streams, checks = list(streams), list(checks)
    n = len(streams)
    descs, keep, outs = _make_descs(streams)
    res = (N.Result * max(n, 1))()
    arr, dig = _make_ranges(checks)
    st = N.lib().xlz_decode_batch_checked(ctx._h, descs, n, res, arr, len(checks), dig)
    if st != OK:
        raise LzmaError(st, "xlz_decode_batch_checked")
    del keep
    return [(outs[i].raw[: res[i].out_len], res[i].status, res[i].in_consumed) for i in range(n)], list(dig[: len(checks)])


def _make_steps(steps):
    """[(stream, filter id, parameter), ...] -> xlz_filter_step array"""
    arr = (N.FilterStep * max(len(steps), 1))()
    for q, (stream, fid, param) in enumerate(steps):
        arr[q].stream, arr[q].id, arr[q].param = int(stream), int(fid), int(param)
    return arr


def filter_host(fid, param, data):
    """one filter step (decoder side) over `data` on the host -> bytes (xlz_filter_host; no device needed).  fid: FILTER_*;
    param: the Delta distance 1..256, or the BCJ start offset"""
    buf = ctypes.create_string_buffer(bytes(data), len(data)) if len(data) else ctypes.create_string_buffer(1)
    st = N.lib().xlz_filter_host(int(fid), int(param), ctypes.cast(buf, ctypes.c_void_p), len(data))
    if st != OK:
        raise LzmaError(st, "xlz_filter_host")
    return buf.raw[: len(data)]


def _cbuf(data):
    """bytes -> (a ctypes buffer that holds them, its address as c_void_p)"""
    buf = ctypes.create_string_buffer(bytes(data), len(data)) if len(data) else ctypes.create_string_buffer(1)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def bcj2_host(main, call, jump, rc, out_len):
    """the BCJ2 merge of a .7z folder's four streams on the host -> bytes (xlz_bcj2_host; no device needed).  Raises
    LzmaError(ERR_RESULT) when the streams do not fill out_len or one of call / jump / rc runs out"""
    bufs = [_cbuf(x) for x in (main, call, jump, rc)]
    out = ctypes.create_string_buffer(max(int(out_len), 1))
    args = []
    for (_, p), x in zip(bufs, (main, call, jump, rc)):
        args += [p, len(x)]
    st = N.lib().xlz_bcj2_host(*args, ctypes.cast(out, ctypes.c_void_p), int(out_len))
    if st != OK:
        raise LzmaError(st, "xlz_bcj2_host")
    return out.raw[: int(out_len)]


def inflate_host(data, out_cap):
    """a raw deflate stream (RFC 1951, no zlib or gzip wrapper) on the host -> (bytes, input bytes used) (xlz_inflate_host; no
    device needed).  Raises LzmaError: ERR_RESULT invalid data, ERR_UNEXPECTED_EOF the input ends first, ERR_OUT_CAP more
    than out_cap bytes"""
    buf, p = _cbuf(data)
    out = ctypes.create_string_buffer(max(int(out_cap), 1))
    produced, consumed = ctypes.c_size_t(), ctypes.c_size_t()
    st = N.lib().xlz_inflate_host(p, len(data), ctypes.cast(out, ctypes.c_void_p), int(out_cap), ctypes.byref(produced), ctypes.byref(consumed))
    if st != OK:
        raise LzmaError(st, "xlz_inflate_host")
    return out.raw[: produced.value], consumed.value


def inflate_batch(ctx, items, dptr, cap):
    """raw deflate streams into one device buffer, each by one wave (xlz_inflate_batch; in deflate mode 2 on host threads).
    items: [(stream bytes, dst_off, dst_cap), ...]; dptr / cap: device memory of the context's device
    -> [(status, produced, in_consumed), ...]"""
    items = list(items)
    n = len(items)
    arr = (N.InflateItem * max(n, 1))()
    keep = []
    for q, (data, dst_off, dst_cap) in enumerate(items):
        buf, p = _cbuf(data)
        keep.append(buf)
        arr[q].inp, arr[q].in_len, arr[q].dst_off, arr[q].dst_cap = p, len(data), int(dst_off), int(dst_cap)
    res = (N.InflateResult * max(n, 1))()
    st = N.lib().xlz_inflate_batch(ctx._h, arr, n, ctypes.c_void_p(int(dptr)), int(cap), res)
    if st != OK:
        raise LzmaError(st, "xlz_inflate_batch")
    return [(res[q].status, res[q].produced, res[q].in_consumed) for q in range(n)]


def decode_batch_filtered(ctx, streams, steps, checks=()):
    """decode_batch_checked with filter steps undone on the GPU between decode and check (xlz_decode_batch_filtered).
    steps: [(stream index, FILTER_*, parameter), ...], the steps of one stream applied in list order; digests are over the
    filtered bytes.  -> (list of (output bytes, status, in_consumed), list of digests)"""
    streams, steps, checks = list(streams), list(steps), list(checks)
    n = len(streams)
    descs, keep, outs = _make_descs(streams)
    res = (N.Result * max(n, 1))()
    arr, dig = _make_ranges(checks)
    st = N.lib().xlz_decode_batch_filtered(ctx._h, descs, n, res, _make_steps(steps), len(steps), arr, len(checks), dig)
    if st != OK:
        raise LzmaError(st, "xlz_decode_batch_filtered")
    del keep
    return [(outs[i].raw[: res[i].out_len], res[i].status, res[i].in_consumed) for i in range(n)], list(dig[: len(checks)])


def _digest_values(ranges, dig):
    """xlz_digest array -> an int per CRC range, 32 bytes per SHA-256 range"""
    return [bytes(dig[q].b) if ranges[q][3] == CHECK_SHA256 else int.from_bytes(bytes(dig[q].b[:8]), "little")
            for q in range(len(ranges))]


def decode_batch_digests(ctx, streams, ranges, steps=()):
    """decode_batch_filtered whose ranges may be CHECK_SHA256 too, kinds mixed (xlz_decode_batch_digests): a SHA-256 range
    is hashed on the GPU, one lane per range, or by host threads, as sha256_plan splits the call's ranges.
    -> (list of (output bytes, status, in_consumed), list of digests: int for a CRC, 32 bytes for a SHA-256)"""
    streams, steps, ranges = list(streams), list(steps), list(ranges)
    n = len(streams)
    descs, keep, outs = _make_descs(streams)
    res = (N.Result * max(n, 1))()
    arr, _ = _make_ranges(ranges)
    dig = (N.Digest * max(len(ranges), 1))()
    st = N.lib().xlz_decode_batch_digests(ctx._h, descs, n, res, _make_steps(steps), len(steps), arr, len(ranges), dig)
    if st != OK:
        raise LzmaError(st, "xlz_decode_batch_digests")
    del keep
    return [(outs[i].raw[: res[i].out_len], res[i].status, res[i].in_consumed) for i in range(n)], _digest_values(ranges, dig)


def sha256_plan(lens, host_threads=0, lane_rate=0, host_rate=0):
    """which ranges of these lengths the device should hash -> list of bool (xlz_sha256_plan; host only).  lane_rate /
    host_rate: bytes per second of one GPU lane / of one host thread, 0 for the built-in ones"""
    lens = list(lens)
    n = len(lens)
    arr = (ctypes.c_uint64 * max(n, 1))(*lens)
    on = (ctypes.c_uint8 * max(n, 1))()
    st = N.lib().xlz_sha256_plan(arr, n, int(host_threads), float(lane_rate), float(host_rate), on)
    if st != OK:
        raise LzmaError(st, "xlz_sha256_plan")
    return [bool(on[i]) for i in range(n)]


def crc32_combine(crc_a, crc_b, len_b):
    """CRC32 of A + B from the CRC32s of A and of B and len(B) (xlz_crc32_combine; host only)"""
    return N.lib().xlz_crc32_combine(crc_a, crc_b, len_b)


def crc64_combine(crc_a, crc_b, len_b):
    """CRC64 (the .xz one) of A + B from the CRC64s of A and of B and len(B) (xlz_crc64_combine; host only)"""
    return N.lib().xlz_crc64_combine(crc_a, crc_b, len_b)


def decode_batch_plan(out_caps):
    """xlz_decode_batch_plan (host only): how decode_batch would cut a call of streams with these output capacities into
    pieces -> (list of the pieces' first stream indices + [n], mode: 0 one piece, 1 overlapped pieces, 2 one-round pieces)"""
    n = len(out_caps)
    descs = (N.StreamDesc * max(n, 1))()
    for i, c in enumerate(out_caps):
        descs[i].out_cap = int(c)
    cuts = (ctypes.c_size_t * (n + 2))()
    k, mode = ctypes.c_size_t(), ctypes.c_int32()
    st = N.lib().xlz_decode_batch_plan(descs, n, cuts, n + 2, ctypes.byref(k), ctypes.byref(mode))
    if st != OK:
        raise LzmaError(st, "xlz_decode_batch_plan")
    return list(cuts[: k.value]), mode.value


def batch_advice(streams, host_threads=0, ctx=None):
    """xlz_batch_advice: what a decode of `streams` would launch and whether the host's cores are the faster decoder
    for it -- host only, nothing is uploaded.  -> dict (units, in_bytes, wave_slots, break_even_units, fill, prefer_cpu)"""
    streams = list(streams)
    descs, keep, _ = _make_descs(streams, with_out=False)
    adv = N.Advice()
    st = N.lib().xlz_batch_advice(ctx._h if ctx else None, descs, len(streams), host_threads, ctypes.byref(adv))
    if st != OK:
        raise LzmaError(st, "xlz_batch_advice")
    del keep
    return {f: getattr(adv, f) for f, _ in N.Advice._fields_ if f != "reserved"}


def multi_plan(n_ctx, streams):
    """xlz_decode_batch_multi_plan (host only): what decode_batch_on would hand to which of n_ctx contexts -> list of dicts
    (stream, in_off, in_len, out_off, out_len, context, whole, first, last), the items of a stream adjacent and in order"""
    streams = list(streams)
    descs, keep, _ = _make_descs(streams, with_out=False)
    n = ctypes.c_size_t()
    st = N.lib().xlz_decode_batch_multi_plan(n_ctx, descs, len(streams), None, 0, ctypes.byref(n))
    if st != OK:
        raise LzmaError(st, "xlz_decode_batch_multi_plan")
    items = (N.MultiItem * max(n.value, 1))()
    st = N.lib().xlz_decode_batch_multi_plan(n_ctx, descs, len(streams), items, n.value, ctypes.byref(n))
    if st != OK:
        raise LzmaError(st, "xlz_decode_batch_multi_plan")
    del keep
    return [dict(stream=it.stream, in_off=it.in_off, in_len=it.in_len, out_off=it.out_off, out_len=it.out_len, context=it.context,
                 whole=bool(it.flags & 1), first=bool(it.flags & 2), last=bool(it.flags & 4)) for it in items[: n.value]]


def decode_batch_on(ctxs, streams):
    """decode_batch over several contexts (one per GPU) through xlz_decode_batch_multi: sharded by
    stream inside the library, one host thread per context, results in input order."""
    streams = list(streams)
    n = len(streams)
    if n == 0:
        return []
    descs, keep, outs = _make_descs(streams)
    res = (N.Result * n)()
    hs = (ctypes.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    st = N.lib().xlz_decode_batch_multi(hs, len(ctxs), descs, n, res)
    if st != OK:
        raise LzmaError(st, "xlz_decode_batch_multi")
    del keep
    return [(outs[i].raw[: res[i].out_len], res[i].status, res[i].in_consumed) for i in range(n)]


class Batch:
    """Device-resident batch: upload once, run many times (xlz_batch)."""

    def __init__(self, ctx, streams):
        self.ctx = ctx
        self.streams = list(streams)
        self.n = len(self.streams)
        descs, keep, _ = _make_descs(self.streams, with_out=False)
        self._h = ctypes.c_void_p()
        st = N.lib().xlz_batch_create(ctx._h, descs, self.n, ctypes.byref(self._h))
        if st != OK:
            raise LzmaError(st, "xlz_batch_create")

    def run(self):
        st = N.lib().xlz_batch_run(self._h)
        if st != OK:
            raise LzmaError(st, "xlz_batch_run")

    def sync(self):
        st = N.lib().xlz_batch_sync(self._h)
        if st != OK:
            raise LzmaError(st, "xlz_batch_sync")

    def kernel_ms(self):
        ms = ctypes.c_float()
        st = N.lib().xlz_batch_last_kernel_ms(self._h, ctypes.byref(ms))
        if st != OK:
            raise LzmaError(st, "xlz_batch_last_kernel_ms")
        return ms.value

    def results(self):
        res = (N.Result * max(self.n, 1))()
        st = N.lib().xlz_batch_results(self._h, res)
        if st != OK:
            raise LzmaError(st, "xlz_batch_results")
        return [(res[i].out_len, res[i].status, res[i].in_consumed) for i in range(self.n)]

    def stats(self):
        a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        st = N.lib().xlz_batch_stats(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        if st != OK:
            raise LzmaError(st, "xlz_batch_stats")
        return a.value, b.value, c.value

    def launch_info(self):
        """(resident single-wave workgroups = wave slots, LDS bytes per workgroup) of the decode launch"""
        a, b = ctypes.c_uint32(), ctypes.c_uint32()
        st = N.lib().xlz_batch_launch_info(self._h, ctypes.byref(a), ctypes.byref(b))
        if st != OK:
            raise LzmaError(st, "xlz_batch_launch_info")
        return a.value, b.value

    def kernel_name(self):
        """the kernel of the batch's main launch (xlz_batch_kernel_name): the full or the compact (pb <= 2) model layout"""
        return N.lib().xlz_batch_kernel_name(self._h).decode()

    def unit_trace(self):
        """(t_start, t_end, in_len) numpy uint32 arrays, one entry per unit of the last run: ticks of
        the device's 100 MHz clock since the first unit started (xlz_batch_unit_trace)."""
        import numpy as np
        n = ctypes.c_size_t()
        st = N.lib().xlz_batch_unit_trace(self._h, None, None, None, 0, ctypes.byref(n))
        if st != OK:
            raise LzmaError(st, "xlz_batch_unit_trace")
        a, b, c = (np.zeros(max(n.value, 1), dtype=np.uint32) for _ in range(3))
        st = N.lib().xlz_batch_unit_trace(self._h, a.ctypes.data, b.ctypes.data, c.ctypes.data, n.value, ctypes.byref(n))
        if st != OK:
            raise LzmaError(st, "xlz_batch_unit_trace")
        return a[: n.value], b[: n.value], c[: n.value]

    def checks(self, ranges):
        """CRC32 / CRC64 of ranges of the decoded outputs, computed on the device; only the digests come back
        (xlz_batch_checks).  ranges: [(stream index, off, len, CHECK_CRC32 | CHECK_CRC64), ...] -> list of digests"""
        ranges = list(ranges)
        arr, dig = _make_ranges(ranges)
        st = N.lib().xlz_batch_checks(self._h, arr, len(ranges), dig)
        if st != OK:
            raise LzmaError(st, "xlz_batch_checks")
        return list(dig[: len(ranges)])

    def digests(self, ranges):
        """checks() whose ranges may be CHECK_SHA256 too, kinds mixed (xlz_batch_digests) -> list of digests: int for a CRC,
        32 bytes for a SHA-256.  The SHA-256 ranges sha256_plan leaves to the host are downloaded and hashed there."""
        ranges = list(ranges)
        arr, _ = _make_ranges(ranges)
        dig = (N.Digest * max(len(ranges), 1))()
        st = N.lib().xlz_batch_digests(self._h, arr, len(ranges), dig)
        if st != OK:
            raise LzmaError(st, "xlz_batch_digests")
        return _digest_values(ranges, dig)

    def _sha256_kernel(self, ranges):
        """measuring aid (tools/sha256_bench.py): every range through the SHA-256 kernel whatever sha256_plan says
        -> (list of 32-byte digests, kernel ms by HIP events)"""
        ranges = list(ranges)
        arr, _ = _make_ranges(ranges)
        dig = (N.Digest * max(len(ranges), 1))()
        ms = ctypes.c_double()
        L = N.lib()
        L.xlz_internal_batch_sha256_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(N.CheckRange), ctypes.c_size_t,
                                                       ctypes.POINTER(N.Digest), ctypes.POINTER(ctypes.c_double)]
        st = L.xlz_internal_batch_sha256_device(self._h, arr, len(ranges), dig, ctypes.byref(ms))
        if st != OK:
            raise LzmaError(st, "xlz_internal_batch_sha256_device")
        return _digest_values(ranges, dig), ms.value

    def filter(self, steps):
        """undo filter steps in place on the decoded outputs, on the device (xlz_batch_filter): download, device_output and
        checks see the filtered bytes afterwards.  steps: [(stream index, FILTER_*, parameter), ...]"""
        steps = list(steps)
        st = N.lib().xlz_batch_filter(self._h, _make_steps(steps), len(steps))
        if st != OK:
            raise LzmaError(st, "xlz_batch_filter")

    def pack(self, items, dptr, cap):
        """copy ranges of the decoded (and filtered) outputs into one device buffer, on the device (xlz_batch_pack).
        items: [(stream index, off, len, dst_off), ...], clipped to what each stream produced; dptr / cap: device memory of
        the context's device, as an integer address and its size -> the bytes copied per item"""
        items = list(items)
        n = len(items)
        arr = (N.PackItem * max(n, 1))()
        for q, (stream, off, length, dst_off) in enumerate(items):
            arr[q].stream, arr[q].off, arr[q].len, arr[q].dst_off = int(stream), int(off), int(length), int(dst_off)
        copied = (ctypes.c_uint64 * max(n, 1))()
        st = N.lib().xlz_batch_pack(self._h, arr, n, ctypes.c_void_p(int(dptr)), int(cap), copied)
        if st != OK:
            raise LzmaError(st, "xlz_batch_pack")
        return list(copied[:n])

    def bcj2(self, items, dptr, cap):
        """merge BCJ2 folders into one device buffer, on the device (xlz_batch_bcj2).  items: [(main, call, jump, rc, out_len,
        dst_off), ...] where main / call / jump are each a stream index of the batch (its decoded output) or bytes (uploaded
        by the call) and rc is bytes; dptr / cap: device memory of the context's device -> [(status, produced), ...]"""
        items = list(items)
        n = len(items)
        arr = (N.Bcj2Item * max(n, 1))()
        keep = []
        for q, (main, call, jump, rc, out_len, dst_off) in enumerate(items):
            for src, v in ((arr[q].main_s, main), (arr[q].call_s, call), (arr[q].jump_s, jump)):
                if isinstance(v, int):
                    src.stream = v
                else:
                    buf, p = _cbuf(v)
                    keep.append(buf)
                    src.stream, src.raw, src.raw_len = N.BCJ2_RAW, p, len(v)
            buf, p = _cbuf(rc)
            keep.append(buf)
            arr[q].rc, arr[q].rc_len, arr[q].out_len, arr[q].dst_off = p, len(rc), int(out_len), int(dst_off)
        res = (N.Bcj2Result * max(n, 1))()
        st = N.lib().xlz_batch_bcj2(self._h, arr, n, ctypes.c_void_p(int(dptr)), int(cap), res)
        if st != OK:
            raise LzmaError(st, "xlz_batch_bcj2")
        return [(res[q].status, res[q].produced) for q in range(n)]

    def download(self, i, length):
        buf = ctypes.create_string_buffer(max(int(length), 1))
        st = N.lib().xlz_batch_download(self._h, i, ctypes.cast(buf, ctypes.c_void_p), int(length))
        if st != OK:
            raise LzmaError(st, "xlz_batch_download")
        return buf.raw[:length]

    def device_output(self, i):
        p, cap = ctypes.c_void_p(), ctypes.c_size_t()
        st = N.lib().xlz_batch_device_output(self._h, i, ctypes.byref(p), ctypes.byref(cap))
        if st != OK:
            raise LzmaError(st, "xlz_batch_device_output")
        return p.value, cap.value

    def close(self):
        if self._h:
            N.lib().xlz_batch_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- exported helpers with the reference's names -------------------------------
def DecodeProp(d):
    """reader1.go:210-221 -> (lc, pb, lp); raises LzmaError(ErrIncorrectProperties)."""
    lc, pb, lp = ctypes.c_uint8(), ctypes.c_uint8(), ctypes.c_uint8()
    st = N.lib().xlz_decode_prop(d, ctypes.byref(lc), ctypes.byref(pb), ctypes.byref(lp))
    if st != OK:
        raise LzmaError(st)
    return lc.value, pb.value, lp.value


def DecodeDictSize(properties):
    """reader1.go:193-208"""
    return N.lib().xlz_decode_dict_size(bytes(properties[:4]))


def DecodeDictSize2(encoded):
    """reader2.go:296-298"""
    return N.lib().xlz_decode_dict_size2(encoded)


def DecodeUnpackSize(header):
    """reader1.go:178-191"""
    return N.lib().xlz_decode_unpack_size(bytes(header[:8]))


# ---- pull-style readers ----------------------------------------------------------
class io_EOF:  # sentinel standing in for Go's io.EOF
    pass


class _Reader:
    def __init__(self, ctx, handle, source=None, piece=1 << 20):
        self._ctx = ctx
        self._h = ctypes.c_void_p(handle)
        self._src = source  # file-like object the rest of the compressed stream is pulled from (streaming input)
        self._piece = piece
        if source is not None:
            st = N.lib().xlz_reader_expect_more(self._h)
            if st != OK:
                raise LzmaError(st, "xlz_reader_expect_more")

    def Read(self, n):
        """Go's Read(p []byte): returns (bytes, err) with err None, io_EOF or LzmaError.  With a
        source (NewReader1 / NewReader2 on a file object) the compressed side is pulled piece by piece
        as the decoder asks for it -- what the Go shim does with its io.Reader."""
        buf = ctypes.create_string_buffer(max(n, 1))
        err = ctypes.c_int()
        got = 0
        while True:
            k = N.lib().xlz_reader_read(self._h, ctypes.cast(ctypes.addressof(buf) + got, ctypes.c_void_p), n - got,
                                        ctypes.byref(err))
            got += k
            if err.value != NEED_INPUT or self._src is None:
                break
            more = self._src.read(self._piece)
            st = N.lib().xlz_reader_feed(self._h, more, len(more)) if more else N.lib().xlz_reader_feed_eof(self._h)
            if st != OK:
                return buf.raw[:got], LzmaError(st, "feeding the reader")
            if got == n and n:
                err.value = OK
                break
        e = None
        if err.value == EOF:
            e = io_EOF
        elif err.value != OK:
            e = LzmaError(err.value, "lzma: error reading" if self._is_closer else "")
        return buf.raw[:got], e

    def read_all(self, chunk=32768):
        """io.Copy(dst, r): returns (bytes, err) where err is None at io.EOF."""
        out = []
        while True:
            b, e = self.Read(chunk)
            out.append(b)
            if e is io_EOF:
                return b"".join(out), None
            if e is not None:
                return b"".join(out), e

    def stats(self):
        """(refill launches, whole-stream fallback decodes, compressed bytes uploaded) -- xlz_reader_stats"""
        a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        N.lib().xlz_reader_stats(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        return a.value, b.value, c.value

    def memory(self):
        """(bytes of the sliding output window on the device, bytes of the window image -- 0 until the stream's first
        dictionary reset behind a non-empty epoch) -- xlz_reader_memory"""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        N.lib().xlz_reader_memory(self._h, ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value

    def Close(self):
        """readCloser.Close (readcloser.go:16-28)."""
        st = N.lib().xlz_reader_close(self._h)
        if st != OK:
            return LzmaError(st)
        return None

    _is_closer = False

    def __del__(self):
        try:
            if self._h:
                N.lib().xlz_reader_free(self._h)
                self._h = ctypes.c_void_p()
        except Exception:
            pass


class Reader1(_Reader):
    def Reset(self):
        """(*Reader1).Reset (reader1.go:161-164)"""
        st = N.lib().xlz_reader_reset(self._h)
        if st != OK:
            raise LzmaError(st, "Reset")

    def Reopen(self, data, unpack_size=UNKNOWN_SIZE, piece=1 << 20):
        """(*Reader1).Reopen(inStream, unpackSize) (reader1.go:166-176): returns err.  `data`: the new raw stream as
        bytes, or a file-like object that is then pulled `piece` bytes at a time (the reference takes an io.ByteReader)"""
        head, src = _head_and_source(data, piece)
        st = N.lib().xlz_reader_reopen(self._h, head, len(head), unpack_size)
        self._src, self._piece = None, piece
        if st == ERR_HEADER_EOF:
            return io_EOF
        if st != OK:
            return LzmaError(st)
        if src is not None:
            st = N.lib().xlz_reader_expect_more(self._h)
            if st != OK:
                return LzmaError(st, "xlz_reader_expect_more")
            self._src = src
        return None


class Reader2(_Reader):
    pass


class ReadCloser(_Reader):
    _is_closer = True


def _head_and_source(data, piece):
    """bytes -> (bytes, None); a file-like object -> (its first piece, the object or None at its end)"""
    if hasattr(data, "read"):
        head = data.read(piece)
        return head, (data if len(head) == piece else None)
    return bytes(data), None


def NewReader1(ctx, data, piece=1 << 20):
    """NewReader1(inStream) (reader1.go:18-24): returns (reader, err).  `data`: the compressed bytes, or a
    file-like object that is then read `piece` bytes at a time as the decoder needs them."""
    head, src = _head_and_source(data, piece)
    err = ctypes.c_int()
    h = N.lib().xlz_new_reader1(ctx._h, head, len(head), ctypes.byref(err))
    if not h:
        return None, LzmaError(err.value)
    return Reader1(ctx, h, src, piece), None


def NewReader2(ctx, data, dict_size, piece=1 << 20):
    """NewReader2(inStream, dictSize) (reader2.go:26-41): returns (reader, err); `data` as for NewReader1."""
    head, src = _head_and_source(data, piece)
    err = ctypes.c_int()
    h = N.lib().xlz_new_reader2(ctx._h, head, len(head), dict_size, ctypes.byref(err))
    if not h:
        return None, LzmaError(err.value)
    return Reader2(ctx, h, src, piece), None


def _sevenzip(fn, ctx, props, unpack_size, readers):
    n = len(readers)
    arr = (ctypes.c_char_p * max(n, 1))(*[bytes(r) for r in readers])
    lens = (ctypes.c_size_t * max(n, 1))(*[len(r) for r in readers])
    err = ctypes.c_int()
    h = fn(ctx._h, bytes(props), len(props), unpack_size, arr, lens, n, ctypes.byref(err))
    if not h:
        return None, LzmaError(err.value)
    return ReadCloser(ctx, h), None


def NewLZMADecompressorForSevenZip(ctx, props, unpack_size, readers):
    """reader1.go:32-61: props = props byte + LE32 dict size; exactly one reader."""
    return _sevenzip(N.lib().xlz_new_lzma_decompressor_for_sevenzip, ctx, props, unpack_size, readers)


def NewLZMA2DecompressorForSevenZip(ctx, props, unpack_size, readers):
    """reader2.go:49-75: props = one dict-size byte; exactly one reader."""
    return _sevenzip(N.lib().xlz_new_lzma2_decompressor_for_sevenzip, ctx, props, unpack_size, readers)


def lzma2_units(data):
    """The unit plan of a raw LZMA2 stream (xlz_lzma2_units; host only): list of dicts (in_off, in_len, out_off,
    out_len, have_reader) -- what a decode of `data` as FMT_LZMA2_RAW launches, one wave per unit."""
    if hasattr(data, "ctypes"):   # a numpy array (uint8, contiguous): planned in place, whatever its size
        ptr, size = ctypes.c_char_p(data.ctypes.data), data.size
    else:
        data = bytes(data)
        ptr, size = data, len(data)
    n = ctypes.c_size_t()
    st = N.lib().xlz_lzma2_units(ptr, size, None, 0, ctypes.byref(n))
    if st != OK:
        raise LzmaError(st, "xlz_lzma2_units")
    units = (N.Lzma2Unit * max(n.value, 1))()
    st = N.lib().xlz_lzma2_units(ptr, size, units, n.value, ctypes.byref(n))
    if st != OK:
        raise LzmaError(st, "xlz_lzma2_units")
    return [{f: getattr(units[k], f) for f, _ in N.Lzma2Unit._fields_ if f != "reserved"} for k in range(n.value)]


# ---- .xz container front-end (include/xlz.h: xlz_xz_index / xlz_xz_decode) -------------------
def xz_index(data):
    """Block index of an .xz file: list of dicts (comp_off, comp_len, uncomp_off, uncomp_len,
    dict_size, check_type) and the total decoded size.  Host only."""
    buf = ctypes.create_string_buffer(data, len(data)) if len(data) else ctypes.create_string_buffer(1)
    n = ctypes.c_size_t()
    total = ctypes.c_uint64()
    st = N.lib().xlz_xz_index(ctypes.cast(buf, ctypes.c_void_p), len(data), None, 0, ctypes.byref(n), ctypes.byref(total))
    if st != OK:
        raise LzmaError(st, "xlz_xz_index")
    blocks = (N.XzBlock * max(n.value, 1))()
    st = N.lib().xlz_xz_index(ctypes.cast(buf, ctypes.c_void_p), len(data), blocks, n.value, ctypes.byref(n),
                              ctypes.byref(total))
    if st != OK:
        raise LzmaError(st, "xlz_xz_index")
    fields = [f for f, _ in N.XzBlock._fields_]
    return [{f: getattr(blocks[i], f) for f in fields} for i in range(n.value)], total.value


def xz_index_chains(data):
    """xz_index for files whose blocks carry Delta / BCJ filters in front of LZMA2 (xlz_xz_index_chains) -> (blocks, steps,
    total): steps = [(block index, FILTER_*, parameter), ...] in the order a decoder applies them.  Host only."""
    buf = ctypes.create_string_buffer(data, len(data)) if len(data) else ctypes.create_string_buffer(1)
    n, ns = ctypes.c_size_t(), ctypes.c_size_t()
    total = ctypes.c_uint64()
    st = N.lib().xlz_xz_index_chains(ctypes.cast(buf, ctypes.c_void_p), len(data), None, 0, ctypes.byref(n), None, 0, ctypes.byref(ns),
                                     ctypes.byref(total))
    if st != OK:
        raise LzmaError(st, "xlz_xz_index_chains")
    blocks = (N.XzBlock * max(n.value, 1))()
    steps = (N.FilterStep * max(ns.value, 1))()
    st = N.lib().xlz_xz_index_chains(ctypes.cast(buf, ctypes.c_void_p), len(data), blocks, n.value, ctypes.byref(n), steps, ns.value,
                                     ctypes.byref(ns), ctypes.byref(total))
    if st != OK:
        raise LzmaError(st, "xlz_xz_index_chains")
    fields = [f for f, _ in N.XzBlock._fields_]
    return ([{f: getattr(blocks[i], f) for f in fields} for i in range(n.value)],
            [(steps[i].stream, steps[i].id, steps[i].param) for i in range(ns.value)], total.value)


def xz_decode(ctx, data, verify=True, max_size=None):
    """Decode a whole .xz file (all streams, all blocks) as one GPU batch -> bytes.
    verify: check every block's CRC32 / CRC64.  max_size: refuse (ERR_OUT_CAP) a file whose index announces more.
    Blocks with Delta / BCJ filters are decoded when the context is in filter mode 1 (Context.set_filter_mode)."""
    total = xz_index_chains(data)[2] if ctx.filter_mode() == 1 else xz_index(data)[1]
    if max_size is not None and total > max_size:
        raise LzmaError(ERR_OUT_CAP, "xlz_xz_decode: the index announces %d bytes, max_size is %d" % (total, max_size))
    out = ctypes.create_string_buffer(max(total, 1))
    n = xz_decode_into(ctx, data, out, verify=verify)
    return out.raw[:n]


def xz_decode_on(ctxs, data, verify=True):
    """xlz_xz_decode_multi: the file's blocks -- and the units inside large blocks -- dealt to several contexts -> bytes"""
    _, total = xz_index(data)
    out = ctypes.create_string_buffer(max(total, 1))
    hs = (ctypes.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    out_len, unverified = ctypes.c_uint64(), ctypes.c_size_t()
    data = bytes(data)
    st = N.lib().xlz_xz_decode_multi(hs, len(ctxs), ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p), len(data),
                                     ctypes.cast(out, ctypes.c_void_p), total, ctypes.byref(out_len), 1 if verify else 0,
                                     ctypes.byref(unverified))
    if st != OK:
        raise LzmaError(st, "xlz_xz_decode_multi")
    return out.raw[: out_len.value]


def xz_decode_into(ctx, data, out, verify=True):
    """xlz_xz_decode with the caller's buffers and nothing else: `data` is read in place (bytes, or any object with the
    buffer interface), the decoded bytes land in `out` (a writable buffer of at least the index's total: bytearray,
    numpy array, ctypes array) -> number of bytes decoded.  What bench.py times for the container line."""
    if not isinstance(data, bytes):
        data = bytes(data)
    src_ptr = ctypes.c_char_p(data)  # the library only reads it: no copy
    dst = out if isinstance(out, ctypes.Array) else (ctypes.c_char * memoryview(out).nbytes).from_buffer(out)
    out_len = ctypes.c_uint64()
    unverified = ctypes.c_size_t()
    st = N.lib().xlz_xz_decode(ctx._h, ctypes.cast(src_ptr, ctypes.c_void_p), len(data), ctypes.cast(dst, ctypes.c_void_p),
                               ctypes.sizeof(dst), ctypes.byref(out_len), 1 if verify else 0, ctypes.byref(unverified))
    if st != OK:
        raise LzmaError(st, "xlz_xz_decode")
    return out_len.value


def sevenzip_decode_on(ctxs, data, verify=True):
    """xlz_7z_decode_multi: the archive's folders dealt to several contexts -> the files' bytes back to back"""
    _, _, total = sevenzip_index(data, ctxs[0])
    buf = ctypes.create_string_buffer(data, len(data))
    out = ctypes.create_string_buffer(max(total, 1))
    hs = (ctypes.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    out_len, unverified = ctypes.c_uint64(), ctypes.c_size_t()
    st = N.lib().xlz_7z_decode_multi(hs, len(ctxs), ctypes.cast(buf, ctypes.c_void_p), len(data), ctypes.cast(out, ctypes.c_void_p),
                                     total, ctypes.byref(out_len), 1 if verify else 0, ctypes.byref(unverified))
    if st != OK:
        raise LzmaError(st, "xlz_7z_decode_multi")
    return out.raw[: out_len.value]


# ---- .7z container front-end (include/xlz.h: xlz_7z_index / xlz_7z_decode) -------------------
def sevenzip_index(data, ctx=None):
    """Folder list of a .7z archive: (list of folder dicts, list of (size, crc or None) per file, total
    decoded size).  ctx is needed when the archive's header is itself compressed (7-Zip's default)."""
    buf = ctypes.create_string_buffer(data, len(data)) if len(data) else ctypes.create_string_buffer(1)
    h = ctx._h if ctx is not None else None
    nf, ns, total = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_uint64()
    st = N.lib().xlz_7z_index(h, ctypes.cast(buf, ctypes.c_void_p), len(data), None, 0, ctypes.byref(nf), None, 0,
                              ctypes.byref(ns), ctypes.byref(total))
    if st != OK:
        raise LzmaError(st, "xlz_7z_index")
    fo = (N.SzFolder * max(nf.value, 1))()
    su = (N.SzSubstream * max(ns.value, 1))()
    st = N.lib().xlz_7z_index(h, ctypes.cast(buf, ctypes.c_void_p), len(data), fo, nf.value, ctypes.byref(nf), su, ns.value,
                              ctypes.byref(ns), ctypes.byref(total))
    if st != OK:
        raise LzmaError(st, "xlz_7z_index")
    fields = [f for f, _ in N.SzFolder._fields_ if f != "reserved"]
    return ([{f: getattr(fo[i], f) for f in fields} for i in range(nf.value)],
            [(su[i].size, su[i].crc if su[i].has_crc else None) for i in range(ns.value)], total.value)


def sevenzip_index_chains(data, ctx=None):
    """sevenzip_index for archives whose folders are Delta / BCJ filters behind an LZMA / LZMA2 coder (xlz_7z_index_chains)
    -> (folders, files, steps, total): such a folder carries its LZMA / LZMA2 coder's method, props and dictionary, and
    steps = [(folder index, FILTER_*, parameter), ...] in the order a decoder applies them"""
    buf = ctypes.create_string_buffer(data, len(data)) if len(data) else ctypes.create_string_buffer(1)
    h = ctx._h if ctx is not None else None
    nf, ns, nst, total = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_uint64()
    st = N.lib().xlz_7z_index_chains(h, ctypes.cast(buf, ctypes.c_void_p), len(data), None, 0, ctypes.byref(nf), None, 0,
                                     ctypes.byref(ns), None, 0, ctypes.byref(nst), ctypes.byref(total))
    if st != OK:
        raise LzmaError(st, "xlz_7z_index_chains")
    fo = (N.SzFolder * max(nf.value, 1))()
    su = (N.SzSubstream * max(ns.value, 1))()
    steps = (N.FilterStep * max(nst.value, 1))()
    st = N.lib().xlz_7z_index_chains(h, ctypes.cast(buf, ctypes.c_void_p), len(data), fo, nf.value, ctypes.byref(nf), su, ns.value,
                                     ctypes.byref(ns), steps, nst.value, ctypes.byref(nst), ctypes.byref(total))
    if st != OK:
        raise LzmaError(st, "xlz_7z_index_chains")
    fields = [f for f, _ in N.SzFolder._fields_ if f != "reserved"]
    return ([{f: getattr(fo[i], f) for f in fields} for i in range(nf.value)],
            [(su[i].size, su[i].crc if su[i].has_crc else None) for i in range(ns.value)],
            [(steps[i].stream, steps[i].id, steps[i].param) for i in range(nst.value)], total.value)


def sevenzip_index_bcj2(data, ctx=None):
    """sevenzip_index_chains plus the BCJ2 folders (xlz_7z_index_bcj2) -> (folders, files, steps, bcj2, total): a BCJ2 folder
    has method 4 and the size of its merged bytes, and a record in bcj2: {"folder": index, "main" / "call" / "jump":
    {pack_off, pack_len, unpack_len, method (1 LZMA, 2 LZMA2, 3 read raw), dict_size, props}, "rc_off", "rc_len"}"""
    buf, bp = _cbuf(data)
    h = ctx._h if ctx is not None else None
    nf, ns, nst, nb, total = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_uint64()
    st = N.lib().xlz_7z_index_bcj2(h, bp, len(data), None, 0, ctypes.byref(nf), None, 0, ctypes.byref(ns), None, 0, ctypes.byref(nst),
                                   None, 0, ctypes.byref(nb), ctypes.byref(total))
    if st != OK:
        raise LzmaError(st, "xlz_7z_index_bcj2")
    fo = (N.SzFolder * max(nf.value, 1))()
    su = (N.SzSubstream * max(ns.value, 1))()
    steps = (N.FilterStep * max(nst.value, 1))()
    recs = (N.SzBcj2 * max(nb.value, 1))()
    st = N.lib().xlz_7z_index_bcj2(h, bp, len(data), fo, nf.value, ctypes.byref(nf), su, ns.value, ctypes.byref(ns), steps, nst.value,
                                   ctypes.byref(nst), recs, nb.value, ctypes.byref(nb), ctypes.byref(total))
    if st != OK:
        raise LzmaError(st, "xlz_7z_index_bcj2")
    fields = [f for f, _ in N.SzFolder._fields_ if f != "reserved"]
    sub_fields = [f for f, _ in N.SzBcj2Sub._fields_ if f != "reserved"]

    def sub(s):
        return {f: getattr(s, f) for f in sub_fields}
    return ([{f: getattr(fo[i], f) for f in fields} for i in range(nf.value)],
            [(su[i].size, su[i].crc if su[i].has_crc else None) for i in range(ns.value)],
            [(steps[i].stream, steps[i].id, steps[i].param) for i in range(nst.value)],
            [{"folder": recs[i].folder, "main": sub(recs[i].main_s), "call": sub(recs[i].call_s), "jump": sub(recs[i].jump_s),
              "rc_off": recs[i].rc_off, "rc_len": recs[i].rc_len} for i in range(nb.value)], total.value)


def _sevenzip_total(ctx, data):
    """the decoded size a .7z front-end call on `ctx` will want: with BCJ2 folders in bcj2 mode 1 / 2 (their merged size),
    with chains in filter mode 1"""
    if ctx.bcj2_mode() != 0 and hasattr(N.lib(), "xlz_7z_index_bcj2"):
        return sevenzip_index_bcj2(data, ctx)[4]
    if ctx.filter_mode() == 1:
        return sevenzip_index_chains(data, ctx)[3]
    return sevenzip_index(data, ctx)[2]


def sevenzip_decode(ctx, data, verify=True, max_size=None):
    """Decode every folder of a .7z archive as one GPU batch -> the files' bytes back to back.
    max_size: refuse (ERR_OUT_CAP) an archive whose header announces more decoded bytes than that -- the sizes come
    from an untrusted header and the output buffer is allocated from them."""
    total = _sevenzip_total(ctx, data) if ctx.bcj2_mode() != 0 else sevenzip_index(data, ctx)[2]
    if max_size is not None and total > max_size:
        raise LzmaError(ERR_OUT_CAP, "xlz_7z_decode: the archive announces %d bytes, max_size is %d" % (total, max_size))
    buf = ctypes.create_string_buffer(data, len(data))
    out = ctypes.create_string_buffer(max(total, 1))
    out_len = ctypes.c_uint64()
    unverified = ctypes.c_size_t()
    st = N.lib().xlz_7z_decode(ctx._h, ctypes.cast(buf, ctypes.c_void_p), len(data), ctypes.cast(out, ctypes.c_void_p),
                               total, ctypes.byref(out_len), 1 if verify else 0, ctypes.byref(unverified))
    if st != OK:
        raise LzmaError(st, "xlz_7z_decode")
    return out.raw[: out_len.value]


# ---- the container front-ends into device memory (include/xlz.h: xlz_xz_decode_device / xlz_7z_decode_device) ----
def _decode_device(name, ctx, data, dptr, cap, verify):
    if not isinstance(data, bytes):
        data = bytes(data)
    out_len, unverified = ctypes.c_uint64(), ctypes.c_size_t()
    st = getattr(N.lib(), name)(ctx._h, ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p), len(data), ctypes.c_void_p(int(dptr)),
                                int(cap), ctypes.byref(out_len), 1 if verify else 0, ctypes.byref(unverified))
    if st != OK:
        raise LzmaError(st, name)
    return out_len.value


def xz_decode_device(ctx, data, dptr, cap, verify=True):
    """xlz_xz_decode_device: decode a whole .xz file into `cap` bytes of device memory at the address `dptr` (on the
    context's device), contiguous; decode, filters, checks and the pack run on the device -> number of bytes decoded.
    Raises LzmaError as xz_decode does.  The call needs about twice the decoded size of device memory."""
    return _decode_device("xlz_xz_decode_device", ctx, data, dptr, cap, verify)


def sevenzip_decode_device(ctx, data, dptr, cap, verify=True):
    """xlz_7z_decode_device: the same for a .7z archive -> number of bytes decoded (the files back to back)"""
    return _decode_device("xlz_7z_decode_device", ctx, data, dptr, cap, verify)


def _tensor_out(ctx, total, out, what):
    """the tensor a *_tensor call writes: `out` if it is a contiguous one-dimensional torch.uint8 tensor of at least `total`
    bytes on the context's device, a new one if it is None; `what` says who wants `total`, for the ERR_OUT_CAP text"""
    import torch  # (only here: importing lzma_amd does not import torch)
    dev = torch.device("cuda", N.lib().xlz_ctx_device(ctx._h))
    if out is None:
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.device == dev and out.dim() == 1 and out.is_contiguous()):
        raise ValueError("out must be a contiguous one-dimensional torch.uint8 tensor on %s" % dev)
    elif out.numel() < total:
        raise LzmaError(ERR_OUT_CAP, "%s %d bytes, out holds %d" % (what, total, out.numel()))
    torch.cuda.synchronize(dev)  # (torch's pending work on the tensor; the library works on a stream of its own and waits for it)
    return out


def _decode_tensor(decode, total, ctx, data, verify, out):
    out = _tensor_out(ctx, total, out, "the index announces")
    n = decode(ctx, data, out.data_ptr(), out.numel(), verify=verify)
    return out[:n]


def xz_decode_tensor(ctx, data, verify=True, out=None):
    """xz_decode_device into a torch.uint8 tensor on the context's device: `out` (one-dimensional, contiguous, at least the
    index's total; ERR_OUT_CAP if smaller) or a new one -> the tensor cut to the decoded size"""
    total = xz_index_chains(data)[2] if ctx.filter_mode() == 1 else xz_index(data)[1]
    return _decode_tensor(xz_decode_device, total, ctx, data, verify, out)


def sevenzip_decode_tensor(ctx, data, verify=True, out=None):
    """sevenzip_decode_device into a torch.uint8 tensor on the context's device, as xz_decode_tensor"""
    total = _sevenzip_total(ctx, data)
    return _decode_tensor(sevenzip_decode_device, total, ctx, data, verify, out)


# ---- byte ranges of an .xz file (include/xlz.h: xlz_xz_open / xlz_xz_cover / xlz_xz_read / xlz_xz_read_device) ----
class _PyBuffer(ctypes.Structure):  # Py_buffer of the C API: what PyObject_GetBuffer fills in
    _fields_ = [("buf", ctypes.c_void_p), ("obj", ctypes.py_object), ("len", ctypes.c_ssize_t), ("itemsize", ctypes.c_ssize_t),
                ("readonly", ctypes.c_int), ("ndim", ctypes.c_int), ("format", ctypes.c_char_p), ("shape", ctypes.POINTER(ctypes.c_ssize_t)),
                ("strides", ctypes.POINTER(ctypes.c_ssize_t)), ("suboffsets", ctypes.POINTER(ctypes.c_ssize_t)), ("internal", ctypes.c_void_p)]


class _Borrowed:
    """what XzFile, SevenZipFile and ZipFile are made on: `data` borrowed through the buffer protocol and the library's handle
    over it, both held until close().  _name: the class as its messages call it; _close: the xlz_*_close of its handle"""
    _name = _close = None

    def _borrow(self, data):
        self._h = ctypes.c_void_p()
        self._view = _PyBuffer()
        if ctypes.pythonapi.PyObject_GetBuffer(ctypes.py_object(data), ctypes.byref(self._view), 0) != 0:  # (raises: no buffer, not contiguous)
            raise TypeError("%s needs bytes or a contiguous buffer" % self._name)
        self._held = True

    def _handle(self):
        if not self._h:
            raise LzmaError(ERR_CLOSED, "%s is closed" % self._name)
        return self._h

    def close(self):
        if self._h:
            getattr(N.lib(), self._close)(self._h)
            self._h = ctypes.c_void_p()
        if getattr(self, "_held", False):
            self._held = False
            ctypes.pythonapi.PyBuffer_Release(ctypes.byref(self._view))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class XzFile(_Borrowed):
    """The parsed index of one .xz file (xlz_xz_open; host only): reads of byte ranges of the DECODED file decode the blocks
    that hold them and nothing else.  `data` is bytes or any contiguous buffer (bytearray, memoryview, mmap -- read-only
    ones too): it is borrowed through the buffer protocol, never copied, and held until close().  Raises LzmaError as
    xz_index_chains does.  Read-only once made: one XzFile may serve several threads and contexts.  A context manager;
    close() may be repeated."""
    _name, _close = "XzFile", "xlz_xz_close"

    def __init__(self, data):
        self._borrow(data)
        try:
            st = N.lib().xlz_xz_open(ctypes.c_void_p(self._view.buf), self._view.len, ctypes.byref(self._h))
            if st != OK:
                self._h = ctypes.c_void_p()
                raise LzmaError(st, "xlz_xz_open")
            size, nb, ns = ctypes.c_uint64(), ctypes.c_size_t(), ctypes.c_size_t()
            N.lib().xlz_xz_file_info(self._h, ctypes.byref(size), ctypes.byref(nb), ctypes.byref(ns))
            self.size = size.value
            blocks = (N.XzBlock * max(nb.value, 1))()
            st = N.lib().xlz_xz_file_blocks(self._h, blocks, nb.value)
            if st != OK:
                raise LzmaError(st, "xlz_xz_file_blocks")
        except Exception:
            self.close()
            raise
        fields = [f for f, _ in N.XzBlock._fields_]
        self.blocks = [{f: getattr(blocks[i], f) for f in fields} for i in range(nb.value)]
        self.steps = ns.value  # how many filter steps the blocks carry (xz_index_chains lists them)

    @staticmethod
    def _ranges(ranges):
        arr = (N.XzRange * max(len(ranges), 1))()
        for i, r in enumerate(ranges):
            arr[i].off, arr[i].len, arr[i].dst_off = int(r[0]), int(r[1]), int(r[2]) if len(r) > 2 else 0
        return arr

    def cover(self, ranges):
        """xlz_xz_cover: the ascending indices of the blocks that [(off, n), ...] touch.  Host only."""
        arr = self._ranges(ranges)
        blocks = (ctypes.c_size_t * max(len(self.blocks), 1))()
        n = ctypes.c_size_t()
        st = N.lib().xlz_xz_cover(self._handle(), arr, len(ranges), blocks, len(self.blocks), ctypes.byref(n))
        if st != OK:
            raise LzmaError(st, "xlz_xz_cover")
        return list(blocks[: n.value])

    def _read(self, name, ctx, arr, n, dst, cap, verify):
        copied = (ctypes.c_uint64 * max(n, 1))()
        unverified = ctypes.c_size_t()
        st = getattr(N.lib(), name)(ctx._h, self._handle(), arr, n, dst, cap, copied, 1 if verify else 0, ctypes.byref(unverified))
        if st != OK:
            raise LzmaError(st, name)
        ctx.last_xz_unverified = unverified.value  # (on the context, like the statistics: the XzFile stays read-only)
        return list(copied[:n])

    def read_ranges(self, ctx, ranges, verify=True):
        """xlz_xz_read of [(off, n), ...] -> list[bytes], each short where the file ends; ONE batch of the covering blocks"""
        laid, at = [], 0
        for off, n in ranges:
            n = min(int(n), max(self.size - int(off), 0))
            laid.append((off, n, at))
            at += n
        out = ctypes.create_string_buffer(max(at, 1))
        copied = self._read("xlz_xz_read", ctx, self._ranges(laid), len(laid), ctypes.cast(out, ctypes.c_void_p), at, verify)
        return [out[d:d + c] for (_, _, d), c in zip(laid, copied)]

    def read(self, ctx, off, n, verify=True):
        """bytes [off, off + n) of the decoded file, like pread: short at the end of the file, b"" behind it"""
        return self.read_ranges(ctx, [(off, n)], verify=verify)[0]

    def read_device(self, ctx, ranges_with_dst, dptr, cap, verify=True):
        """xlz_xz_read_device: [(off, n, dst_off), ...] into `cap` bytes of device memory at the address `dptr` (on the
        context's device), range i to dptr + dst_off -> the bytes written per range"""
        return self._read("xlz_xz_read_device", ctx, self._ranges(ranges_with_dst), len(ranges_with_dst), ctypes.c_void_p(int(dptr)),
                          int(cap), verify)

    def read_tensor(self, ctx, off, n, verify=True, out=None):
        """read_device of one range into a torch.uint8 tensor on the context's device: `out` (one-dimensional, contiguous, at
        least the clipped length; ERR_OUT_CAP if smaller) or a new one -> the tensor cut to the bytes read"""
        want = min(int(n), max(self.size - int(off), 0))

        def read(ctx, data, dptr, cap, verify):
            return self.read_device(ctx, [(off, want, 0)], dptr, cap, verify=verify)[0]
        return _decode_tensor(read, want, ctx, None, verify, out)


# ---- the files of a .7z archive (include/xlz.h: xlz_7z_open / xlz_7z_cover / xlz_7z_extract / xlz_7z_extract_device) ----
SevenZipEntry = collections.namedtuple("SevenZipEntry", "name size is_dir has_stream crc mtime attributes folder folder_off is_anti")


class _EntryArchive(_Borrowed):
    """what SevenZipFile and ZipFile share: an entry from its index or name, the windows of wanted entries, the three
    forms of an extraction.  _prefix: of the C functions ("xlz_7z", "xlz_zip"); _Want / _Result: their structs; _row: the
    fields of a result that make its tuple, status and out_len first"""
    _prefix = _Want = _Result = _row = None

    def index(self, which):
        """an entry's index from an index or a name (the first entry of that name)"""
        if isinstance(which, str):
            try:
                return self.names.index(which)
            except ValueError:
                raise KeyError(which)
        return int(which)

    def _list(self, which):
        return [self.index(w) for w in ([which] if isinstance(which, (int, str)) else which)]

    def _wants(self, wants):
        arr = (self._Want * max(len(wants), 1))()
        for i, w in enumerate(wants):
            arr[i].entry, arr[i].dst_off, arr[i].dst_cap = int(w[0]), int(w[1]), int(w[2])
        return arr

    def layout(self, which, align=1):
        idx = self._list(which)
        arr = self._wants([(i, 0, 0) for i in idx])
        total = ctypes.c_uint64()
        name = self._prefix + "_extract_layout"
        st = getattr(N.lib(), name)(self._handle(), arr, len(idx), int(align), ctypes.byref(total))
        if st != OK:
            raise LzmaError(st, name)
        return [(arr[i].entry, arr[i].dst_off, arr[i].dst_cap) for i in range(len(idx))], total.value

    def _extract(self, name, ctx, wants, dst, cap, verify):
        res = (self._Result * max(len(wants), 1))()
        st = getattr(N.lib(), name)(ctx._h if ctx is not None else None, self._handle(), self._wants(wants), len(wants), dst, int(cap),
                                    1 if verify else 0, res)
        if st != OK:
            raise LzmaError(st, name)
        return [tuple(getattr(res[i], f) for f in self._row) for i in range(len(wants))]

    def extract_into(self, ctx, wants, out, verify=True):
        dst = out if isinstance(out, ctypes.Array) else (ctypes.c_char * memoryview(out).nbytes).from_buffer(out)
        return self._extract(self._prefix + "_extract", ctx, wants, ctypes.cast(dst, ctypes.c_void_p), ctypes.sizeof(dst), verify)

    def extract_device(self, ctx, wants, dptr, cap, verify=True):
        return self._extract(self._prefix + "_extract_device", ctx, wants, ctypes.c_void_p(int(dptr)), cap, verify)

    def extract_tensor(self, ctx, which, verify=True, align=1, out=None):
        """extract_device into a torch.uint8 tensor on the context's device: `out` (one-dimensional, contiguous, at least the
        layout's total; ERR_OUT_CAP if smaller) or a new one -> (tensor, [(entry, off, out_len, status)]): an entry is
        tensor[off:off + out_len] where its status is OK"""
        wants, total = self.layout(which, align)
        out = _tensor_out(ctx, total, out, "the layout needs")
        res = self.extract_device(ctx, wants, out.data_ptr(), out.numel(), verify=verify)
        return out, [(w[0], w[1], r[1], r[0]) for w, r in zip(wants, res)]


class SevenZipFile(_EntryArchive):
    """The file table of one .7z archive (xlz_7z_open) and the extraction of chosen files as ONE batch: the folders that hold
    them, each decoded only as far as the last wanted file reaches.  `data` is bytes or any contiguous buffer; it is
    borrowed through the buffer protocol, never copied, and held until close().  ctx: needed only for an archive whose
    header is encoded (it is decoded on the device).  Raises LzmaError as sevenzip_index_bcj2 does, and for a FilesInfo
    section the parser refuses.  Names are AS STORED in the archive: do not trust one as a path.  Read-only once made; a
    context manager; close() may be repeated."""
    _name, _close, _prefix = "SevenZipFile", "xlz_7z_close", "xlz_7z"
    _Want, _Result, _row = N.SzWant, N.SzFileResult, ("status", "out_len", "unverified")

    def __init__(self, data, ctx=None):
        self._borrow(data)
        try:
            L = N.lib()
            st = L.xlz_7z_open(ctx._h if ctx is not None else None, ctypes.c_void_p(self._view.buf), self._view.len, ctypes.byref(self._h))
            if st != OK:
                self._h = ctypes.c_void_p()
                raise LzmaError(st, "xlz_7z_open")
            ne, nf, nb, total = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_uint64()
            L.xlz_7z_archive_info(self._h, ctypes.byref(ne), ctypes.byref(nf), ctypes.byref(nb), ctypes.byref(total))
            ents = (N.SzEntry * max(ne.value, 1))()
            pool = ctypes.create_string_buffer(max(nb.value, 1))
            st = L.xlz_7z_archive_entries(self._h, ents, ne.value, ctypes.cast(pool, ctypes.c_void_p), nb.value)
            if st != OK:
                raise LzmaError(st, "xlz_7z_archive_entries")
            fo = (N.SzFolder * max(nf.value, 1))()
            st = L.xlz_7z_archive_folders(self._h, fo, nf.value)
            if st != OK:
                raise LzmaError(st, "xlz_7z_archive_folders")
        except Exception:
            self.close()
            raise
        self.total_size = total.value
        raw = pool.raw
        self.entries = []
        for i in range(ne.value):
            x = ents[i]
            has_stream = bool(x.flags & N.SZ_ENTRY_HAS_STREAM)
            mtime = (x.mtime - 116444736000000000) / 1e7 if x.flags & N.SZ_ENTRY_HAS_MTIME else None  # FILETIME -> Unix seconds
            self.entries.append(SevenZipEntry(
                raw[x.name_off:x.name_off + x.name_len].decode("utf-8"), x.size, bool(x.flags & N.SZ_ENTRY_IS_DIR), has_stream,
                x.crc if x.flags & N.SZ_ENTRY_HAS_CRC else None, mtime, x.attributes if x.flags & N.SZ_ENTRY_HAS_ATTRIBUTES else None,
                x.folder if has_stream else None, x.folder_off if has_stream else None, bool(x.flags & N.SZ_ENTRY_IS_ANTI)))
        fields = [f for f, _ in N.SzFolder._fields_ if f != "reserved"]
        self.folders = [{f: getattr(fo[i], f) for f in fields} for i in range(nf.value)]
        self.names = [e.name for e in self.entries]

    def cover(self, which):
        """xlz_7z_cover: [(folder, decode_len, in_len)] for the wanted entries (indices or names).  Host only."""
        idx = self._list(which)
        arr = (ctypes.c_uint64 * max(len(idx), 1))(*idx)
        items = (N.SzCoverItem * max(len(self.folders), 1))()
        n = ctypes.c_size_t()
        st = N.lib().xlz_7z_cover(self._handle(), arr, len(idx), items, len(self.folders), ctypes.byref(n))
        if st != OK:
            raise LzmaError(st, "xlz_7z_cover")
        return [(items[i].folder, items[i].decode_len, items[i].in_len) for i in range(n.value)]

    def layout(self, which, align=1):
        """xlz_7z_extract_layout: windows of the wanted entries back to back -> ([(entry, dst_off, dst_cap)], total)"""
        return super().layout(which, align)

    def extract_into(self, ctx, wants, out, verify=True):
        """xlz_7z_extract with the caller's buffer: wants = [(entry, dst_off, dst_cap)] into `out` (a writable buffer); the
        windows of entries with bytes must not overlap -> [(status, out_len, unverified)]"""
        return super().extract_into(ctx, wants, out, verify)

    def extract_device(self, ctx, wants, dptr, cap, verify=True):
        """xlz_7z_extract_device: the same into `cap` bytes of device memory at the address `dptr` (on the context's device)"""
        return super().extract_device(ctx, wants, dptr, cap, verify)

    def extract(self, ctx, which, verify=True):
        """the wanted entries (indices or names) as ONE batch -> a list with bytes, or an LzmaError INSTANCE, per entry; only
        what concerns the whole call is raised"""
        wants, total = self.layout(which)
        out = ctypes.create_string_buffer(max(total, 1))
        res = self._extract(self._prefix + "_extract", ctx, wants, ctypes.cast(out, ctypes.c_void_p), total, verify)
        base = ctypes.addressof(out)
        return [ctypes.string_at(base + w[1], n) if st == OK else LzmaError(st, "xlz_7z_extract: entry %d" % w[0])
                for w, (st, n, _) in zip(wants, res)]

    def read(self, ctx, which, verify=True):
        """one entry's bytes (b"" for an entry without a stream); raises LzmaError"""
        got = self.extract(ctx, [self.index(which)], verify=verify)[0]
        if isinstance(got, LzmaError):
            raise got
        return got


# ---- the entries of a .zip archive (include/xlz.h: xlz_zip_open / xlz_zip_extract / xlz_zip_extract_device) ----
class ZipFile(_EntryArchive):
    """The table of one .zip archive (xlz_zip_open; host only) and the extraction of chosen entries as ONE batch: every
    wanted method-14 (LZMA) entry is a stream of one decode launch sequence, stored entries go up in one transfer, the
    CRC32 of every entry is checked on the device.  `data` is bytes or any contiguous buffer; it is borrowed through the
    buffer protocol, never copied, and held until close().  Raises LzmaError where the central directory cannot be walked
    or the archive spans disks; what is wrong with one entry (deflate, encryption, a broken header) is that entry's
    status when it is extracted.  .entries: one dict per entry with the fields of xlz_zip_entry, `name`, `mtime` (a tuple
    like zipfile's date_time) and `supported`, `is_dir`, `bad`, `deflate` (method 8 and well formed: extracted in the
    context's deflate mode 1 / 2, refused in mode 0; `supported` is false for it as ever); .names: decoded as zipfile does, UTF-8 where flag bit 11
    is set, else CP437.  Names are AS STORED in the archive: do not trust one as a path.  Read-only once made; a context
    manager; close() may be repeated."""
    _name, _close, _prefix = "ZipFile", "xlz_zip_close", "xlz_zip"
    _Want, _Result, _row = N.ZipWant, N.ZipFileResult, ("status", "out_len")

    def __init__(self, data):
        self._borrow(data)
        try:
            L = N.lib()
            st = L.xlz_zip_open(ctypes.c_void_p(self._view.buf), self._view.len, ctypes.byref(self._h))
            if st != OK:
                self._h = ctypes.c_void_p()
                raise LzmaError(st, "xlz_zip_open")
            ne, nb, total, shift = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_uint64(), ctypes.c_uint64()
            L.xlz_zip_archive_info(self._h, ctypes.byref(ne), ctypes.byref(nb), ctypes.byref(total), ctypes.byref(shift))
            ents = (N.ZipEntry * max(ne.value, 1))()
            pool = ctypes.create_string_buffer(max(nb.value, 1))
            st = L.xlz_zip_archive_entries(self._h, ents, ne.value, ctypes.cast(pool, ctypes.c_void_p), nb.value)
            if st != OK:
                raise LzmaError(st, "xlz_zip_archive_entries")
        except Exception:
            self.close()
            raise
        self.total_size, self.shift = total.value, shift.value
        raw = pool.raw
        fields = [f for f, _ in N.ZipEntry._fields_ if f not in ("reserved", "name_off", "name_len")]
        self.entries = []
        for i in range(ne.value):
            x = ents[i]
            d = {f: getattr(x, f) for f in fields}
            stored = raw[x.name_off:x.name_off + x.name_len]
            d["name"] = stored.decode("utf-8" if x.flags & N.ZIP_ENTRY_UTF8 else "cp437", "replace")
            t, day = x.dos_time_date & 0xFFFF, x.dos_time_date >> 16
            d["mtime"] = ((day >> 9) + 1980, (day >> 5) & 15, day & 31, t >> 11, (t >> 5) & 63, (t & 31) * 2)
            d["supported"], d["is_dir"], d["bad"] = (bool(x.flags & N.ZIP_ENTRY_SUPPORTED), bool(x.flags & N.ZIP_ENTRY_IS_DIR),
                                                     bool(x.flags & N.ZIP_ENTRY_BAD))
            d["deflate"] = bool(x.flags & N.ZIP_ENTRY_DEFLATE)
            self.entries.append(d)
        self.names = [e["name"] for e in self.entries]

    def layout(self, which, align=1):
        """xlz_zip_extract_layout: windows of the wanted entries back to back -> ([(entry, dst_off, dst_cap)], total)"""
        return super().layout(which, align)

    def extract_into(self, ctx, wants, out, verify=True):
        """xlz_zip_extract with the caller's buffer: wants = [(entry, dst_off, dst_cap)] into `out` (a writable buffer); the
        windows of entries with bytes must not overlap -> [(status, out_len)]"""
        return super().extract_into(ctx, wants, out, verify)

    def extract_device(self, ctx, wants, dptr, cap, verify=True):
        """xlz_zip_extract_device: the same into `cap` bytes of device memory at the address `dptr` (on the context's device)"""
        return super().extract_device(ctx, wants, dptr, cap, verify)

    def extract(self, ctx, which, verify=True):
        """the wanted entries (indices or names) as ONE batch -> [(status, bytes)], bytes empty unless the status is OK; only
        what concerns the whole call is raised"""
        wants, total = self.layout(which)
        out = ctypes.create_string_buffer(max(total, 1))
        res = self._extract(self._prefix + "_extract", ctx, wants, ctypes.cast(out, ctypes.c_void_p), total, verify)
        base = ctypes.addressof(out)
        return [(st, ctypes.string_at(base + w[1], n) if st == OK else b"") for w, (st, n) in zip(wants, res)]

    def read(self, ctx, which, verify=True):
        """one entry's bytes (b"" for a directory); raises LzmaError on a failed entry"""
        i = self.index(which)
        st, got = self.extract(ctx, [i], verify=verify)[0]
        if st != OK:
            raise LzmaError(st, "xlz_zip_extract: entry %d" % i)
        return got


# ---- the members of a .tar image (include/xlz.h: xlz_tar_parse_host / xlz_tar_scan_device / xlz_xz_tar_list) ----
TarEntry = collections.namedtuple("TarEntry", "name linkname size type mode uid gid mtime hdr_off data_off")
TarTable = collections.namedtuple("TarTable", "entries end_status end_off")


def _tar_table(h):
    """the table of an xlz_tar handle, which is closed -> TarTable.  Names are bytes in the archive: decoded as UTF-8 with
    surrogateescape, as tarfile does.  type is one byte, as tarfile's; mtime an int, or a float for a pax time with a fraction."""
    L = N.lib()
    try:
        n, nb, end, off = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int(), ctypes.c_uint64()
        L.xlz_tar_info(h, ctypes.byref(n), ctypes.byref(nb), ctypes.byref(end), ctypes.byref(off))
        ents = (N.TarEntry * max(n.value, 1))()
        pool = ctypes.create_string_buffer(max(nb.value, 1))
        st = L.xlz_tar_entries(h, ents, n.value, ctypes.cast(pool, ctypes.c_void_p), nb.value)
        if st != OK:
            raise LzmaError(st, "xlz_tar_entries")
    finally:
        L.xlz_tar_close(h)
    raw = pool.raw
    entries = []
    for i in range(n.value):
        x = ents[i]
        entries.append(TarEntry(raw[x.name_off:x.name_off + x.name_len].decode("utf-8", "surrogateescape"),
                                raw[x.link_off:x.link_off + x.link_len].decode("utf-8", "surrogateescape"), x.size, bytes([x.type]), x.mode,
                                x.uid, x.gid, x.mtime_s + x.mtime_ns * 1e-9 if x.mtime_ns else x.mtime_s, x.hdr_off, x.data_off))
    return TarTable(entries, end.value, off.value)


def tar_parse(image):
    """xlz_tar_parse_host: the members of a .tar image in host memory (bytes) -> TarTable(entries, end_status, end_off): what
    tarfile.getmembers() reports, and how the walk along the headers ended (OK, or the status and the offset of the header
    where it stopped; the members in front of it are listed).  Host only, no device needed."""
    if not isinstance(image, bytes):
        image = bytes(image)
    h = ctypes.c_void_p()
    st = N.lib().xlz_tar_parse_host(ctypes.cast(ctypes.c_char_p(image), ctypes.c_void_p), len(image), ctypes.byref(h))
    if st != OK:
        raise LzmaError(st, "xlz_tar_parse_host")
    return _tar_table(h)


def tar_scan_device(ctx, dptr, n):
    """xlz_tar_scan_device: the same for `n` bytes of device memory at the address `dptr` (a multiple of 16, on the context's
    device): the blocks are classified where they lie, only the flags, the header candidates and the data of long-name /
    pax entries come to the host.  Member i is bytes [data_off, data_off + size) of the image."""
    h = ctypes.c_void_p()
    st = N.lib().xlz_tar_scan_device(ctx._h, ctypes.c_void_p(int(dptr)), int(n), ctypes.byref(h))
    if st != OK:
        raise LzmaError(st, "xlz_tar_scan_device")
    return _tar_table(h)


def xz_tar_tensor(ctx, data, verify=True):
    """a .tar.xz into device memory and its member table: xz_decode_tensor, then tar_scan_device over the tensor ->
    (image, entries, end_status); member i is the view image[e.data_off:e.data_off + e.size]"""
    image = xz_decode_tensor(ctx, data, verify=verify)
    table = tar_scan_device(ctx, image.data_ptr() if image.numel() else 0, image.numel())
    return image, table.entries, table.end_status


class TarXzFile:
    """One .tar.xz: the index of the .xz file (XzFile; host only) and, after list(), its member table.  Members are read
    through the range reader over (data_off, size), so a read decodes only the .xz blocks that hold the wanted members
    -- ONE batch per call.  `data` as for XzFile (borrowed, held until close()).  A context manager; close() may be repeated."""

    def __init__(self, data):
        self.xz = XzFile(data)
        self.entries = self.names = self.end_status = self.end_off = None

    def list(self, ctx, verify=True, strict=True):
        """xlz_xz_tar_list: the whole file decoded into device scratch and scanned there -> the entries; fills .entries,
        .names, .end_status and .end_off.  Raises LzmaError as a read of the whole file does, and -- unless strict is
        False -- when the archive does not end cleanly (.entries then holds the members in front of that place)."""
        h, unverified = ctypes.c_void_p(), ctypes.c_size_t()
        st = N.lib().xlz_xz_tar_list(ctx._h, self.xz._handle(), 1 if verify else 0, ctypes.byref(h), ctypes.byref(unverified))
        if st != OK:
            raise LzmaError(st, "xlz_xz_tar_list")
        ctx.last_xz_unverified = unverified.value
        self.entries, self.end_status, self.end_off = _tar_table(h)
        self.names = [e.name for e in self.entries]
        if strict and self.end_status != OK:
            raise LzmaError(self.end_status, "xlz_xz_tar_list: the archive ends at offset %d" % self.end_off)
        return self.entries

    def index(self, which):
        """a member's index from an index or a name (the LAST member of that name, as tarfile.getmember)"""
        if self.entries is None:
            raise ValueError("TarXzFile.list() has not run")
        if isinstance(which, str):
            for i in range(len(self.names) - 1, -1, -1):
                if self.names[i] == which:
                    return i
            raise KeyError(which)
        return range(len(self.entries))[int(which)]

    def span(self, which):
        """(data_off, n) of a member (index or name): where its bytes lie in the decoded file.  n is 0 for a member without
        data (types '1'-'6': links, directories, devices), whatever its size field says."""
        e = self.entries[self.index(which)]
        return e.data_off, 0 if b"1" <= e.type <= b"6" else e.size

    def read_many(self, ctx, which, verify=True):
        """the bytes of the wanted members (indices or names) -> list[bytes]: ONE batch of the covering .xz blocks
        (ctx.last_xz_read_stats())"""
        return self.xz.read_ranges(ctx, [self.span(w) for w in which], verify=verify)

    def read(self, ctx, which, verify=True):
        return self.read_many(ctx, [which], verify=verify)[0]

    def read_tensor(self, ctx, which, verify=True, out=None):
        """one member into a torch.uint8 tensor on the context's device, as XzFile.read_tensor"""
        off, n = self.span(which)
        return self.xz.read_tensor(ctx, off, n, verify=verify, out=out)

    def close(self):
        self.xz.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---- many .xz files as one batch (include/xlz.h: xlz_xz_many_layout / xlz_xz_decode_many / xlz_xz_decode_many_device) ----
class _ManyFiles:
    """an xlz_xz_many_file array over `datas` (bytes or contiguous buffers: bytearray, memoryview, mmap), every one borrowed
    through the buffer protocol as XzFile borrows its file -- never copied -- and held until release()"""

    def __init__(self, datas, windows=None):
        self.n = len(datas)
        if windows is not None and len(windows) != self.n:
            raise ValueError("one window per file")
        self.arr = (N.XzManyFile * max(self.n, 1))()
        self.res = (N.XzManyResult * max(self.n, 1))()
        self._views = (_PyBuffer * max(self.n, 1))()
        self._held = 0
        try:
            for i, d in enumerate(datas):
                ctypes.pythonapi.PyObject_GetBuffer(ctypes.py_object(d), ctypes.byref(self._views[i]), 0)  # (raises: no buffer, not contiguous)
                self._held = i + 1
                self.arr[i].file, self.arr[i].len = self._views[i].buf, self._views[i].len
                if windows is not None:
                    self.arr[i].dst_off, self.arr[i].dst_cap = int(windows[i][0]), int(windows[i][1])
        except Exception:
            self.release()
            raise

    def layout(self, chains, align):
        total = ctypes.c_uint64()
        st = N.lib().xlz_xz_many_layout(self.arr, self.n, 1 if chains else 0, int(align), self.res, ctypes.byref(total))
        if st != OK:
            raise LzmaError(st, "xlz_xz_many_layout")
        return total.value

    def decode(self, name, ctx, dst, cap, verify):
        st = getattr(N.lib(), name)(ctx._h, self.arr, self.n, dst, int(cap), 1 if verify else 0, self.res)
        if st != OK:
            raise LzmaError(st, name)
        return [(self.res[i].status, self.res[i].out_len, self.res[i].unverified) for i in range(self.n)]

    def release(self):
        for i in range(self._held):
            ctypes.pythonapi.PyBuffer_Release(ctypes.byref(self._views[i]))
        self._held = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()


def _chains_of(chains, ctx):
    return bool(chains) if chains is not None else ctx is not None and ctx.filter_mode() == 1


def xz_many_layout(datas, chains=None, align=1, ctx=None):
    """xlz_xz_many_layout: the windows of many .xz files back to back in one destination, each dst_off a multiple of
    `align` -> ([(dst_off, dst_cap, status)], total); dst_cap is the index's total, 0 for a file whose index is refused
    (status says why).  chains: accept Delta / BCJ filter chains (None: as ctx.filter_mode() says where a ctx is given,
    otherwise no).  Host only.  Raises LzmaError(ERR_OUT_CAP) when the windows do not fit 64 bits."""
    with _ManyFiles(datas) as m:
        total = m.layout(_chains_of(chains, ctx), align)
        return [(m.arr[i].dst_off, m.arr[i].dst_cap, m.res[i].status) for i in range(m.n)], total


def xz_decode_many(ctx, datas, verify=True, max_size=None):
    """xlz_xz_decode_many: many whole .xz files as ONE batch, into one host buffer laid out by xz_many_layout -> a list of
    (bytes or None, status, unverified), one per file: what xz_decode gives for that file alone, except that a bad file is
    its own status here and no exception.  max_size: refuse (ERR_OUT_CAP) a set whose indexes announce more in all.
    Raises LzmaError only for what concerns the whole call."""
    with _ManyFiles(datas) as m:
        total = m.layout(_chains_of(None, ctx), 1)
        if max_size is not None and total > max_size:
            raise LzmaError(ERR_OUT_CAP, "xlz_xz_decode_many: the indexes announce %d bytes, max_size is %d" % (total, max_size))
        out = ctypes.create_string_buffer(max(total, 1))
        res = m.decode("xlz_xz_decode_many", ctx, ctypes.cast(out, ctypes.c_void_p), total, verify)
        base = ctypes.addressof(out)
        return [(ctypes.string_at(base + m.arr[i].dst_off, n) if st == OK else None, st, nu) for i, (st, n, nu) in enumerate(res)]


def xz_decode_many_into(ctx, datas, out, windows, verify=True):
    """xlz_xz_decode_many with the caller's buffer: file i goes to its window (dst_off, dst_cap) = windows[i] of `out` (a
    writable buffer: bytearray, numpy array, ctypes array); windows must not overlap -> [(status, out_len, unverified)]"""
    dst = out if isinstance(out, ctypes.Array) else (ctypes.c_char * memoryview(out).nbytes).from_buffer(out)
    with _ManyFiles(datas, windows) as m:
        return m.decode("xlz_xz_decode_many", ctx, ctypes.cast(dst, ctypes.c_void_p), ctypes.sizeof(dst), verify)


def xz_decode_many_device(ctx, datas, dptr, cap, windows, verify=True):
    """xlz_xz_decode_many_device: the same into `cap` bytes of device memory at the address `dptr` (on the context's device)
    -- ONE batch over the blocks of all files, the filters, the checks and one pack on the device -> [(status, out_len,
    unverified)] as xz_decode_device gives them for each file alone"""
    with _ManyFiles(datas, windows) as m:
        return m.decode("xlz_xz_decode_many_device", ctx, ctypes.c_void_p(int(dptr)), cap, verify)


def xz_decode_many_tensor(ctx, datas, verify=True, align=1, out=None):
    """xz_decode_many_device into a torch.uint8 tensor on the context's device: `out` (one-dimensional, contiguous, at least
    the layout's total; ERR_OUT_CAP if smaller) or a new one -> (tensor, [(off, out_len, status, unverified)]): file i is
    tensor[off:off + out_len] where its status is OK"""
    with _ManyFiles(datas) as m:
        out = _tensor_out(ctx, m.layout(_chains_of(None, ctx), align), out, "the indexes announce")
        res = m.decode("xlz_xz_decode_many_device", ctx, ctypes.c_void_p(out.data_ptr()), out.numel(), verify)
        return out, [(m.arr[i].dst_off, n, st, nu) for i, (st, n, nu) in enumerate(res)]
