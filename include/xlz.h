/*
 * xlz.h -- C ABI of the MI355X-native batched LZMA / LZMA2 decoder (libxlz.so).
 *
 * This is the drop-in boundary for the hot path of kulaginds/lzma:
 * (*Reader1).decompress (decompress.go:8-1136) and everything it drives
 * (window.go, state.go, range_decoder.go), plus the LZMA2 chunk framing of
 * reader2.go:100-298.  The reference is pure Go with no FFI; the entry points
 * below are what a cgo binding for that path binds (see INTEGRATION.md for the
 * Go side).  Plain pointers and sizes only; no C++ or torch types.
 *
 * All compute runs in hand-written HIP kernels on gfx950.  There is NO CPU
 * decode path in this library: without a usable HIP device every decode entry
 * point fails with XLZ_ERR_DEVICE.
 *
 * The library reads ONE environment variable, a debugging aid: XLZ_DEBUG (any
 * value) prints failed HIP calls and the phase times of xlz_decode_batch to
 * stderr.  Nothing tunes the decode.  (An A/B build made with -DXLZ_DEV_KNOBS also reads
 * XLZ_STORED_UNIT_KIB, the least size of a unit of stored LZMA2 chunks; the shipped build
 * does not contain that code.)
 *
 * file:line citations are into the reference repository.
 */
#ifndef XLZ_H
#define XLZ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XLZ_VERSION_MAJOR 0
#define XLZ_VERSION_MINOR 1

/* ---- per-stream status -------------------------------------------------- */
/* >= 0: the reference's reader would have ended with io.EOF (no error).
 *  < 0: the reference's constructor or Read would have returned an error.   */
enum {
    XLZ_OK = 0,                  /* clean end: size reached with Code==0, or end marker
                                    (decompress.go:14-20,633-641)                               */
    XLZ_OK_INPUT_EOF = 1,        /* input exhausted; the reference turns ReadByte's io.EOF into a
                                    normal end of stream (decompress.go:35-38, reader1.go:246)  */
    XLZ_ERR_RESULT = -1,         /* ErrResultError (errors.go:8)                                 */
    XLZ_ERR_PROPS = -2,          /* ErrIncorrectProperties (reader1.go:211-213)                  */
    XLZ_ERR_HEADER_EOF = -3,     /* constructor error: input ended inside the 13-byte header or
                                    the 5 range-coder init bytes (reader1.go:78-98,153-156)     */
    XLZ_ERR_RC_INIT = -4,        /* first range-coder byte != 0 (range_decoder.go:32-34)         */
    XLZ_ERR_UNEXPECTED_EOF = -5, /* io.ErrUnexpectedEOF from LZMA2 framing (reader2.go:104-127)  */
    XLZ_ERR_OUT_CAP = -6,        /* new: out_cap smaller than the decoded size (the reference has no
                                    output limit); out_len==out_cap, in_consumed = the input read
                                    when the packet / stored chunk that did not fit was complete   */
    XLZ_ERR_BAD_ARG = -7,        /* new: NULL pointer / unknown format                           */
    XLZ_ERR_DEVICE = -8,         /* new: HIP runtime failure or no gfx950 device                 */
    XLZ_ERR_UNSUPPORTED = -9,    /* new: stream outside what the GPU path implements (DESIGN.md
                                    section 5.2: a dictionary > 2 GiB on a stream >= 4 GiB; a unit
                                    >= 4 GiB of a device-resident xlz_batch; container features) */
    XLZ_ERR_CLOSED = -10,        /* errAlreadyClosed (readcloser.go:14)                          */
    XLZ_ERR_NEED_ONE_READER = -11, /* errNeedOneReader (reader1.go:26)                           */
    XLZ_ERR_INSUFFICIENT_PROPS = -12 /* errInsufficientProperties (reader2.go:43)                */
};

/* ---- stream formats ------------------------------------------------------ */
enum {
    XLZ_FMT_LZMA_ALONE = 0, /* NewReader1: 13-byte header in-band (reader1.go:18-24,77-101)       */
    XLZ_FMT_LZMA_RAW = 1,   /* NewLZMADecompressorForSevenZip: props byte, dict size and unpack
                               size out of band (reader1.go:32-61)                               */
    XLZ_FMT_LZMA2_RAW = 2   /* NewReader2(in, dictSize) (reader2.go:26-41)                        */
};

typedef struct xlz_stream_desc {
    const uint8_t *in;    /* compressed bytes (host memory)                                       */
    size_t in_len;
    uint8_t *out;         /* host destination; may be NULL for device-resident batches            */
    size_t out_cap;       /* capacity reserved for this stream's output                           */
    uint32_t format;      /* XLZ_FMT_*                                                            */
    uint32_t dict_size;   /* LZMA_RAW: value of DecodeDictSize(props[1:5]); LZMA2_RAW: dictSize
                             argument of NewReader2 (values < 4096 mean 8 MiB, reader2.go:88-91)  */
    uint64_t unpack_size; /* LZMA_RAW only; all-ones = unknown (state.go:135-151)                 */
    uint8_t props;        /* LZMA_RAW only: the lc/lp/pb byte                                     */
    uint8_t flags;        /* XLZ_STREAM_F_* (0 for an ordinary stream); any other bit, or the slice flag
                             on a format that has no slices: XLZ_ERR_BAD_ARG for the call           */
    uint8_t reserved[6];  /* must be zero (memset the descriptor): XLZ_ERR_BAD_ARG otherwise        */
} xlz_stream_desc;

/* LZMA2_RAW: `in` is a SLICE of a longer stream that does not begin at the stream's start -- it begins
 * where a unit of xlz_lzma2_units begins (callers that deal the units of one stream to several GPUs or
 * processes: xlz_decode_batch_multi does it by itself).  Bytes in front of the slice's first
 * dictionary epoch belong to units that are not in this call: a (malformed) stream that reads them,
 * or whose units do not decode to what their headers announce, ends in XLZ_ERR_UNSUPPORTED instead
 * of being settled inside the slice -- decode the whole stream then.  A slice that ends before its
 * stream does (no end byte) ends in XLZ_ERR_UNEXPECTED_EOF with all of its input consumed: that is
 * its clean outcome.                                                                              */
#define XLZ_STREAM_F_LZMA2_SLICE 1u

typedef struct xlz_result {
    uint64_t out_len;     /* bytes produced by the decoder (even when status < 0)                 */
    uint64_t in_consumed; /* input bytes pulled from the source, header included                  */
    int32_t status;       /* XLZ_OK ... */
    int32_t reserved;
} xlz_result;

/* ---- library ------------------------------------------------------------- */
const char *xlz_version(void);
const char *xlz_build_id(void);       /* hash of the sources this binary was compiled from (lzma_amd/build.py);
                                         measurements quote it so that a number names the kernel that ran   */
const char *xlz_kernel_id(void);      /* the same over the device code's sources only: what rocprof profiles are tied to   */
const char *xlz_strerror(int status); /* text of the matching reference error (errors.go:5-12)    */
int xlz_device_count(void);           /* number of HIP devices, 0 if none                         */

/* helpers with the reference's exported names */
int xlz_decode_prop(uint8_t d, uint8_t *lc, uint8_t *pb, uint8_t *lp); /* DecodeProp reader1.go:210 */
uint32_t xlz_decode_dict_size(const uint8_t properties[4]);            /* DecodeDictSize   :193    */
uint32_t xlz_decode_dict_size2(uint8_t encoded);                       /* DecodeDictSize2 reader2.go:296 */
uint64_t xlz_decode_unpack_size(const uint8_t header[8]);              /* DecodeUnpackSize :178    */

/* ---- context: one per (host thread, GPU) ---------------------------------- */
typedef struct xlz_ctx xlz_ctx;
int xlz_ctx_create(int device, xlz_ctx **ctx); /* XLZ_OK or XLZ_ERR_DEVICE                         */
void xlz_ctx_destroy(xlz_ctx *ctx);
int xlz_ctx_device(const xlz_ctx *ctx);

/* HIP events on the context's stream, for callers that time a region of enqueued work
 * (bench.py): slot 0..63.  elapsed_ms waits for event `b`.                           */
int xlz_ctx_event_record(xlz_ctx *ctx, int slot);
int xlz_ctx_event_elapsed_ms(xlz_ctx *ctx, int slot_a, int slot_b, float *ms);

/* Coalescing of pull-style readers.  The reference's readers are
 * independent single-goroutine objects; many goroutines each doing io.Copy(dst, NewReader1(src))
 * would each occupy one wave of the GPU with a launch of its own.  After this call, every refill
 * of a reader of `ctx` is handed to a background thread that waits up to `window_us` for refills
 * of other readers (at most `max_streams`) and runs them as ONE launch; xlz_reader_read blocks
 * until its refill is done.                                                                      */
int xlz_ctx_enable_batching(xlz_ctx *ctx, uint32_t window_us, uint32_t max_streams);
int xlz_ctx_batching_stats(xlz_ctx *ctx, uint64_t *batches, uint64_t *streams);

/* ---- one-shot batch decode: host buffers in, host buffers out -------------- */
/* Replaces a loop of `r, _ := NewReader1(src); io.Copy(dst, r)` over n independent
 * streams (reader1_test.go:76-80).  One bad stream never fails the batch: the return
 * value is XLZ_OK unless the call itself could not run; per-stream outcomes are in
 * results[i].  Thread-safe across contexts; calls on one context are serialised.
 * A call of several wave rounds (>= 8192 streams and >= 1 GiB of output) is cut into up
 * to ten sub-batches whose upload, decode and download overlap; a call of ONE wave round (and
 * at least 256 MiB of output) runs as up to eight launches whose downloads overlap the decode
 * (xlz_call_stats.slices, xlz_ctx_set_slicing).  Bytes of `out` beyond out_len are unspecified.
 * BREAK-EVEN: one wave decodes one unit (a stream; an LZMA2 dictionary-reset unit) at
 * 4-6 MB/s and the chip holds 4096 of them (up to 6144 on calls of many rounds), so a call with few units is slower than the
 * host's own cores: measured on 1 MiB text streams, 64 units 0.34 GiB/s (16 host cores:
 * 1.27), 256 units 1.37 (1.28), 1024 units 5.2, 4096 units 17.2.  Below about 250 units
 * per 16 host cores decode on the CPU, or gather more streams first;
 * xlz_batch_advice answers that question for a given call before anything is uploaded.  */
int xlz_decode_batch(xlz_ctx *ctx, const xlz_stream_desc *streams, size_t n, xlz_result *results);
/* Host only (no device needed; only out_cap of every stream is looked at): how xlz_decode_batch would cut this call into
 * pieces.  cuts[k] = index of the first stream of piece k, one entry more than there are pieces (the last is n); *n_cuts =
 * entries (XLZ_ERR_OUT_CAP if max_cuts is smaller; cuts may be NULL with max_cuts = 0 to ask for the count); *mode (may be
 * NULL): 0 one piece (a call of one wave round overlaps its copies with its own decode: slices), 1 a pipeline of pieces
 * whose launches overlap on two streams (many short streams), 2 pieces of exactly one wave round of 4096 streams, one
 * behind the other, each sliced (few rounds of long streams: 256 KiB and more on average).                          */
int xlz_decode_batch_plan(const xlz_stream_desc *streams, size_t n, size_t *cuts, size_t max_cuts, size_t *n_cuts, int *mode);

/* BEFORE uploading anything: how much of a GPU would this call fill, and is the host the faster
 * decoder for it?  Host only (reads stream and LZMA2 chunk headers; no device needed; `ctx` may be
 * NULL: an MI355X's 4096 wave slots are assumed).  Two estimated times are compared, in compressed
 * bytes of serial work (decode time tracks them):
 *   GPU: one wave decodes one unit -- an LZMA1 stream, or one unit of an LZMA2 stream's plan
 *        (xlz_lzma2_units) -- and `wave_slots` units run at once:
 *        gpu_cost = max(largest unit, all bytes / wave_slots);
 *   CPU: a host core decodes about 16 times as fast as a wave (65-80 MB/s of output against 4-6), but
 *        ONE stream is ONE thread whatever its format -- the reference's Reader2 is one goroutine
 *        (reader2.go:216-250), the units of an LZMA2 stream are parallel work for the GPU only:
 *        cpu_cost = max(largest stream, all bytes / host_threads) / 16.
 * prefer_cpu = cpu_cost < gpu_cost.  For equal LZMA1 streams that is "fewer than 16 units per host
 * thread" (break_even_units; bench.py: stream_count_sweep, 256 units for 16 threads); one LZMA2 stream
 * of 100 units is the GPU's job on any host, 64 big LZMA1 streams are the host's.  `host_threads` = 0:
 * the hardware concurrency of this machine.  The library has no CPU decoder: a caller that is told
 * prefer_cpu = 1 decodes with the reference's own readers (reader1.go:18-24, reader2.go:26-41; the Go
 * shim does that by itself) or gathers more streams. */
typedef struct xlz_advice {
    uint64_t units;            /* independent work units the call would launch                    */
    uint64_t in_bytes;         /* compressed bytes of all streams                                  */
    uint32_t wave_slots;       /* units a GPU decodes at once (resident single-wave workgroups)    */
    uint32_t break_even_units; /* 16 x host_threads: the break-even for EQUAL LZMA1 streams         */
    double   fill;             /* min(1, units / wave_slots): the share of the chip the call uses  */
    int32_t  prefer_cpu;       /* 1: cpu_cost < gpu_cost (or nothing to decode)                    */
    uint32_t reserved;
    double   cpu_cost;         /* estimated serial work per host thread, in wave-equivalent bytes  */
    double   gpu_cost;         /* estimated serial work per wave slot, in compressed bytes         */
} xlz_advice;
int xlz_batch_advice(const xlz_ctx *ctx, const xlz_stream_desc *streams, size_t n, uint32_t host_threads,
                     xlz_advice *out);

/* What the most recent successful xlz_decode_batch on `ctx` spent where, and how well it filled the GPU.
 * ONE wave decodes one stream (LZMA1 has no parallelism inside a stream: decompress.go:13 is a serial
 * chain), at about 5 MB/s of output; the chip holds `wave_slots` (4096) of them.  A call with few
 * streams leaves most of the chip idle -- slot_occupancy says how much of it worked -- and below the
 * break-even stated in INTEGRATION.md the host's own cores are faster.                              */
typedef struct xlz_call_stats {
    double upload_ms;      /* parse headers, pack the inputs into pinned memory, host -> device     */
    double decode_ms;      /* decode launch(es) until the per-stream results are on the host        */
    double download_ms;    /* device -> host and scatter into the callers' buffers                  */
    double total_ms;
    double kernel_span_ms; /* first wave's start to last wave's end over all launches of the call (device clock) */
    double slot_occupancy; /* busy wave time / (wave_slots x kernel span): 1.0 = every slot busy throughout */
    uint64_t streams;      /* n of the call                                                          */
    uint64_t units;        /* work units of the main launch (streams; LZMA2: dictionary-reset units and
                              256 KiB pieces of runs of stored chunks)                               */
    uint32_t wave_slots;   /* resident single-wave workgroups of the launch                          */
    uint32_t sub_batches;  /* > 1: the call ran as a pipeline (upload k+1 / decode k / download k-1); then
                              upload_ms = until the first sub-batch was on the device, decode_ms = first
                              launch to last results, download_ms = what was left after that            */
    uint32_t slices;       /* > 1: a call of ONE wave round -- or every one-round piece of a call of few rounds
                              of long streams (sub_batches > 1) -- ran as a sequence of that many launches, each
                              advancing every unit by a share of its output, the download of share k-1 under
                              the decode of share k (the reference's Read pump in batch form,
                              reader1.go:223-254); for a call of one piece decode_ms = the launches (HIP
                              events), download_ms = what was left after them; slot_occupancy = the mean over
                              the launches                                                                */
    uint32_t refetched;    /* streams of a sliced call downloaded once more after their slices had gone out: a unit
                              fell short of a launch's bound, a re-run wrote bytes again, or a model beyond LDS
                              decoded behind the slices (summed over the sub-batches)                       */
} xlz_call_stats;
int xlz_ctx_last_call_stats(xlz_ctx *ctx, xlz_call_stats *out);
/* xlz_decode_batch keeps the device and pinned memory of its (sub-)batches in the context between calls (a
 * call of the same shape finds its blocks again; what two calls in a row did not use is released by
 * itself).  xlz_ctx_trim releases all of it now; *released (may be NULL) = the bytes given back.      */
int xlz_ctx_trim(xlz_ctx *ctx, uint64_t *released);
/* Tuning of xlz_decode_batch's sliced form (xlz_call_stats.slices): a call of one wave round with at least
 * min_call_bytes of output room runs as one launch for every slice_bytes of it, at most max_slices (<= 63; from
 * four on the last share is cut in two -- its download is the one nothing overlaps --: one launch more).
 * 0 = the default of that argument (256 MiB, 128 MiB, 8); max_slices = 1 turns slicing off.  The decoded
 * bytes, statuses and consumed input do not depend on it.  The reference's counterpart is the size of the
 * buffer its caller hands to Read (reader1.go:223-254: decompress(need) runs until `need` bytes are pending). */
int xlz_ctx_set_slicing(xlz_ctx *ctx, uint64_t min_call_bytes, uint64_t slice_bytes, uint32_t max_slices);

/* ---- device-resident batch: upload once, decode many times ---------------- */
typedef struct xlz_batch xlz_batch;
/* Parses headers / LZMA2 framing on the host, uploads the compressed bytes and
 * allocates the output arena in HBM.  streams[i].out may be NULL.                 */
int xlz_batch_create(xlz_ctx *ctx, const xlz_stream_desc *streams, size_t n, xlz_batch **batch);
int xlz_batch_run(xlz_batch *batch);  /* enqueue one full decode pass on the context's stream     */
int xlz_batch_sync(xlz_batch *batch); /* wait for everything enqueued so far                      */
int xlz_batch_results(xlz_batch *batch, xlz_result *results); /* sync + fetch per-stream results  */
int xlz_batch_download(xlz_batch *batch, size_t i, uint8_t *dst, size_t cap); /* copy out stream i */
int xlz_batch_device_output(xlz_batch *batch, size_t i, void **dptr, size_t *cap);
/* HIP-event time of the decode kernel(s) of the most recent completed run, in ms */
int xlz_batch_last_kernel_ms(xlz_batch *batch, float *ms);
/* algorithmic bytes (compressed in + decoded out) the last run moved, and units  */
int xlz_batch_stats(xlz_batch *batch, uint64_t *in_bytes, uint64_t *out_bytes, uint64_t *units);
/* When each unit of the last run started and ended on its wave, in ticks of the device's 100 MHz
 * clock since the first unit started, and its compressed size (the work-queue key).  Arrays of
 * `cap` entries (any may be NULL); *n_units = units of the batch.  For slot-occupancy / tail
 * analysis of the persistent grid (bench.py: roofline.issue.slot_occupancy).                */
int xlz_batch_unit_trace(xlz_batch *batch, uint32_t *t_start, uint32_t *t_end, uint32_t *in_len,
                         size_t cap, size_t *n_units);
/* shape of the decode launch: resident single-wave workgroups (= wave slots) and LDS bytes each */
int xlz_batch_launch_info(xlz_batch *batch, uint32_t *workgroups, uint32_t *lds_bytes);
/* which kernel the batch's main launch is (profiles are matched by it): "xlz::xlz_decode_kernel" -- the model laid out
 * with room for 16 posStates (pb <= 4) --, "xlz::xlz_decode_kernel_pb2" -- room for 4: every unit's pb <= 2, the
 * default of liblzma and 7-Zip; five LDS granules instead of six for lc+lp = 3, 24 workgroups per CU instead of 21 --
 * or "xlz::xlz_decode_kernel_hbm_model" (only models beyond LDS, lc+lp > 8)                                          */
const char *xlz_batch_kernel_name(xlz_batch *batch);
void xlz_batch_destroy(xlz_batch *batch);

/* ---- integrity checks on the device ----------------------------------------------------------
 * Outside the reference (which has no checks).  CRC32 (IEEE 802.3, reflected 0xEDB88320: .xz check 1, .7z) and CRC64
 * (.xz check 4, reflected 0xC96C5795D7870F42) of RANGES of the decoded output, computed by HIP kernels on the bytes where
 * the decode left them in HBM (lzma_amd/csrc/xlz_check_dev.hip): a caller that keeps the output on
 * the GPU verifies it without downloading it, and a host-to-host call gets its digests before its arenas go back to the
 * pool.  A range's digest covers [off, off + len) of its stream's output cut to [0, out_len) -- what the decoder produced
 * of it; an empty intersection gives 0, the CRC of no bytes.  Digests are the published CRCs (what zlib.crc32 and liblzma
 * give), CRC32 zero-extended to 64 bits.                                                              */
enum { XLZ_CHECK_NONE = 0, XLZ_CHECK_CRC32 = 1, XLZ_CHECK_CRC64 = 4, XLZ_CHECK_SHA256 = 10 }; /* the .xz check ids */
typedef struct xlz_check_range {
    uint64_t stream;   /* index into the call's / the batch's streams; >= n: XLZ_ERR_BAD_ARG for the call */
    uint64_t off, len; /* bytes of THAT STREAM'S OUTPUT                                               */
    uint32_t kind;     /* XLZ_CHECK_CRC32 / XLZ_CHECK_CRC64 (the _digests calls: XLZ_CHECK_SHA256 too), else
                          XLZ_ERR_BAD_ARG                                                            */
    uint32_t reserved; /* 0, else XLZ_ERR_BAD_ARG                                                      */
} xlz_check_range;
/* Device-resident: waits for and collects the latest run like xlz_batch_results, runs the check kernels on the batch's
 * stream and fetches the n digests; nothing else leaves the device.  Ranges may overlap and come in any order.      */
int xlz_batch_checks(xlz_batch *batch, const xlz_check_range *ranges, size_t n, uint64_t *digests);
/* xlz_decode_batch plus the digests of n_ranges ranges, computed on the device behind every (sub-)batch's results, in all
 * three forms of the pipeline (xlz_decode_batch_plan).  Streams that never sit in an arena (4 GiB and more; streams that
 * failed on the host) get theirs from the host's code over the caller's buffer (xlz_check_stats.host_ranges).        */
int xlz_decode_batch_checked(xlz_ctx *ctx, const xlz_stream_desc *streams, size_t n, xlz_result *results,
                             const xlz_check_range *ranges, size_t n_ranges, uint64_t *digests);
/* crc(A || B) from crc(A), crc(B) and the length of B: host only, no device needed.  What folds the digests of the slices
 * of one stream that were checked apart (several GPUs, several calls).                                   */
uint32_t xlz_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);
uint64_t xlz_crc64_combine(uint64_t crc_a, uint64_t crc_b, uint64_t len_b);
/* Where xlz_xz_decode / xlz_7z_decode verify.  0 (default): on host threads after the call's download, as ever.  1: every
 * CRC32 / CRC64 block, folder and file (per-file ranges inside solid folders) through xlz_decode_batch_checked, digests
 * compared on the host; SHA-256 blocks, reserved check types and .7z Copy folders (never on the device) stay on the host.
 * 2: mode 1, and the SHA-256 blocks of an .xz file through xlz_decode_batch_digests: the device hashes the blocks that
 * xlz_sha256_plan gives it, the host threads the others (a .7z archive has no SHA-256: there 2 is 1).
 * Bytes, status and *unverified are the same in all modes.  xlz_xz_decode_multi / xlz_7z_decode_multi ignore the mode:
 * they check on the host.  Any other value: XLZ_ERR_BAD_ARG.                                              */
int xlz_ctx_set_check_mode(xlz_ctx *ctx, int mode);
int xlz_ctx_check_mode(const xlz_ctx *ctx);
/* Of the most recent xlz_batch_checks / xlz_decode_batch_checked on `ctx`, or of the most recent xlz_xz_decode /
 * xlz_7z_decode in check mode 1 (summed over the batches it made): who checked what.                      */
typedef struct xlz_check_stats {
    uint64_t device_ranges; /* ranges whose bytes the check kernels read ...                              */
    uint64_t device_bytes;  /* ... and how many bytes that was                                             */
    uint64_t host_ranges;   /* ranges the host's code checked (streams outside the arenas; the front-ends' SHA-256
                               blocks and Copy folders)                                                     */
    uint64_t host_bytes;
    uint64_t empty_ranges;  /* ranges with nothing to check: no byte of them was produced                  */
    double kernel_ms;       /* the check kernels by HIP events, summed over the launches                   */
    uint32_t launches;      /* (sub-)batches that ran check kernels                                        */
    uint32_t reserved;
} xlz_check_stats;
int xlz_ctx_last_check_stats(xlz_ctx *ctx, xlz_check_stats *out);

/* ---- filters on the device ------------------------------------------------------------------
 * Outside the reference (which has no filters).  The filters an .xz block or a .7z folder may put in front of its LZMA
 * coder -- Delta and the BCJ branch converters -- undone by HIP kernels on the decoded bytes where they lie in HBM
 * (lzma_amd/csrc/xlz_filter_dev.hip), before any check reads them and before they are downloaded.
 * A STEP transforms [0, out_len) of one stream in place.  The steps of one stream are applied in array order to the decoded
 * bytes -- the reverse of the order a block header lists its chain in --, at most three per stream; steps of different
 * streams are independent: a launch takes one step of every stream that still has one.  ARM64 (0x0A), RISC-V (0x0B) and
 * BCJ2 are not implemented.                                                                          */
enum { XLZ_FILTER_DELTA = 3, XLZ_FILTER_X86 = 4, XLZ_FILTER_POWERPC = 5, XLZ_FILTER_IA64 = 6,
       XLZ_FILTER_ARM = 7, XLZ_FILTER_ARMTHUMB = 8, XLZ_FILTER_SPARC = 9 };   /* the .xz filter ids */
typedef struct xlz_filter_step {
    uint64_t stream;   /* index into the call's / the batch's streams */
    uint32_t id;       /* XLZ_FILTER_* */
    uint32_t param;    /* Delta: distance 1..256; BCJ: start offset (a multiple of the filter's alignment) */
    uint32_t reserved[2];
} xlz_filter_step;
/* XLZ_ERR_BAD_ARG (all entry points): an unknown id, a distance outside 1..256, a start offset that is not a multiple of
 * the filter's alignment (x86 1, ARM-Thumb 2, ARM / PowerPC / SPARC 4, IA-64 16), non-zero reserved words, a stream index
 * >= n, more than three steps for one stream.                                                         */
/* One step over a host buffer: host only, no device needed (the serial form of what the kernels do).  What filters streams
 * that never sit in an arena, and what a caller uses on bytes it decoded elsewhere.                   */
int xlz_filter_host(uint32_t id, uint32_t param, uint8_t *buf, size_t len);
/* Device-resident: waits for and collects the latest run like xlz_batch_checks and filters in place on the batch's stream.
 * Afterwards xlz_batch_download, xlz_batch_device_output and xlz_batch_checks see the filtered bytes; a later
 * xlz_batch_run decodes afresh.                                                                       */
int xlz_batch_filter(xlz_batch *batch, const xlz_filter_step *steps, size_t n);
/* xlz_decode_batch_checked with the filter between decode and check: digests are over the FILTERED bytes, which is what
 * an .xz check and a .7z CRC cover.  With n_steps = 0 it is xlz_decode_batch_checked.  A (sub-)batch that has steps does
 * not run sliced (xlz_call_stats.slices <= 1 for a call of one piece): a sliced call ships every slice's bytes while the
 * next slice decodes, before a filter could see them; the pipelined forms hide piece k's filter and check under piece
 * k + 1's decode as they are.  Streams of 4 GiB and more are filtered on the host over the caller's buffer
 * (xlz_filter_stats.host_steps).  A stream with XLZ_STREAM_F_LZMA2_SLICE and a step: XLZ_ERR_BAD_ARG.  On a machine
 * without a HIP device (no context can exist: ctx == NULL) the call returns XLZ_ERR_DEVICE: xlz_filter_host is no decoder. */
int xlz_decode_batch_filtered(xlz_ctx *ctx, const xlz_stream_desc *streams, size_t n, xlz_result *results,
                              const xlz_filter_step *steps, size_t n_steps, const xlz_check_range *ranges, size_t n_ranges,
                              uint64_t *digests);
/* What xlz_xz_decode / xlz_7z_decode do with filter chains.  0 (default): they refuse them (XLZ_ERR_UNSUPPORTED), as ever.
 * 1: they decode chains of one to three of the filters above in front of the LZMA coder.  The _multi forms ignore the
 * mode.  Any other value: XLZ_ERR_BAD_ARG.                                                            */
int xlz_ctx_set_filter_mode(xlz_ctx *ctx, int mode);
int xlz_ctx_filter_mode(const xlz_ctx *ctx);
/* Of the most recent xlz_batch_filter / xlz_decode_batch_filtered (with steps) on `ctx`, or of the most recent
 * xlz_xz_decode / xlz_7z_decode in filter mode 1 (summed over the batches it made): what ran where.      */
typedef struct xlz_filter_stats {
    uint64_t device_steps; /* steps the kernels ran ...                                                  */
    uint64_t device_bytes; /* ... and the bytes they covered (a stream of two steps counts twice)         */
    uint64_t host_steps;   /* steps the host's code ran (streams outside the arenas)                      */
    uint64_t host_bytes;
    uint64_t empty_steps;  /* steps of streams that produced no byte                                      */
    double kernel_ms;      /* the filter kernels by HIP events, summed over the (sub-)batches             */
    uint32_t launches;     /* kernels queued (BCJ 1, x86 2, Delta 4 per round of steps)                   */
    uint32_t reserved;
} xlz_filter_stats;
int xlz_ctx_last_filter_stats(xlz_ctx *ctx, xlz_filter_stats *out);

/* ---- SHA-256 on the device --------------------------------------------------------------------
 * The third .xz check (id 10, what xz --check=sha256 writes), by a HIP kernel that gives every range a lane of its own:
 * one SHA-256 is a serial chain, a batch has hundreds to tens of thousands of them (lzma_amd/csrc/xlz_sha256_dev.hip;
 * DESIGN.md section 3.12).  The calls below are xlz_batch_checks / xlz_decode_batch_filtered with a digest format that
 * holds 32 bytes and with kind XLZ_CHECK_SHA256 allowed, kinds mixed freely; the older calls keep refusing it.
 *   CRC32 / CRC64: the published value little-endian in b[0..7], the rest 0.
 *   SHA-256: the 32 bytes in FIPS 180-4 order, as an .xz block stores them; of an empty intersection, the SHA-256 of no
 *   bytes (counted as empty_ranges).
 * A lane is slow (tens of MB/s), a launch of thousands of ranges is fast: xlz_sha256_plan decides per call which SHA-256
 * ranges the device takes; the others -- and the ranges of streams outside the arenas -- are hashed by host threads, over
 * bytes downloaded for it (xlz_batch_digests) or over the caller's buffer (xlz_decode_batch_digests): host_ranges.     */
typedef struct xlz_digest {
    uint8_t b[32];
} xlz_digest;
int xlz_batch_digests(xlz_batch *batch, const xlz_check_range *ranges, size_t n, xlz_digest *out);
int xlz_decode_batch_digests(xlz_ctx *ctx, const xlz_stream_desc *streams, size_t n, xlz_result *results,
                             const xlz_filter_step *steps, size_t n_steps, const xlz_check_range *ranges, size_t n_ranges,
                             xlz_digest *out);
/* Host only, no device needed: which of n ranges of lens[] bytes the device should hash (on_device[i] = 1) and which the
 * host (0).  The device's time is its longest range over the lane rate, times the rounds of lanes that run side by side;
 * the host's is its bytes over host_threads x rate; ranges longer than a threshold go to the host, and the threshold is
 * the one that minimises the larger time.  No range that would keep a launch busy for more than 0.5 s at the built-in
 * lane rate is ever the device's.  host_threads 0: 16; a rate of 0: the built-in one (lzma_amd/csrc/xlz_sha256_dev.h says
 * whether it is measured or still the instruction-count estimate).  NULL lens or on_device with n > 0: XLZ_ERR_BAD_ARG. */
int xlz_sha256_plan(const uint64_t *lens, size_t n, uint32_t host_threads, double lane_bytes_per_s,
                    double host_bytes_per_s_per_thread, uint8_t *on_device);
/* Of the SHA-256 ranges of the most recent xlz_batch_digests / xlz_decode_batch_digests on `ctx`, or of the most recent
 * xlz_xz_decode in check mode 2.  (xlz_check_stats counts them too, in its device / host / empty fields.)         */
typedef struct xlz_sha256_stats {
    uint64_t device_ranges, device_bytes; /* hashed by the kernel                                          */
    uint64_t host_ranges, host_bytes;     /* hashed by host threads: the plan's choice, or streams outside the arenas */
    uint64_t empty_ranges;
    uint64_t threshold;  /* the longest range the plan gave the device (the largest over the launches; 0: none) */
    double kernel_ms;    /* the kernel by HIP events, summed over the launches                            */
    uint32_t launches;
    uint32_t reserved;
} xlz_sha256_stats;
int xlz_ctx_last_sha256_stats(xlz_ctx *ctx, xlz_sha256_stats *out);

/* ---- pack into device memory (lzma_amd/csrc/xlz_pack_dev.hip) -------
 * The output arena keeps every stream in a region of its own, so a decoded file is never contiguous in HBM.  The pack
 * copies ranges of the decoded (and, behind xlz_batch_filter, filtered) outputs of a batch into ONE caller-owned device
 * buffer, on the device: nothing leaves HBM.  Like xlz_batch_checks it waits for and collects the batch's latest run.
 * An item is clipped to what its stream produced, as a check range is; copied[i] (copied may be NULL) = the bytes written
 * for item i, 0 for a stream that never sat in the arena.  Bytes of the destination that no item covers are not written.
 * The call returns when its stream has drained; no other stream may use d_dst meanwhile.  XLZ_ERR_BAD_ARG: NULL
 * arguments with n > 0; a stream index >= the batch's streams; d_dst is not device memory of the context's device, or
 * dst_cap reaches past its allocation; an item's [dst_off, dst_off + len) does not fit in dst_cap (or the sum
 * overflows); the declared destination ranges of two items overlap.  Nothing is written then.                    */
typedef struct xlz_pack_item {
    uint64_t stream;   /* index into the batch's streams                                                     */
    uint64_t off, len; /* bytes of THAT STREAM'S OUTPUT, clipped to what it produced                         */
    uint64_t dst_off;  /* where they go in the destination                                                   */
} xlz_pack_item;
int xlz_batch_pack(xlz_batch *batch, const xlz_pack_item *items, size_t n, void *d_dst, size_t dst_cap, uint64_t *copied);
/* Of the most recent xlz_batch_pack on `ctx`, or of the pack of the most recent xlz_xz_decode_device /
 * xlz_7z_decode_device.                                                                                           */
typedef struct xlz_pack_stats {
    uint64_t items, bytes;    /* what the kernel copied                                                      */
    uint64_t congruent_items; /* ... of them: source and destination addresses congruent modulo 16 (one load per store) */
    uint64_t empty_items;     /* clipped to nothing: they never reach the kernel                             */
    double kernel_ms;         /* the kernel by HIP events                                                    */
    uint32_t launches;
    uint32_t reserved;
} xlz_pack_stats;
int xlz_ctx_last_pack_stats(xlz_ctx *ctx, xlz_pack_stats *out);

/* ---- BCJ2 folders of .7z archives (lzma_amd/csrc/xlz_bcj2_dev.hip) ----
 * Outside the reference.  BCJ2 (method 03 03 01 1B) is what 7-Zip puts in front of LZMA for x86 executables.  It is no
 * in-place filter: a folder is THREE compressed streams -- main, call, jump -- and a raw range-coder stream, and a serial
 * merge interleaves them into an output longer than the main stream (the statement of the format is at the head of
 * lzma_amd/csrc/xlz_bcj2_dev.h).  The merge is a stage of its own between decode and check, with a destination of its own:
 * one wave per folder, only the decisions serial.                                                       */
/* The serial merge over host buffers: host only, no device needed.  XLZ_OK: out holds out_len bytes.  XLZ_ERR_RESULT: the
 * streams do not fill out_len, or a call / jump / rc stream ran out (no stream is read past its end; the contents of out
 * are unspecified then).  Input left over is ignored.  XLZ_ERR_BAD_ARG: a NULL pointer with a length behind it.   */
int xlz_bcj2_host(const uint8_t *main_s, size_t main_len, const uint8_t *call_s, size_t call_len, const uint8_t *jump_s,
                  size_t jump_len, const uint8_t *rc_s, size_t rc_len, uint8_t *out, size_t out_len);
#define XLZ_BCJ2_RAW (~(uint64_t)0)
typedef struct xlz_bcj2_src { /* one of main / call / jump: the output of a stream of the batch, or bytes of the caller's */
    uint64_t stream;    /* index into the batch's streams -- its length is what that stream PRODUCED --, or XLZ_BCJ2_RAW */
    const uint8_t *raw; /* XLZ_BCJ2_RAW: host memory, uploaded by the call                                       */
    uint64_t raw_len;
} xlz_bcj2_src;
typedef struct xlz_bcj2_item {
    xlz_bcj2_src main_s, call_s, jump_s;
    const uint8_t *rc;  /* the range-coder stream: always raw                                                    */
    uint64_t rc_len;
    uint64_t out_len;   /* the folder's size                                                                     */
    uint64_t dst_off;   /* where it goes in the destination                                                      */
} xlz_bcj2_item;
typedef struct xlz_bcj2_result {
    uint64_t produced;  /* out_len for XLZ_OK, else 0 (the item's destination range holds unspecified bytes)     */
    int32_t status;     /* XLZ_OK; XLZ_ERR_RESULT: the merge failed, or a stream it names did not decode; XLZ_ERR_UNSUPPORTED:
                           out_len or a stream of 4 GiB or more, or a stream that never sat in the arena          */
    int32_t reserved;
} xlz_bcj2_result;
/* Like xlz_batch_pack it waits for and collects the batch's latest run, then merges every item into ONE caller-owned device
 * buffer.  One bad item never fails the call.  XLZ_ERR_BAD_ARG, with nothing written: NULL arguments with n > 0; a stream
 * index >= the batch's streams (other than XLZ_BCJ2_RAW); a raw stream without a pointer; d_dst is not device memory of the
 * context's device, or dst_cap reaches past its allocation; an item's [dst_off, dst_off + out_len) does not fit in dst_cap;
 * the declared destination ranges of two items overlap.  Nothing outside the items' ranges is written.  An item longer
 * than the launch-length cap (0.5 s of one wave: xlzbcj2::kMaxDeviceLen), and every item in bcj2 mode 2, is merged by
 * xlz_bcj2_host's code on host threads over downloaded streams and uploaded.                              */
int xlz_batch_bcj2(xlz_batch *batch, const xlz_bcj2_item *items, size_t n, void *d_dst, size_t dst_cap, xlz_bcj2_result *results);
/* What xlz_7z_decode / xlz_7z_decode_device do with BCJ2 folders.  0 (default): they refuse them (XLZ_ERR_UNSUPPORTED), as
 * ever.  1: they decode them, merged on the device.  2: as 1, but merged on host threads over downloaded streams and
 * uploaded -- the fallback path and the A/B yardstick.  The _multi form and the pull readers ignore the mode.  Any other
 * value: XLZ_ERR_BAD_ARG.                                                                                 */
int xlz_ctx_set_bcj2_mode(xlz_ctx *ctx, int mode);
int xlz_ctx_bcj2_mode(const xlz_ctx *ctx);
/* Of the most recent xlz_batch_bcj2 on `ctx`, or of the most recent xlz_7z_decode / xlz_7z_decode_device in bcj2 mode 1 / 2. */
typedef struct xlz_bcj2_stats {
    uint64_t device_items, device_bytes; /* merged by the kernel (bytes of output)                            */
    uint64_t host_items, host_bytes;     /* merged on host threads: mode 2, or longer than the cap            */
    uint64_t failed_items;               /* of either: status < 0                                             */
    double kernel_ms;                    /* the kernel by HIP events                                          */
    uint32_t launches;
    uint32_t reserved;
} xlz_bcj2_stats;
int xlz_ctx_last_bcj2_stats(xlz_ctx *ctx, xlz_bcj2_stats *out);

/* ---- raw deflate streams (lzma_amd/csrc/xlz_inflate_dev.hip) ----
 * Outside the reference.  Deflate (RFC 1951) is method 8 of a .zip archive: what nearly every archive uses.  A stream is
 * decoded by ONE wave -- symbol decode wave-uniform, tables and input window in LDS, the lanes carrying literals, matches
 * and stored blocks --, and the window is the output itself in device memory (the statement of the format, of the wave
 * scheme and of what is which error is at the head of lzma_amd/csrc/xlz_inflate_dev.h).  Written from the RFC; the
 * classes of failure are those of zlib 1.2.11, the first defect in stream order deciding:
 *   XLZ_OK                  the final block's end-of-block was reached; input behind it is ignored, *consumed / in_consumed
 *                           says where it stopped (the byte that holds the last bit included)
 *   XLZ_ERR_RESULT          invalid data: block type 3, LEN / NLEN mismatch, too many length or distance symbols, a bad
 *                           repeat, an over-subscribed or incomplete set of code lengths as zlib judges them, no
 *                           end-of-block code, an invalid literal/length or distance code, a distance too far back
 *   XLZ_ERR_UNEXPECTED_EOF  the input ends first
 *   XLZ_ERR_OUT_CAP         the output would pass out_cap
 * On a failure produced is 0 and the item's own range holds unspecified bytes.  No zlib or gzip wrapper is read.        */
/* The serial decoder over host buffers: host only, no device needed.  XLZ_ERR_BAD_ARG: a NULL pointer with a length
 * behind it.  produced and consumed may be NULL.                                                            */
int xlz_inflate_host(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap, size_t *produced, size_t *consumed);
typedef struct xlz_inflate_item {
    const uint8_t *in;  /* host memory: the stream                                                               */
    uint64_t in_len;
    uint64_t dst_off;   /* where its output goes in the destination                                              */
    uint64_t dst_cap;   /* the room there                                                                        */
} xlz_inflate_item;
typedef struct xlz_inflate_result {
    uint64_t produced;    /* 0 unless XLZ_OK                                                                     */
    uint64_t in_consumed; /* 0 unless XLZ_OK                                                                     */
    int32_t status;
    uint32_t reserved;
} xlz_inflate_result;
/* Inflates every item into ONE caller-owned device buffer: host threads gather the inputs into one pinned block of the
 * context's pool, each at a padded offset that is a multiple of 16, the block goes up in one transfer with the item table
 * in front (xlz_inflate_stats::uploads stays 1 below 256 MiB of input), one launch sequence writes every item straight
 * into d_dst + dst_off, and the call waits.  One bad item never fails the call.  XLZ_ERR_BAD_ARG, with nothing written:
 * NULL arguments with n > 0; an item without a pointer to its length; an item's [dst_off, dst_off + dst_cap) does not fit
 * in dst_cap; the ranges of two items share a byte; d_dst is not device memory of the context's device, or dst_cap
 * reaches past its allocation.  n = 0 is XLZ_OK.  Nothing outside the items' ranges is written.  An item whose input or
 * room is longer than the launch-length cap (0.5 s of one wave: xlzinf::kMaxDeviceLen) or 0xFFFF0000 bytes and more, and
 * every item in deflate mode 2, is inflated by xlz_inflate_host's code on host threads and uploaded.  The call itself does
 * not look at whether the mode is 0.                                                                        */
int xlz_inflate_batch(xlz_ctx *ctx, const xlz_inflate_item *items, size_t n, void *d_dst, size_t dst_cap, xlz_inflate_result *results);
/* What xlz_zip_extract / xlz_zip_extract_device do with deflate entries (XLZ_ZIP_ENTRY_DEFLATE).  0 (default): they refuse
 * them (XLZ_ERR_UNSUPPORTED), as ever.  1: they inflate them on the device, in the same call as the LZMA batch and the
 * stored scatter.  2: as 1, but on host threads, uploaded -- the fallback path and the A/B yardstick.  Any other value:
 * XLZ_ERR_BAD_ARG.                                                                                          */
int xlz_ctx_set_deflate_mode(xlz_ctx *ctx, int mode);
int xlz_ctx_deflate_mode(const xlz_ctx *ctx);
/* Of the most recent xlz_inflate_batch on `ctx`, or of the most recent xlz_zip_extract / xlz_zip_extract_device in deflate
 * mode 1 / 2 that had a deflate entry to inflate.                                                            */
typedef struct xlz_inflate_stats {
    uint64_t device_items, device_bytes; /* inflated by the kernel (bytes of output of the good ones)          */
    uint64_t host_items, host_bytes;     /* inflated on host threads: mode 2, or longer than the cap           */
    uint64_t failed_items;               /* of either: status < 0                                              */
    uint32_t uploads;                    /* transfers of gathered inputs                                       */
    uint32_t launches;
} xlz_inflate_stats;
int xlz_ctx_last_inflate_stats(xlz_ctx *ctx, xlz_inflate_stats *out);

/* ---- pull-style readers mirroring the reference's Go surface --------------- */
/* Constructors take the compressed stream as a buffer (a Go shim slurps its io.Reader
 * first) and copy it.  Constructor-time errors are the ones the reference's
 * constructors return; decode errors surface from xlz_reader_read once all bytes
 * produced before the error have been delivered.
 *
 * A reader is a resumable decode on the device (reader1.go:223-254 / decompress.go:13:
 * decompress(need) returns once `need` bytes are pending): every refill continues the
 * saved decoder state for about 1 MiB of output and stops.  Memory is bounded like the
 * reference's: one refill chunk on the host, 2 x dictSize + one chunk of window on the
 * device (less for streams of known size), a 4 MiB input window on the device.  The
 * stream is decoded exactly once, whatever its size or compression ratio.  An LZMA2
 * stream whose headers announce eight or more dictionary-reset units is served in runs
 * of whole units (<= 64 MiB of output each) decoded unit-parallel by the batch engine.
 * Sessions cover the reference's whole parameter range: a model with lc+lp > 8 (it does not fit
 * a CU's LDS) runs in the HBM-model launch, an LZMA2 chunk that renews the model with larger
 * properties makes the session grow its state block, and copies that read behind an LZMA2
 * dictionary reset are served from an image of the reference's uncleared window buffer
 * (window.go:135-140) that the device keeps per reader (dictSize bytes, like the window itself). */
typedef struct xlz_reader xlz_reader;
xlz_reader *xlz_new_reader1(xlz_ctx *ctx, const uint8_t *in, size_t in_len, int *err); /* NewReader1 */
xlz_reader *xlz_new_reader2(xlz_ctx *ctx, const uint8_t *in, size_t in_len, int dict_size,
                            int *err);                                              /* NewReader2 */
/* NewLZMADecompressorForSevenZip(props, unpackSize, readers) reader1.go:32-61 */
xlz_reader *xlz_new_lzma_decompressor_for_sevenzip(xlz_ctx *ctx, const uint8_t *props,
                                                   size_t props_len, uint64_t unpack_size,
                                                   const uint8_t *const *readers,
                                                   const size_t *reader_lens, size_t n_readers,
                                                   int *err);
/* NewLZMA2DecompressorForSevenZip(props, _, readers) reader2.go:49-75 */
xlz_reader *xlz_new_lzma2_decompressor_for_sevenzip(xlz_ctx *ctx, const uint8_t *props,
                                                    size_t props_len, uint64_t unpack_size,
                                                    const uint8_t *const *readers,
                                                    const size_t *reader_lens, size_t n_readers,
                                                    int *err);
/* Read(p): returns bytes copied (>= 0).  *err: XLZ_OK while more may follow;
 * XLZ_EOF at end of stream; a negative status on error.                          */
#define XLZ_EOF 100
#define XLZ_NEED_INPUT 101 /* streaming input only: feed the next piece (or declare the end), read again */
long xlz_reader_read(xlz_reader *r, uint8_t *p, size_t n, int *err);
/* Streaming input: the reference's readers pull from an io.Reader as they go (reader1.go:18-24,
 * decompress.go:35: one ReadByte per normalisation); the C ABI takes buffers, so the pull is turned
 * around.  Construct the reader from the FIRST piece of the stream (at least the .lzma header / the
 * first LZMA2 chunk header and the five range-coder bytes: the constructors check those), call
 * xlz_reader_expect_more once, then: xlz_reader_read returns XLZ_NEED_INPUT whenever the decoder has
 * used up its input -- feed the next piece (any size; >= 128 KiB keeps LZMA2 chunks whole) or
 * declare the end, and read again.  The library keeps only the bytes the decoder has not consumed:
 * with this, a reader's memory is bounded on BOTH sides.  A fed reader decodes everything a reader
 * over the whole buffer decodes (models up to lc = 8, lp = 4 taken up in mid-stream; copies that read
 * behind an LZMA2 dictionary reset).  xlz_reader_expect_more is also accepted right after
 * xlz_reader_reopen: (*Reader1).Reopen takes an io.ByteReader (reader1.go:166-176), `in` is then the
 * first piece of the new stream (at least its five range-coder bytes).                            */
int xlz_reader_expect_more(xlz_reader *r);
int xlz_reader_feed(xlz_reader *r, const uint8_t *data, size_t n);
int xlz_reader_feed_eof(xlz_reader *r);
/* (*Reader1).Reset (reader1.go:161-164): the probability model, state and reps start over, the window
 * and the input position stay.  (*Reader1).Reopen (reader1.go:166-176): continue on a NEW raw LZMA
 * stream (no header) with the given unpack size (all-ones = unknown), same window and model; its
 * return value is rangeDec.Reopen's error (XLZ_ERR_HEADER_EOF = io.EOF, XLZ_ERR_RESULT).  Readers
 * made by xlz_new_reader1 / ..._lzma_decompressor_for_sevenzip only.                              */
int xlz_reader_reset(xlz_reader *r);
int xlz_reader_reopen(xlz_reader *r, const uint8_t *in, size_t in_len, uint64_t unpack_size);
int xlz_reader_close(xlz_reader *r); /* readCloser.Close (readcloser.go:16-28); second call ->
                                        XLZ_ERR_CLOSED; the handle stays valid until _free       */
void xlz_reader_free(xlz_reader *r);
/* launches that refilled this reader, whole-stream fallback decodes (0 unless one of the two
 * cases above), compressed bytes uploaded so far -- for tests of the one-pass property     */
int xlz_reader_stats(const xlz_reader *r, uint64_t *refills, uint64_t *whole_decodes,
                     uint64_t *in_uploaded);
/* device memory the reader holds right now: its sliding output window, and the image of the
 * reference's uncleared window buffer (dictSize bytes; window.go:135-140) -- 0 until the stream's
 * first dictionary reset behind a non-empty epoch, i.e. for nearly every stream                 */
int xlz_reader_memory(const xlz_reader *r, uint64_t *window_bytes, uint64_t *image_bytes);

/* Multi-GPU form of xlz_decode_batch: one context per GPU; every context
 * decodes its shard on its own host thread, results come back in input order.  No device-to-device
 * traffic.  The work is dealt by COMPRESSED bytes (what the kernel's own work queue is keyed by):
 * whole streams, and -- for a raw LZMA2 stream that is a large part of the call -- runs of its units
 * (xlz_lzma2_units: a dictionary reset with new properties starts an independent unit,
 * reader2.go:100-173), each GPU getting a slice of the compressed input and a disjoint slice of the
 * caller's output buffer.  A stream whose slices do not decode to exactly what their headers
 * announce (malformed streams only) is decoded again as a whole on one context, so bytes, status
 * and in_consumed are the single-GPU call's.                                                     */
int xlz_decode_batch_multi(xlz_ctx *const *ctxs, size_t n_ctx, const xlz_stream_desc *streams,
                           size_t n, xlz_result *results);
/* The plan of such a call alone (host only, no GPU): the items -- whole streams and runs of units of
 * LZMA2 streams -- and the context each goes to.  At most max_items entries are filled, *n_items =
 * their number (XLZ_ERR_OUT_CAP when larger than max_items > 0; max_items = 0 counts).  The items of
 * a stream are adjacent and in stream order.                                                      */
typedef struct xlz_multi_item {
    uint64_t stream;           /* index into streams                                               */
    uint64_t in_off, in_len;   /* the slice of the stream's input                                  */
    uint64_t out_off, out_len; /* the slice of its output (whole streams: 0, out_cap)              */
    uint32_t context;          /* index into ctxs                                                  */
    uint32_t flags;            /* 1 whole stream, 2 begins at the stream's start, 4 ends at its end */
} xlz_multi_item;
int xlz_decode_batch_multi_plan(size_t n_ctx, const xlz_stream_desc *streams, size_t n, xlz_multi_item *items,
                                size_t max_items, size_t *n_items);

/* ---- the unit plan of a raw LZMA2 stream (host only, no GPU needed) ------------------------
 * What a decode of `in` as XLZ_FMT_LZMA2_RAW launches: the stream is cut where a chunk starts
 * that depends on nothing before it (Reader2.startChunk, reader2.go:100-173: a dictionary reset
 * with new properties; a stored chunk that resets the dictionary when no LZMA chunk behind it
 * continues an earlier model; every 256 KiB inside a run of stored chunks that ends at a dictionary
 * reset or at the end of the stream) -- one wave per unit.  Fills at most `max_units` entries,
 * *n_units = the number of units (XLZ_ERR_OUT_CAP when larger than max_units > 0; pass
 * max_units = 0 to count).  Offsets are trusted from the chunk headers: a stream whose real
 * decode leaves them is decoded again as ONE unit after the launch.                          */
typedef struct xlz_lzma2_unit {
    uint64_t in_off, in_len;   /* bytes of `in` the unit walks                                   */
    uint64_t out_off, out_len; /* where its output goes and how much its headers announce        */
    uint32_t have_reader;      /* an LZMA chunk precedes it in the stream (Reader2.lzmaReader)   */
    uint32_t reserved;
} xlz_lzma2_unit;
int xlz_lzma2_units(const uint8_t *in, size_t len, xlz_lzma2_unit *units, size_t max_units, size_t *n_units);

/* ---- .xz container front-end ----------------------------
 * Outside the reference (which has no container code): an .xz file is a list of independent
 * blocks, each ONE raw LZMA2 stream with its own dictionary -- what NewReader2(in, dictSize)
 * takes (reader2.go:26-41) -- so a file is one batch.  By default only filter chains made of a
 * single LZMA2 filter are accepted (BCJ / Delta: XLZ_ERR_UNSUPPORTED); in filter mode 1
 * (xlz_ctx_set_filter_mode) xlz_xz_decode also takes blocks with one to three Delta / BCJ filters
 * in front of LZMA2 and undoes them on the device between decode and check (xlz_xz_index_chains
 * lists them).  xlz_xz_index and xlz_xz_decode_multi refuse such blocks in either mode.         */
typedef struct xlz_xz_block {
    uint64_t comp_off;   /* raw LZMA2 payload inside the file                                   */
    uint64_t comp_len;
    uint64_t uncomp_off; /* where the block's bytes go in the decoded file                      */
    uint64_t uncomp_len;
    uint64_t check_off;  /* the block's integrity check inside the file                         */
    uint32_t dict_size;
    uint32_t check_type; /* 0 none, 1 CRC32, 4 CRC64, 10 SHA-256                                */
} xlz_xz_block;

/* Block index of a whole .xz file (concatenated streams and stream padding included), host
 * only.  blocks may be NULL with max_blocks 0 to obtain the counts.  XLZ_ERR_OUT_CAP: more
 * blocks than max_blocks (*n_blocks is the full count).                                      */
int xlz_xz_index(const uint8_t *file, size_t len, xlz_xz_block *blocks, size_t max_blocks,
                 size_t *n_blocks, uint64_t *total_uncompressed);
/* xlz_xz_index for files whose blocks carry filter chains: one to three of the filters Delta (0x03), x86 (0x04), PowerPC
 * (0x05), IA-64 (0x06), ARM (0x07), ARM-Thumb (0x08), SPARC (0x09) in front of the LZMA2 filter.  Their steps come back
 * in the order a decoder applies them (the reverse of the block header's), step.stream = the block's index; a block of
 * one LZMA2 filter has none.  What liblzma refuses is XLZ_ERR_UNSUPPORTED: a wrong property size, a start offset that
 * is not a multiple of the filter's alignment, LZMA2 not last, another filter last, ARM64 / RISC-V / unknown ids.
 * steps may be NULL with max_steps 0 to obtain the count; XLZ_ERR_OUT_CAP: more steps than max_steps.      */
int xlz_xz_index_chains(const uint8_t *file, size_t len, xlz_xz_block *blocks, size_t max_blocks, size_t *n_blocks,
                        xlz_filter_step *steps, size_t max_steps, size_t *n_steps, uint64_t *total_uncompressed);
/* Decode a whole .xz file into out as ONE GPU batch.  verify != 0: check every block's CRC32 /
 * CRC64 / SHA-256 on the host; *unverified (optional) = number of blocks whose check type is a
 * reserved one.  A failed check or a block that does not match the index:
 * XLZ_ERR_RESULT.                                                                             */
int xlz_xz_decode(xlz_ctx *ctx, const uint8_t *file, size_t len, uint8_t *out, size_t out_cap,
                  uint64_t *out_len, int verify, size_t *unverified);
/* xlz_xz_decode into DEVICE memory: d_out is out_cap bytes on the context's device, and the decoded file ends up
 * there contiguous -- decode, filters (filter mode 1, as xlz_xz_decode), checks and a pack (xlz_batch_pack) all run on the
 * device; only the digests come to the host, where they are compared.  Same status, *out_len and *unverified as
 * xlz_xz_decode on the same context for every input, with one exception: a block of 4 GiB or more is
 * XLZ_ERR_UNSUPPORTED.  verify != 0 always checks through the check kernels (CRC32 / CRC64) and the xlz_batch_digests
 * path (SHA-256), whatever the context's check mode: that mode says where a host-destination call verifies.  On failure
 * *out_len = 0 and the contents of d_out are unspecified.  The call holds the output arena AND the destination: about
 * twice the decoded size of device memory.  It returns when its work on the device is done; no other stream may use
 * d_out meanwhile.                                                                                                 */
int xlz_xz_decode_device(xlz_ctx *ctx, const uint8_t *file, size_t len, void *d_out, size_t out_cap,
                         uint64_t *out_len, int verify, size_t *unverified);
/* the same over several contexts (one per GPU): the blocks -- and the units inside large blocks -- are
 * dealt to the contexts by xlz_decode_batch_multi                                                */
int xlz_xz_decode_multi(xlz_ctx *const *ctxs, size_t n_ctx, const uint8_t *file, size_t len, uint8_t *out,
                        size_t out_cap, uint64_t *out_len, int verify, size_t *unverified);

/* ---- byte ranges of an .xz file ---------------------------------------
 * The index at the end of an .xz file says where every block's bytes lie in the decoded file, so bytes [off, off + len)
 * of the DECODED file cost the blocks that hold them and nothing else.  xlz_xz_open parses the file once -- as
 * xlz_xz_index_chains does, with the same status for every input -- and keeps the block table, the filter steps and a
 * BORROWED pointer to `file`: the caller keeps those bytes alive and unchanged until xlz_xz_close (an mmap is fine; a
 * read touches only the payloads and check fields of the blocks it decodes).  The handle never changes afterwards: any
 * number of threads and contexts may use one at once.  Open, close, info, blocks and cover are host only, no device
 * needed.  xlz_xz_file_blocks: the table as xlz_xz_index_chains gives it (XLZ_ERR_OUT_CAP: more blocks than max_blocks).
 *
 * A range is clipped to the decoded size like pread: copied[i] (copied may be NULL) = the bytes written for range i, 0
 * for len == 0 or off >= size.  Two ranges may read the same bytes.  xlz_xz_cover: the ascending, duplicate-free
 * indices of the blocks the ranges touch, by binary search over uncomp_off (blocks may be NULL with max_blocks 0 to
 * obtain the count; XLZ_ERR_OUT_CAP: more than max_blocks).
 *
 * xlz_xz_read_device: ONE batch of the covering blocks -- each decoded once, however many ranges hit it --, then on the
 * device the filter steps of those blocks (filter mode 1; a covering block with a filter chain on a context in filter
 * mode 0 is XLZ_ERR_UNSUPPORTED, a chain on a block outside the cover never matters), the checks and ONE pack of
 * (range, block) pieces to d_out + dst_off.  verify != 0 verifies every covering block's check over the WHOLE block,
 * through the check kernels and the xlz_batch_digests path as xlz_xz_decode_device does; *unverified (optional) = the
 * covering blocks whose check type is a reserved one.  A covering block must produce what the index says and use its
 * whole payload (XLZ_ERR_RESULT, or the block's own status), and one of 4 GiB or more is XLZ_ERR_UNSUPPORTED.  Damage
 * in a block outside the cover is not seen.  xlz_xz_read: the same into host memory, through a device staging buffer of
 * the sum of the clipped lengths that the context keeps for the next read (xlz_ctx_trim releases it).
 * XLZ_ERR_BAD_ARG: NULL arguments with n > 0; a clipped destination [dst_off, dst_off + copied[i]) that does not fit
 * out_cap; two clipped destinations that share a byte (these are tested before the context is used; a range clipped to
 * nothing declares no byte, wherever its dst_off points); d_out that is not out_cap bytes of device memory of the
 * context's device.  Such a call, and one refused for a covering chain in filter mode 0, launches nothing, writes
 * nothing and leaves every statistic as it was.  On every failure all copied[i] are 0 and the contents of the
 * destination ranges are unspecified; bytes that no range covers are never written.  The call holds the arena of the
 * covering blocks plus the destination (or staging), and returns when its device work is done.                    */
typedef struct xlz_xz_file xlz_xz_file;
int xlz_xz_open(const uint8_t *file, size_t len, xlz_xz_file **f);
void xlz_xz_close(xlz_xz_file *f);
int xlz_xz_file_info(const xlz_xz_file *f, uint64_t *size, size_t *n_blocks, size_t *n_steps);
int xlz_xz_file_blocks(const xlz_xz_file *f, xlz_xz_block *blocks, size_t max_blocks);
typedef struct xlz_xz_range {
    uint64_t off, len; /* bytes of the DECODED file, clipped to its size                                 */
    uint64_t dst_off;  /* where they go in the destination                                               */
} xlz_xz_range;
int xlz_xz_cover(const xlz_xz_file *f, const xlz_xz_range *ranges, size_t n, size_t *blocks, size_t max_blocks,
                 size_t *n_blocks);
int xlz_xz_read(xlz_ctx *ctx, const xlz_xz_file *f, const xlz_xz_range *ranges, size_t n, uint8_t *out, size_t out_cap,
                uint64_t *copied, int verify, size_t *unverified);
int xlz_xz_read_device(xlz_ctx *ctx, const xlz_xz_file *f, const xlz_xz_range *ranges, size_t n, void *d_out,
                       size_t out_cap, uint64_t *copied, int verify, size_t *unverified);
/* Of the most recent xlz_xz_read / xlz_xz_read_device on `ctx` (which also starts the check, SHA-256, filter and pack
 * statistics over and fills them).                                                                                  */
typedef struct xlz_xz_read_stats {
    uint64_t ranges, empty_ranges; /* as given; of them clipped to nothing                                */
    uint64_t blocks, comp_bytes;   /* the cover: the blocks decoded and their payload bytes               */
    uint64_t decoded_bytes;        /* the sum of the covering blocks' decoded sizes                       */
    uint64_t copied_bytes;         /* the sum of copied[] (0 when the read failed)                        */
} xlz_xz_read_stats;
int xlz_ctx_last_xz_read_stats(xlz_ctx *ctx, xlz_xz_read_stats *out);

/* ---- many .xz files as ONE batch, each with a status of its own ---------
 * What xz writes by default is one block per file, so a directory of small .xz files is a batch only across files.
 * Every file has a window [dst_off, dst_off + dst_cap) in one destination; xlz_xz_many_layout (host only, no device) lays
 * the windows out back to back: it parses every index -- results[i].status = what xlz_xz_index (chains == 0) or
 * xlz_xz_index_chains (chains != 0) returns for file i --, sets dst_cap = the index's total (0 for a refused file) and
 * dst_off = the next multiple of align (>= 1; 0: XLZ_ERR_BAD_ARG), and *total = the end of the last window.
 * XLZ_ERR_OUT_CAP: the windows do not fit 64 bits.  `file` is borrowed for the call; the same file may be named twice.
 *
 * Per file: results[i].status and .unverified are what xlz_xz_decode (xlz_xz_decode_many) or xlz_xz_decode_device
 * (xlz_xz_decode_many_device) returns for (file, len, a buffer of dst_cap bytes) ALONE on the same context with the same
 * filter and check mode, and when that is XLZ_OK, out_len and the bytes at dst_off are what it produces.  That includes
 * the order in which a file's failures are found: the index parse; XLZ_ERR_OUT_CAP when the index announces more than
 * dst_cap; in the device form XLZ_ERR_UNSUPPORTED for a block of 4 GiB or more; the first block in file order whose own
 * status is negative or whose sizes are not the index's (XLZ_ERR_RESULT); the first failed check (XLZ_ERR_RESULT).  A
 * chain in filter mode 0 is XLZ_ERR_UNSUPPORTED, from the index parse.  A file that fails before the batch is made puts
 * nothing into the batch (blocks = comp_bytes = 0).  An empty .xz file (no blocks) is a good file of out_len 0.
 *
 * The call itself returns XLZ_OK whenever it ran, however many files failed.  XLZ_ERR_BAD_ARG: ctx, files, results or
 * the destination NULL (with n > 0 and out_cap > 0); a window that does not fit out_cap (no sum is formed unless it
 * fits); two windows that share a byte (a window with dst_cap == 0 declares no byte, wherever its dst_off points) --
 * these are tested before the context is used --; d_out that is not out_cap bytes of device memory of the context's
 * device.  Such a call launches nothing, writes nothing -- results[] included -- and leaves every statistic as it was; so
 * does n == 0, which is XLZ_OK.  Another negative status (XLZ_ERR_DEVICE): the batch could not run, and every
 * results[i].status is that status too.
 *
 * Bytes outside every window are never written; inside the window of a good file, bytes behind out_len are not written;
 * inside the window of a failed file the contents are unspecified.
 *
 * xlz_xz_decode_many_device is ONE batch (xlz_batch_create / run / results) over all blocks of all files that got that
 * far, then on the device the filter steps (filter mode 1), the digests of every block with a known check (verify != 0;
 * whatever the check mode, as xlz_xz_decode_device) and ONE pack; a block that failed or does not match its index is
 * left out of these.  xlz_xz_decode_many goes the way of xlz_xz_decode -- the pipelined, sliced xlz_decode_batch with
 * every block's output inside its file's window, sessions for blocks of 4 GiB and more -- and verifies where the
 * context's check mode says.  The call holds the arena of all files (the device form: plus the destination); a set that
 * does not fit device memory is the caller's to cut -- the layout's total tells.                                       */
typedef struct xlz_xz_many_file {
    const uint8_t *file; /* one whole .xz file, borrowed for the call                                    */
    size_t len;
    uint64_t dst_off;    /* its window [dst_off, dst_off + dst_cap) in the destination                   */
    uint64_t dst_cap;
} xlz_xz_many_file;
typedef struct xlz_xz_many_result {
    int32_t status;      /* what the single-file call would return for this file                         */
    uint32_t unverified; /* its blocks with a reserved check type (0 unless status == XLZ_OK)            */
    uint64_t out_len;    /* decoded bytes at dst_off; 0 unless status == XLZ_OK                          */
    uint64_t blocks;     /* what it put into the batch: blocks ...                                       */
    uint64_t comp_bytes; /* ... and their payload bytes                                                  */
} xlz_xz_many_result;
int xlz_xz_many_layout(xlz_xz_many_file *files, size_t n, int chains, uint64_t align, xlz_xz_many_result *results,
                       uint64_t *total);
int xlz_xz_decode_many(xlz_ctx *ctx, const xlz_xz_many_file *files, size_t n, uint8_t *out, size_t out_cap, int verify,
                       xlz_xz_many_result *results);
int xlz_xz_decode_many_device(xlz_ctx *ctx, const xlz_xz_many_file *files, size_t n, void *d_out, size_t out_cap,
                              int verify, xlz_xz_many_result *results);
/* Of the most recent xlz_xz_decode_many / xlz_xz_decode_many_device on `ctx` that ran (which also starts the check,
 * SHA-256, filter and pack statistics over and fills them).                                                         */
typedef struct xlz_xz_many_stats {
    uint64_t files, failed_files; /* as given; of them with a status other than XLZ_OK                  */
    uint64_t blocks, comp_bytes;  /* the batch: the blocks decoded and their payload bytes              */
    uint64_t decoded_bytes;       /* the sum of out_len over the good files                             */
} xlz_xz_many_stats;
int xlz_ctx_last_xz_many_stats(xlz_ctx *ctx, xlz_xz_many_stats *out);

/* ---- .7z container front-end ----------------------------
 * (The parser was written from 7-Zip's published format description.  It is exercised on archives
 * built from that description by tests/sevenzip_craft.py and their mutations AND on archives by an
 * independent writer -- libarchive's 7zip writer, which `cmake -E tar cf x.7z --format=7zip` drives
 * in this image: solid LZMA1 folders, LZMA-encoded headers, per-file CRCs, an 8 MiB dictionary that
 * wraps; tests/golden/libarchive_solid.7z is one of them.  7-Zip's own binary is not in the image.)
 * Outside the reference, which only offers the two bodgit/sevenzip decompressor constructors
 * (reader1.go:28-61 method 03 01 01, reader2.go:45-75 method 21).  A .7z archive keeps its data in
 * folders, each ONE compressed stream with out-of-band properties -- exactly what those
 * constructors take -- and folders are independent, so an archive is one batch.  Folders with a
 * single LZMA, LZMA2 or Copy coder are decoded; in filter mode 1 (xlz_ctx_set_filter_mode)
 * xlz_7z_decode also takes folders that are a line of Delta / BCJ filters behind one LZMA / LZMA2
 * coder (xlz_7z_index_chains) and undoes the filters on the device between decode and CRC; in bcj2
 * mode 1 / 2 (xlz_ctx_set_bcj2_mode) also BCJ2 folders (xlz_7z_index_bcj2), merged on the device.  Other
 * coder graphs, encryption and external / multi-volume layouts are reported as unsupported.  xlz_7z_decode and its kin do not
 * look at file names: their output is the folders' bytes back to back = the archive's files back to back.  The file table
 * (names, sizes, times) and the extraction of chosen files are xlz_7z_open / xlz_7z_extract below.  */
enum { XLZ_7Z_UNSUPPORTED = 0, XLZ_7Z_LZMA = 1, XLZ_7Z_LZMA2 = 2, XLZ_7Z_COPY = 3,
       XLZ_7Z_BCJ2 = 4 /* xlz_7z_index_bcj2 only */ };
typedef struct xlz_7z_folder {
    uint64_t pack_off;   /* the folder's packed stream inside the file                           */
    uint64_t pack_len;
    uint64_t unpack_off; /* where its bytes go in the decoded output                             */
    uint64_t unpack_len;
    uint32_t method;     /* XLZ_7Z_*                                                             */
    uint32_t dict_size;  /* LZMA: LE32 of props[1:5]; LZMA2: DecodeDictSize2(props[0])           */
    uint32_t crc;        /* CRC32 of the folder's output when has_crc                            */
    uint32_t first_substream, n_substreams; /* its files in the substream array                  */
    uint8_t props;       /* LZMA: the lc/lp/pb byte; LZMA2: the dictionary byte                  */
    uint8_t has_crc;
    uint8_t reserved[2];
} xlz_7z_folder;
typedef struct xlz_7z_substream { /* one file's bytes inside a (solid) folder                    */
    uint64_t size;
    uint32_t crc;
    uint32_t has_crc;
} xlz_7z_substream;
/* Folder list of a .7z archive.  An encoded (compressed) header -- what 7-Zip writes by default --
 * is itself an LZMA folder and is decoded on the GPU first: ctx may be NULL only for archives with a
 * plain header.  Arrays may be NULL with capacity 0 to obtain the counts; XLZ_ERR_OUT_CAP when a
 * non-zero capacity is too small (the counts are still set).                                      */
int xlz_7z_index(xlz_ctx *ctx, const uint8_t *file, size_t len, xlz_7z_folder *folders,
                 size_t max_folders, size_t *n_folders, xlz_7z_substream *substreams,
                 size_t max_substreams, size_t *n_substreams, uint64_t *total_unpacked);
/* xlz_7z_index for archives whose folders are coder chains.  A folder of 2-4 coders is accepted when every coder has one
 * input and one output, the coders are bound into one line, there is exactly one packed stream, an LZMA / LZMA2 coder reads
 * it and all the others are Delta (method 03, one property byte) or BCJ filters (x86 03030103, PowerPC 03030205, IA-64
 * 03030401, ARM 03030501, ARM-Thumb 03030701, SPARC 03030805; no properties: start offset 0) and every size in the
 * folder's unpack-size list is the same.  Such a folder carries the method, props and dictionary of its LZMA / LZMA2 coder,
 * and its filters come back as steps in the order a decoder applies them, step.stream = the folder's index.  Anything
 * else (BCJ2, encryption, ARM64, ...) stays XLZ_7Z_UNSUPPORTED.  xlz_7z_index keeps reporting every chain as method 0. */
int xlz_7z_index_chains(xlz_ctx *ctx, const uint8_t *file, size_t len, xlz_7z_folder *folders, size_t max_folders,
                        size_t *n_folders, xlz_7z_substream *substreams, size_t max_substreams, size_t *n_substreams,
                        xlz_filter_step *steps, size_t max_steps, size_t *n_steps, uint64_t *total_unpacked);
/* xlz_7z_index_chains plus the BCJ2 folders: a folder that is one of the two BCJ2 forms comes back with method
 * XLZ_7Z_BCJ2 -- here only: xlz_7z_index and xlz_7z_index_chains keep reporting it as method 0 --, unpack_len = the size of
 * the MERGED bytes (what its CRC and its files' CRCs cover), pack_off / pack_len = its first packed stream, and a record
 * that places its four streams.  The two forms, found by following the bind pairs and the packed-stream index list:
 *   four coders: three LZMA / LZMA2 coders (one input, one output each) feeding inputs 0 (main), 1 (call), 2 (jump) of a
 *   BCJ2 coder (4 inputs, 1 output, no properties); four packed streams: the three coders' inputs and BCJ2's input 3 (rc);
 *   two coders: one LZMA / LZMA2 coder feeding input 0; call, jump and rc are packed streams read raw.
 * Everything else stays XLZ_7Z_UNSUPPORTED: other stream counts, properties on BCJ2, an input bound twice, rc fed by a
 * coder, a sub-coder that is neither LZMA nor LZMA2, filters in front of the sub-coders or behind BCJ2, a call / jump size
 * that is not a multiple of 4.  bcj2 may be NULL with max_bcj2 0 to obtain the count; XLZ_ERR_OUT_CAP as above.     */
typedef struct xlz_7z_bcj2_sub {
    uint64_t pack_off, pack_len; /* inside the file                                                          */
    uint64_t unpack_len;         /* raw: pack_len                                                             */
    uint32_t method;             /* XLZ_7Z_LZMA / XLZ_7Z_LZMA2, or XLZ_7Z_COPY: read raw                      */
    uint32_t dict_size;
    uint8_t props;
    uint8_t reserved[7];
} xlz_7z_bcj2_sub;
typedef struct xlz_7z_bcj2 {
    uint64_t folder;             /* index into folders                                                        */
    xlz_7z_bcj2_sub main_s, call_s, jump_s;
    uint64_t rc_off, rc_len;
} xlz_7z_bcj2;
int xlz_7z_index_bcj2(xlz_ctx *ctx, const uint8_t *file, size_t len, xlz_7z_folder *folders, size_t max_folders,
                      size_t *n_folders, xlz_7z_substream *substreams, size_t max_substreams, size_t *n_substreams,
                      xlz_filter_step *steps, size_t max_steps, size_t *n_steps, xlz_7z_bcj2 *bcj2, size_t max_bcj2,
                      size_t *n_bcj2, uint64_t *total_unpacked);
/* Decode every folder of a .7z archive into out as ONE GPU batch.  verify != 0: CRC32 of every file
 * (or folder) that carries one; *unverified (optional) = folders without any CRC.  XLZ_ERR_UNSUPPORTED
 * when a folder is not a single LZMA / LZMA2 / Copy coder (filter mode 1: nor a chain as above; bcj2 mode 1 / 2: nor a
 * BCJ2 folder).  In bcj2 mode 1 / 2 an archive that HAS a BCJ2 folder is decoded as xlz_7z_decode_device decodes it, into a
 * device buffer from the context's pool, followed by one download; a BCJ2 folder of 4 GiB or more is XLZ_ERR_UNSUPPORTED, one
 * whose streams do not decode to their announced sizes or whose merge fails XLZ_ERR_RESULT.  Other archives take the path
 * they always took.                                                                                     */
int xlz_7z_decode(xlz_ctx *ctx, const uint8_t *file, size_t len, uint8_t *out, size_t out_cap,
                  uint64_t *out_len, int verify, size_t *unverified);
/* xlz_7z_decode into DEVICE memory, as xlz_xz_decode_device: same status, *out_len and *unverified as xlz_7z_decode,
 * except that a folder of 4 GiB or more is XLZ_ERR_UNSUPPORTED.  A Copy folder is uploaded from the file; its CRC is
 * computed on the host over the file's bytes.  About twice the decoded size of device memory.  In bcj2 mode 1 / 2 the
 * streams of a BCJ2 folder join the one batch, the folder is merged into d_out behind the pack (xlz_batch_bcj2), and its
 * CRCs are computed by the check kernels over the destination.                                                     */
int xlz_7z_decode_device(xlz_ctx *ctx, const uint8_t *file, size_t len, void *d_out, size_t out_cap,
                         uint64_t *out_len, int verify, size_t *unverified);
/* the same over several contexts (one per GPU; encoded headers are decoded on the first)         */
int xlz_7z_decode_multi(xlz_ctx *const *ctxs, size_t n_ctx, const uint8_t *file, size_t len, uint8_t *out,
                        size_t out_cap, uint64_t *out_len, int verify, size_t *unverified);

/* ---- the files of a .7z archive: the table, and chosen files as ONE batch ----------------
 * xlz_7z_open parses the streams as xlz_7z_index_bcj2 does -- the same status for every input, the same folder list --
 * and then the FilesInfo section (7zFormat.txt): names, empty-stream / empty-file / anti bits, modification times and
 * Windows attributes; other properties are skipped.  ctx may be NULL for a plain header; an encoded header is decoded
 * on the device as ever.  An archive without FilesInfo has no entries; one whose FilesInfo has no names has entries
 * with empty names.  Refused: External data (XLZ_ERR_UNSUPPORTED); a property whose data does not fill, or overruns,
 * its announced size, a name pool that does not hold exactly one terminated name per entry, a number of entries with a
 * stream that is not the number of substreams, a byte behind the StreamsInfo that is neither FilesInfo nor the header's end
 * mark, a FilesInfo that the end mark does not follow (XLZ_ERR_RESULT).  These are all that xlz_7z_open refuses beyond
 * xlz_7z_index_bcj2, which never reads behind the StreamsInfo.  xlz_7z_index* and xlz_7z_decode* keep ignoring
 * FilesInfo: an archive with a broken one still decodes through them.  The handle BORROWS `file` until xlz_7z_close
 * and never changes after open: any number of threads and contexts may use one at once.  Open, close, info, entries,
 * folders, cover and layout are host only.
 *
 * Names are converted from UTF-16LE to UTF-8 (an unpaired surrogate becomes U+FFFD) and handed out AS STORED, each
 * NUL-terminated in one pool: no separator is normalised, no ".." removed, nothing is made relative.  The library
 * writes no files; A CALLER THAT DOES MUST NOT TRUST A NAME AS A PATH.
 *
 * The entries that have a stream map, in order, onto the substreams of the folders: entry -> (folder, folder_off, size,
 * crc).  An entry without a stream is a directory when it is not marked as an empty file.
 *
 * xlz_7z_cover: for the wanted entries, the ascending, duplicate-free folders that hold bytes of them, and how much of
 * each must be decoded.  With P = the largest folder_off + size over the wanted entries of a folder: an LZMA folder and
 * an LZMA2 folder of one unit are cut at P (decode_len = P, the input whole); an LZMA2 folder of several units
 * (xlz_lzma2_units) is cut at the end of the unit that holds byte P - 1, its INPUT too (in_len), so that it is still
 * launched unit-parallel; a folder with filter steps, a Copy folder, a BCJ2 folder and an unsupported one are never cut.
 * items may be NULL with max_items 0 to obtain the count; XLZ_ERR_OUT_CAP when a non-zero capacity is too small (the
 * count is still set).  xlz_7z_extract_layout sets wants[i].dst_cap = the entry's size and dst_off = the next multiple of
 * align (>= 1; 0: XLZ_ERR_BAD_ARG) behind the window before, *total = the end of the last window (XLZ_ERR_OUT_CAP: the
 * windows do not fit 64 bits; XLZ_ERR_BAD_ARG: an entry index outside the table).
 *
 * xlz_7z_extract_device: ONE batch of the covering folders (xlz_batch_create / run / results), then on the device the
 * filter steps (filter mode 1), the CRC32 of every wanted entry that has one as a range over its folder's stream
 * (verify != 0, whatever the check mode) and ONE pack of the wanted entries' bytes into their windows.  Entries of Copy
 * folders are uploaded from the file; their CRC is computed on the host over the file's bytes.  xlz_7z_extract: the
 * same through a staging block of the context's pool that holds the wanted sizes back to back, one download, and a
 * scatter into the windows; the block stays with the context until xlz_ctx_trim.
 *
 * Per wanted entry, in this order: XLZ_ERR_OUT_CAP -- dst_cap is smaller than the entry (the entry then asks nothing of
 * its folder); XLZ_ERR_UNSUPPORTED -- the folder's method is unsupported, it is a filter chain on a context in filter
 * mode 0, it is a BCJ2 folder (in any bcj2 mode), or the folder or its packed stream is 4 GiB or more, whatever its cut; the
 * folder's stream did not end as expected -- a whole folder: a status >= 0 with exactly its size; a folder cut by
 * capacity: XLZ_ERR_OUT_CAP with exactly decode_len bytes; a folder cut at a unit: XLZ_ERR_UNEXPECTED_EOF with exactly
 * decode_len bytes and all of in_len used --: the stream's own status where that is another negative one, else
 * XLZ_ERR_RESULT, for EVERY wanted entry of that folder (such a stream is left out of steps, ranges and pack);
 * XLZ_ERR_RESULT -- the entry's CRC differs: only that entry fails.  An entry without bytes is XLZ_OK with out_len 0,
 * whatever its window.  unverified = 1: verify is on and the entry has bytes but no CRC.  The same entry may be wanted
 * twice, into two windows.
 *
 * INVARIANT: an entry that is XLZ_OK in a call is XLZ_OK with the same bytes when it is extracted alone -- alone its
 * folder is cut no later.  The reverse does not hold: damage behind a folder's cut is not seen.
 *
 * The call returns XLZ_OK whenever it ran.  XLZ_ERR_BAD_ARG: NULL arguments with n > 0; an entry index outside the table;
 * a window of an entry with bytes that does not fit out_cap; two such windows that share a byte (these are tested
 * before the context is used; the window of an entry without bytes declares nothing); d_out that is not out_cap bytes of
 * device memory of the context's device.  Such a call launches nothing, writes nothing -- results[] included -- and
 * leaves every statistic as it was; an empty want list launches nothing either and is XLZ_OK.  Another negative status
 * (XLZ_ERR_DEVICE): the batch could not run, and every results[i].status is that status.  Bytes outside every window are
 * never written; inside the window of a good entry nothing behind out_len is written.                                 */
typedef struct xlz_7z_archive xlz_7z_archive;
#define XLZ_7Z_NO_FOLDER (~(uint64_t)0)
enum { XLZ_7Z_ENTRY_HAS_STREAM = 1, XLZ_7Z_ENTRY_HAS_CRC = 2, XLZ_7Z_ENTRY_IS_DIR = 4, XLZ_7Z_ENTRY_IS_ANTI = 8,
       XLZ_7Z_ENTRY_HAS_MTIME = 16, XLZ_7Z_ENTRY_HAS_ATTRIBUTES = 32 };
typedef struct xlz_7z_entry {  /* 64 bytes */
    uint64_t size;       /* 0 without a stream                                                             */
    uint64_t folder;     /* index into the folders; XLZ_7Z_NO_FOLDER without a stream                      */
    uint64_t folder_off; /* where its bytes begin inside the folder's decoded bytes                        */
    uint64_t substream;  /* index into the substreams of xlz_7z_index*; XLZ_7Z_NO_FOLDER without a stream  */
    uint64_t mtime;      /* raw FILETIME: 100 ns since 1601-01-01 UTC (XLZ_7Z_ENTRY_HAS_MTIME)             */
    uint64_t name_off;   /* into the name pool: UTF-8, NUL-terminated                                      */
    uint32_t name_len;   /* bytes, without the NUL                                                         */
    uint32_t crc;        /* CRC32 of its bytes (XLZ_7Z_ENTRY_HAS_CRC)                                      */
    uint32_t attributes; /* Windows attributes (XLZ_7Z_ENTRY_HAS_ATTRIBUTES)                               */
    uint32_t flags;      /* XLZ_7Z_ENTRY_*                                                                 */
} xlz_7z_entry;
typedef struct xlz_7z_want {
    uint64_t entry;      /* index into the entries                                                         */
    uint64_t dst_off;    /* its window [dst_off, dst_off + dst_cap) in the destination                     */
    uint64_t dst_cap;
} xlz_7z_want;
typedef struct xlz_7z_file_result {
    int32_t status;
    uint32_t unverified; /* 1: verify was on, the entry has bytes and no CRC (0 unless status == XLZ_OK)   */
    uint64_t out_len;    /* bytes at dst_off; 0 unless status == XLZ_OK                                    */
} xlz_7z_file_result;
typedef struct xlz_7z_cover_item {
    uint64_t folder;
    uint64_t decode_len; /* how much of the folder's bytes the batch is asked for                          */
    uint64_t in_len;     /* how much of its packed stream goes into the batch                              */
} xlz_7z_cover_item;
int xlz_7z_open(xlz_ctx *ctx, const uint8_t *file, size_t len, xlz_7z_archive **a);
void xlz_7z_close(xlz_7z_archive *a);
/* every pointer but `a` may be NULL.  name_bytes: the size of the name pool; total_size: the sum of the entries' sizes  */
int xlz_7z_archive_info(const xlz_7z_archive *a, size_t *n_entries, size_t *n_folders, size_t *name_bytes,
                        uint64_t *total_size);
/* at most max_entries entries and names_cap bytes of the pool are copied; XLZ_ERR_OUT_CAP: there are more of either   */
int xlz_7z_archive_entries(const xlz_7z_archive *a, xlz_7z_entry *entries, size_t max_entries, char *names,
                           size_t names_cap);
/* the folders as xlz_7z_index_bcj2 lists them; XLZ_ERR_OUT_CAP: more than max_folders                                  */
int xlz_7z_archive_folders(const xlz_7z_archive *a, xlz_7z_folder *folders, size_t max_folders);
int xlz_7z_cover(const xlz_7z_archive *a, const uint64_t *entries, size_t n, xlz_7z_cover_item *items, size_t max_items,
                 size_t *n_items);
int xlz_7z_extract_layout(const xlz_7z_archive *a, xlz_7z_want *wants, size_t n, uint64_t align, uint64_t *total);
int xlz_7z_extract(xlz_ctx *ctx, const xlz_7z_archive *a, const xlz_7z_want *wants, size_t n, uint8_t *out,
                   size_t out_cap, int verify, xlz_7z_file_result *results);
int xlz_7z_extract_device(xlz_ctx *ctx, const xlz_7z_archive *a, const xlz_7z_want *wants, size_t n, void *d_out,
                          size_t out_cap, int verify, xlz_7z_file_result *results);
/* Of the most recent xlz_7z_extract / xlz_7z_extract_device on `ctx` that ran: one that passed its argument tests and had a
 * want list that is not empty.  Such a call starts the check, filter and pack statistics over, fills them, and publishes
 * these at its end -- also when the device then failed it (XLZ_ERR_DEVICE: failed_entries == entries, copied_bytes 0). */
typedef struct xlz_7z_extract_stats {
    uint64_t entries, empty_entries; /* as wanted; of them without bytes                                  */
    uint64_t failed_entries;         /* with a status other than XLZ_OK                                   */
    uint64_t folders, comp_bytes;    /* the cover of the entries that asked for their folder (Copy folders
                                        included), and what goes in of their packed streams (in_len)       */
    uint64_t decoded_bytes;          /* what the batch was asked to decode of them (the sum of decode_len) */
    uint64_t folder_bytes;           /* their full sizes: folder_bytes - decoded_bytes is what the cuts saved */
    uint64_t copied_bytes;           /* the sum of out_len                                                */
} xlz_7z_extract_stats;
int xlz_ctx_last_7z_extract_stats(xlz_ctx *ctx, xlz_7z_extract_stats *out);

/* ---- the members of a .tar image, in host or device memory -----------------------------
 * Outside the reference (which has no tar code).  Almost every .xz file is a tarball; decoded into device memory
 * (xlz_xz_decode_device) it is one flat image, and where its members lie follows from a chain of headers, each of which
 * says where the next one is.  xlz_tar_scan_device finds them without downloading the image and without one round trip per
 * member: a kernel classifies every 512-byte block in HBM by its checksum field (lzma_amd/csrc/xlz_tar_dev.h: zero /
 * header candidate / other), the flags (len / 512 bytes) and then the candidate blocks alone come to the host, the host
 * walks the chain over them (lzma_amd/csrc/xlz_tar_walk.h), a second gather fetches the data of the meta entries the walk
 * met (GNU long names, pax records), and the walk is finished.  Candidates that are file data -- a tar stored inside the
 * tar -- are downloaded but never reached; if every block is a candidate the download equals the image: correct, slow,
 * and visible in xlz_tar_stats.  The image is only read.  xlz_tar_parse_host is the same walk over a host image, no
 * device needed; both give the same table, end_status and end_off for the same bytes.
 *
 * The table is what Python's tarfile.getmembers() reports: per member its name and link name (bytes AS STORED, each
 * NUL-terminated in one pool: A CALLER THAT WRITES FILES MUST NOT TRUST A NAME AS A PATH), size, type ('0' for a regular
 * file, '5' a directory, '1' / '2' hard and symbolic links, ...; a '\0' type is reported as it is, or as '5' when the
 * name ends in '/'), mode, uid, gid, mtime, hdr_off (the offset of its header, or of the first GNU long-name / pax
 * header in front of it: tarfile's offset) and data_off (offset_data).  On the device a member is bytes
 * [data_off, data_off + size) of the image, 512-aligned: a view, no copy.  ustar, GNU ('L' / 'K' long names, base-256
 * numbers) and pax ('x' / 'g' records: path, linkpath, size, mtime, uid, gid) archives are read; the rules are at the head
 * of xlz_tar_walk.h.
 *
 * A call returns XLZ_OK whenever the walk ran; how the walk ENDED is end_status: XLZ_OK (a zero block, or the image's end
 * at a header position); XLZ_ERR_UNEXPECTED_EOF (the image ends inside a header or inside a member's data);
 * XLZ_ERR_RESULT (a block that is no header where one must be, a malformed number or pax record, meta data over 1 MiB);
 * XLZ_ERR_UNSUPPORTED (old GNU sparse 'S', multi-volume 'M', GNU.sparse.* pax keys).  The members in front of that
 * place stay in the table, end_off is the offset of the header where the walk stopped.
 *
 * XLZ_ERR_BAD_ARG: out is NULL; image is NULL with len > 0; ctx is NULL; d_image is not a multiple of 16 (device memory
 * from hipMalloc and torch is) or not len bytes of device memory of the context's device.  len < 512 launches nothing.
 * xlz_xz_tar_list: the whole of an open .xz file (xlz_xz_open) decoded into device scratch from the context's pool by
 * xlz_xz_read_device for [0, size) -- the same checks, filters, statuses and *unverified as that call --, scanned, and
 * the scratch given back: the listing of a .tar.xz.  Its members are then read with xlz_xz_read / xlz_xz_read_device over
 * (data_off, size), which decode only the blocks that hold them.                                                   */
typedef struct xlz_tar xlz_tar;
typedef struct xlz_tar_entry { /* 72 bytes */
    uint64_t hdr_off, data_off, size;
    int64_t mtime_s;     /* whole seconds since 1970-01-01 UTC (floor)                                     */
    uint32_t mtime_ns;   /* a pax mtime's fraction; 0 otherwise                                            */
    uint32_t mode, uid, gid;
    uint32_t name_off, name_len, link_off, link_len; /* into the name pool, lengths without the NUL        */
    uint8_t type;
    uint8_t reserved[7];
} xlz_tar_entry;
int xlz_tar_parse_host(const void *image, uint64_t len, xlz_tar **out);
int xlz_tar_scan_device(xlz_ctx *ctx, const void *d_image, uint64_t len, xlz_tar **out);
int xlz_xz_tar_list(xlz_ctx *ctx, const xlz_xz_file *f, int verify, xlz_tar **out, size_t *unverified);
/* every pointer but `t` may be NULL */
void xlz_tar_info(const xlz_tar *t, size_t *n_entries, size_t *name_bytes, int *end_status, uint64_t *end_off);
/* at most cap entries and names_cap bytes of the pool are copied; XLZ_ERR_OUT_CAP: there are more of either */
int xlz_tar_entries(const xlz_tar *t, xlz_tar_entry *e, size_t cap, void *names, size_t names_cap);
void xlz_tar_close(xlz_tar *t);
/* Of the most recent xlz_tar_scan_device / xlz_xz_tar_list on `ctx` whose scan ran.                        */
typedef struct xlz_tar_stats {
    uint64_t blocks;           /* complete 512-byte blocks of the image                                    */
    uint64_t zero_blocks;      /* flag 2                                                                   */
    uint64_t candidate_blocks; /* flag 1: gathered and downloaded                                          */
    uint64_t header_blocks;    /* headers the walk reached (meta entries included)                         */
    uint64_t meta_bytes;       /* data blocks of meta entries, gathered and downloaded                     */
    uint64_t downloaded_bytes; /* flags + candidate blocks + meta blocks                                   */
    double kernel_ms;          /* the classify and gather kernels by HIP events                            */
    uint32_t launches;
    uint32_t reserved;
} xlz_tar_stats;
int xlz_ctx_last_tar_stats(xlz_ctx *ctx, xlz_tar_stats *s);

/* ---- the entries of a .zip archive: the table, and chosen entries as ONE batch -----------
 * Outside the reference (which has no ZIP code; Go callers register it with archive/zip for method 14 and are then
 * called once per entry).  Every entry of a ZIP archive is a stream of its own, so an archive written with method 14
 * (LZMA: 7-Zip -tzip -mm=LZMA, WinZip .zipx, Python's zipfile.ZIP_LZMA) is thousands of independent LZMA1 streams, each
 * with a known size and a CRC32: the shape the decoder is built for, with nothing to be found first.  Written from
 * PKWARE's APPNOTE.TXT; the parser is lzma_amd/csrc/xlz_zip.h.
 *
 * xlz_zip_open (host only, no context) finds the end record -- the last PK\5\6 of the last 65 557 bytes at a position p
 * with p + 22 + comment_len <= len, so bytes behind the comment are tolerated --, follows a ZIP64 locator 20 bytes in front
 * of it to the ZIP64 end record (where the locator says, else right in front of the locator) and takes counts, size and
 * offset from there; takes the central directory to end where that end record begins, so that
 * shift = cd_pos_found - cd_offset_declared is the number of bytes in front of the archive (self-extractor stubs), added
 * to every local header offset (an all-ones declared offset without a ZIP64 end record, as Info-ZIP's zip -fz writes it,
 * tells nothing: shift = 0); and walks the central directory.  Per record it reads method, general-purpose flags, DOS
 * time and date, CRC32, sizes, name, local header offset, external attributes and the ZIP64 extra field (0x0001: the
 * values that are all-ones in the record, in the order size, compressed size, offset); other extra fields and the entry
 * comment are skipped.  It fails with XLZ_ERR_UNSUPPORTED for a multi-disk archive (a disk number other than 0, entry
 * counts that differ), XLZ_ERR_UNEXPECTED_EOF for a file shorter than an end record or a central directory that is cut
 * (longer than what lies in front of the end record, or a record that leaves it), XLZ_ERR_RESULT where there is no end
 * record, a locator leads to no ZIP64 end record, the directory would begin in front of its declared offset, a record has
 * another signature, or the announced number of records does not fill the directory's size exactly.  Nothing else fails
 * it: what is wrong with ONE entry is that entry's class.
 *
 * Every entry is resolved against its LOCAL header at open: that header must lie inside the file and carry PK\3\4,
 * data_off = header_off + 30 + the local header's OWN name and extra lengths, and [data_off, data_off + comp_size) must
 * lie in front of the central directory.  Sizes and CRC are the central directory's only (an entry written with a data
 * descriptor, flag bit 3, has zeros in its local header).  A method-14 payload is 2 version bytes, a 2-byte little-endian
 * property size that must be 5, the lc/lp/pb byte (< 225), a 4-byte dictionary size, then the raw stream; flag bit 1 says
 * whether that stream ends in an end marker (decoded with the size unknown and out_cap = size) or at `size` (decoded with
 * unpack_size = size).  The classes, fixed at open:
 *   supported    method 0 (stored), or method 14 and well formed: XLZ_ZIP_ENTRY_SUPPORTED
 *   unsupported  any other method (deflate 8, bzip2 12, xz 95, ...); encrypted (flag bit 0 or 6); patched data (bit 5);
 *                method 0 with comp_size != size; a size or a payload above 0xFFFF0000 bytes ("4 GiB": what a unit's
 *                32-bit counters hold): neither bit
 *   bad          the local header is out of the file or without signature, or the ZIP64 extra field is too short
 *                (data_off = 0); the data is out of bounds; the LZMA header is malformed (comp_size < 9, a property size
 *                other than 5, a props byte >= 225): XLZ_ZIP_ENTRY_BAD
 *   deflate      XLZ_ZIP_ENTRY_DEFLATE, a bit of its own beside the classes, which are set exactly as above (a deflate
 *                entry is unsupported: neither bit): method 8, not encrypted or patched, local header and data in bounds,
 *                size and payload below 0xFFFF0000 bytes.  Method 9 (Deflate64) never has it.
 * A directory is an entry whose name ends in '/'; it has no bytes, whatever its fields say.  The handle BORROWS `file`
 * until xlz_zip_close and never changes after open: any number of threads and contexts may use one at once.
 *
 * Names are handed out AS STORED, each NUL-terminated in one pool (UTF-8 where XLZ_ZIP_ENTRY_UTF8 is set, else by
 * convention code page 437): no separator is normalised, no ".." removed.  The library writes no files; A CALLER THAT
 * DOES MUST NOT TRUST A NAME AS A PATH.
 *
 * xlz_zip_extract_layout sets wants[i].dst_cap = the entry's size (0 for one without bytes) and dst_off = the next
 * multiple of align (>= 1; 0: XLZ_ERR_BAD_ARG) behind the window before, in want order, *total = the end of the last window
 * (XLZ_ERR_OUT_CAP: the windows do not fit 64 bits; XLZ_ERR_BAD_ARG: an entry index outside the table).
 *
 * xlz_zip_extract_device: the wanted method-14 entries are ONE batch (xlz_batch_create / run / results) whose
 * descriptors point INTO the file image (in = file + data_off + 9, in_len = comp_size - 9): one decode launch sequence,
 * however many entries.  With verify != 0 the CRC32 of every wanted entry is computed on the device by the check kernels,
 * whatever the context's check mode: a method-14 entry as a range over its stream, a stored entry over its bytes where
 * they lie in the destination.  ONE pack writes the method-14 entries into their windows.  Stored entries do not go up
 * one copy each: host threads gather their bytes into ONE pinned staging block of the context's pool, each at an offset
 * congruent to its destination modulo 16, the block goes up in one transfer together with its item table, and the pack
 * kernel scatters it with the block as its source.  A block holds up to 256 MiB of stored bytes (one entry above that
 * has a block to itself); xlz_zip_extract_stats::stored_uploads counts the transfers, 1 for anything smaller and never
 * growing with the number of entries.  xlz_zip_extract: the same steps into a staging block of the context's pool that
 * holds the wanted sizes back to back, one download, and a scatter of the good entries into the windows.
 *
 * Per wanted entry, in this order: an entry without bytes (a directory, size 0 -- a size-0 method-14 entry is not
 * launched) is XLZ_OK with out_len 0, whatever its window and class; XLZ_ERR_OUT_CAP -- dst_cap is smaller than the entry
 * (it then asks nothing of the batch); XLZ_ERR_UNSUPPORTED -- an unsupported entry; XLZ_ERR_RESULT -- a bad entry; the
 * stream did not end with a status >= 0 and exactly `size` bytes: the stream's own status where that is negative, else
 * XLZ_ERR_RESULT -- XLZ_ERR_OUT_CAP from an end-marker stream, which only wanted to go on behind the declared size, is
 * reported as XLZ_ERR_RESULT -- and such a stream is left out of ranges and pack; XLZ_ERR_RESULT -- the CRC32 differs.
 * out_len is 0 unless the status is XLZ_OK.  The same entry may be wanted twice, into two windows.
 *
 * INVARIANT: an entry's result in a call of many equals its result when it is extracted alone.
 *
 * The call returns XLZ_OK whenever it ran.  XLZ_ERR_BAD_ARG: NULL arguments with n > 0; an entry index outside the table;
 * a window of an entry with bytes that does not fit out_cap; two such windows that share a byte (these are tested
 * before the context is used; the window of an entry without bytes declares nothing); d_out that is not out_cap bytes of
 * device memory of the context's device.  Such a call launches nothing, writes nothing -- results[] included -- and
 * leaves every statistic as it was; an empty want list launches nothing either and is XLZ_OK.  Another negative status
 * (XLZ_ERR_DEVICE): the call could not run, and every results[i].status is that status.  Bytes outside every window are
 * never written; inside the window of a good entry nothing behind out_len is written.  The window of an entry that failed
 * is untouched in the host form; in the device form it is untouched too unless the entry failed by its CRC32 alone, which
 * is known only when its bytes lie there.  xlz_batch_advice tells when a handful of entries is the host's job; there is
 * no fallback in here.
 *
 * DEFLATE ENTRIES (xlz_ctx_set_deflate_mode; 0, the default: everything above, a deflate entry is XLZ_ERR_UNSUPPORTED).
 * In deflate mode 1 / 2 a wanted XLZ_ZIP_ENTRY_DEFLATE entry is an item of xlz_inflate_batch's machinery in the same call,
 * behind the LZMA batch and the stored scatter and in front of the CRC32s: mode 1 on the device, mode 2 on host threads;
 * in the device form written straight into its window, in the host form into the staging block.  With verify its CRC32
 * is taken by the check kernels over the bytes where they lie, as for a stored entry.  Its verdict, in this order: what
 * settles an entry before the batch, as above (XLZ_ERR_OUT_CAP for a window smaller than the entry); the inflate status
 * where it is negative -- XLZ_ERR_OUT_CAP, which only says that the stream wanted to go on behind the declared size, as
 * XLZ_ERR_RESULT, as for end-marker streams --; XLZ_ERR_RESULT unless exactly `size` bytes were produced; XLZ_ERR_RESULT
 * when the CRC32 differs.  The INVARIANT holds for them.  The one difference: in the device form the window of a deflate
 * entry that FAILED holds unspecified bytes, because it was decoded in place.  xlz_zip_extract_stats keeps its layout:
 * entries, failed_entries, comp_bytes and copied_bytes count deflate entries, lzma_entries and stored_entries do not; the
 * rest is in xlz_ctx_last_inflate_stats.                                                                              */
typedef struct xlz_zip_archive xlz_zip_archive;
enum { XLZ_ZIP_ENTRY_SUPPORTED = 1, XLZ_ZIP_ENTRY_IS_DIR = 2, XLZ_ZIP_ENTRY_UTF8 = 4, XLZ_ZIP_ENTRY_ENCRYPTED = 8,
       XLZ_ZIP_ENTRY_HAS_DESCRIPTOR = 16, XLZ_ZIP_ENTRY_ZIP64 = 32, XLZ_ZIP_ENTRY_BAD = 64, XLZ_ZIP_ENTRY_END_MARKER = 128,
       XLZ_ZIP_ENTRY_DEFLATE = 256 };
typedef struct xlz_zip_entry { /* 72 bytes (the fields do not fit 64) */
    uint64_t size, comp_size;      /* from the central directory                                           */
    uint64_t header_off, data_off; /* shifted; data_off = 0 for a BAD entry whose header is unusable       */
    uint64_t name_off;             /* into the name pool: bytes AS STORED, NUL-terminated                  */
    uint32_t name_len, crc;        /* name_len: bytes, without the NUL                                     */
    uint32_t dos_time_date;        /* time in the low, date in the high half                               */
    uint32_t external_attr;
    uint32_t dict_size;            /* method 14, well formed                                               */
    uint16_t method, gp_flags;
    uint8_t props, reserved[3];    /* props: method 14, well formed: the lc/lp/pb byte                     */
    uint32_t flags;                /* XLZ_ZIP_ENTRY_*                                                      */
} xlz_zip_entry;
typedef struct xlz_zip_want {
    uint64_t entry;                /* index into the entries                                               */
    uint64_t dst_off, dst_cap;     /* its window [dst_off, dst_off + dst_cap) in the destination           */
} xlz_zip_want;
typedef struct xlz_zip_file_result {
    int32_t status;
    uint32_t reserved;
    uint64_t out_len;              /* bytes at dst_off; 0 unless status == XLZ_OK                          */
} xlz_zip_file_result;
int xlz_zip_open(const uint8_t *file, size_t len, xlz_zip_archive **a); /* host only; the file must outlive a */
void xlz_zip_close(xlz_zip_archive *a);
/* every pointer but `a` may be NULL.  name_bytes: the size of the name pool; total_size: the sum of the sizes of the
 * entries that have bytes; shift: the bytes in front of the archive                                                  */
int xlz_zip_archive_info(const xlz_zip_archive *a, size_t *n_entries, size_t *name_bytes, uint64_t *total_size,
                         uint64_t *shift);
/* at most max_entries entries and names_cap bytes of the pool are copied; XLZ_ERR_OUT_CAP: there are more of either   */
int xlz_zip_archive_entries(const xlz_zip_archive *a, xlz_zip_entry *entries, size_t max_entries, char *names,
                            size_t names_cap);
int xlz_zip_extract_layout(const xlz_zip_archive *a, xlz_zip_want *wants, size_t n, uint64_t align, uint64_t *total);
int xlz_zip_extract(xlz_ctx *ctx, const xlz_zip_archive *a, const xlz_zip_want *wants, size_t n, uint8_t *out,
                    size_t out_cap, int verify, xlz_zip_file_result *results);
int xlz_zip_extract_device(xlz_ctx *ctx, const xlz_zip_archive *a, const xlz_zip_want *wants, size_t n, void *d_out,
                           size_t out_cap, int verify, xlz_zip_file_result *results);
/* Of the most recent xlz_zip_extract / xlz_zip_extract_device on `ctx` that ran: one that passed its argument tests and
 * had a want list that is not empty.  Such a call starts the check and pack statistics over, fills them (the scatter of
 * the stored entries counts as a pack launch), and publishes these at its end -- also when the device then failed it
 * (XLZ_ERR_DEVICE: failed_entries == entries, copied_bytes 0).                                                       */
typedef struct xlz_zip_extract_stats {
    uint64_t entries, empty_entries; /* as wanted; of them without bytes                                  */
    uint64_t failed_entries;         /* with a status other than XLZ_OK                                   */
    uint64_t lzma_entries;           /* method-14 streams given to the batch                              */
    uint64_t stored_entries;         /* stored entries gathered, uploaded and scattered                   */
    uint64_t comp_bytes;             /* payload bytes of both kinds read from the file (comp_size)        */
    uint64_t copied_bytes;           /* the sum of out_len                                                */
    uint32_t stored_uploads;         /* host-to-device transfers made for the stored entries              */
    uint32_t reserved;
} xlz_zip_extract_stats;
int xlz_ctx_last_zip_extract_stats(xlz_ctx *ctx, xlz_zip_extract_stats *out);

/* ---- Adler-32 of ranges of a device buffer (lzma_amd/csrc/xlz_adler_dev.hip) ----
 * RFC 1950 section 8.2: A = 1 + the sum of the bytes, B = the sum of the running A, both mod 65521; the digest is
 * B << 16 | A.  The scheme (rows of 64 lanes x 16 bytes, one wave per segment of 128 KiB, a fold by the combine rule) and
 * how long the modulo is deferred are at the head of lzma_amd/csrc/xlz_adler_dev.h.                                    */
typedef struct xlz_adler_range { uint64_t off, len; } xlz_adler_range;
/* Adler-32 of n ranges of a device buffer of the context's device, digests[i] for ranges[i]; the ranges may overlap and
 * come in any order, they start and end at any byte, d_buf needs no alignment; a range of length 0 has the digest 1.  No
 * byte outside a range is read.  The call waits for its kernels.  XLZ_ERR_BAD_ARG: a NULL argument with n > 0; a range
 * outside [0, buf_len); d_buf is not device memory of the context's device, or buf_len reaches past its allocation.
 * XLZ_ERR_UNSUPPORTED: more than 2^32 - 1 ranges or segments (512 TiB) in one call.  n = 0 is XLZ_OK.                     */
int xlz_adler32_device(xlz_ctx *ctx, const void *d_buf, size_t buf_len, const xlz_adler_range *ranges, size_t n, uint32_t *digests);
/* Host only.  The digest of `adler`'s bytes followed by p[0 .. n) (adler = 1: of p alone) ...                           */
uint32_t xlz_adler32_host(uint32_t adler, const uint8_t *p, size_t n);
/* ... and adler32(A || B) from a = adler32(A), b = adler32(B) and len_b = |B|, like xlz_crc32_combine.                  */
uint32_t xlz_adler32_combine(uint32_t a, uint32_t b, uint64_t len_b);

/* ---- gzip files, BGZF files and zlib streams as one batch (lzma_amd/csrc/xlz_gz.h, xlz_gz.hip) ----
 * A gzip file (RFC 1952) is one or more members; a BGZF file (bgzip, BAM, tabix) is a gzip file whose every member
 * announces its own size, so that all of its blocks are known without inflating a byte; a zlib stream (RFC 1950) is one
 * deflate stream with a two-byte header and an Adler-32 behind it.  The formats, what is which status and the verdict
 * are described at the head of lzma_amd/csrc/xlz_gz.h:
 *   XLZ_ERR_RESULT          wrong magic, a bad zlib header, bytes that are neither zero nor a member behind a member, invalid
 *                           deflate data, a size or check value that differs, ANY failure of a BGZF block
 *   XLZ_ERR_UNSUPPORTED     a compression method other than 8, a reserved FLG bit, a zlib stream that wants a dictionary
 *   XLZ_ERR_UNEXPECTED_EOF  the input ends inside a header, a deflate stream or a trailer
 *   XLZ_ERR_OUT_CAP         the file decodes to more than its dst_cap
 * WHAT THIS MAKES FAST, and what not: every stream is inflated by ONE wave (xlz_inflate_batch's machinery), and a lone wave
 * is slower than a host core.  BGZF files and batches of many files or streams fill the device; one ordinary
 * single-member .gz of a large file is the host's job -- a member above the launch-length cap goes to host threads anyway
 * -- and stays so.                                                                                                   */
enum { XLZ_GZ_AUTO = 0, XLZ_GZ_GZIP = 1, XLZ_GZ_ZLIB = 2 }; /* AUTO: 1f 8b -> gzip, else a valid zlib header -> zlib, else
                                                               XLZ_ERR_RESULT (fewer than 2 bytes: XLZ_ERR_UNEXPECTED_EOF) */
enum { XLZ_GZ_F_BGZF = 1, XLZ_GZ_F_NAME = 2, XLZ_GZ_F_COMMENT = 4, XLZ_GZ_F_HCRC = 8 };
typedef struct xlz_gz_info {
    uint32_t format, flags; /* resolved format; flags of the first member                                         */
    uint64_t members;       /* BGZF: blocks, empty ones included; otherwise 0 = not known before decoding          */
    uint64_t size_hint;     /* BGZF: the sum of the blocks' ISIZE (exact for a sound file); gzip: the last four bytes
                               (what gzip -l prints: exact for ONE member below 4 GiB); zlib: 0                    */
    uint32_t mtime;         /* of the first member                                                                */
    uint32_t name_off, name_len; /* its FNAME inside the input, without the zero byte (XLZ_GZ_F_NAME)             */
    uint32_t reserved;
} xlz_gz_info;
/* Host only: what the headers say (no FHCRC is compared, nothing is inflated).  -> XLZ_OK or the header's status;
 * XLZ_ERR_BAD_ARG: out is NULL, in is NULL with in_len > 0, an unknown format.                                        */
int xlz_gz_probe(const uint8_t *in, size_t in_len, uint32_t format, xlz_gz_info *out);
typedef struct xlz_gz_file {
    const uint8_t *in;  /* host memory: the file or stream                                                        */
    uint64_t in_len;
    uint64_t dst_off;   /* its window in the destination                                                          */
    uint64_t dst_cap;
    uint32_t format;    /* XLZ_GZ_AUTO / _GZIP / _ZLIB                                                            */
    uint32_t reserved;
} xlz_gz_file;
typedef struct xlz_gz_result {
    int32_t status;
    uint32_t members;     /* members or BGZF blocks that were inflated                                            */
    uint64_t out_len;     /* bytes at dst_off; 0 unless status == XLZ_OK (the window then holds unspecified bytes) */
    uint64_t in_consumed; /* gzip: in_len; zlib: where the trailer ended; 0 unless status == XLZ_OK               */
} xlz_gz_result;
/* Host only, the serial twin: one file into host memory.  The call returns XLZ_OK whenever it ran, the file's outcome is
 * *r.  XLZ_ERR_BAD_ARG: r is NULL, a NULL pointer with a length behind it, an unknown format.                          */
int xlz_gz_decode_host(const uint8_t *in, size_t in_len, uint32_t format, uint8_t *out, size_t out_cap, int verify, xlz_gz_result *r);
/* Many files as ONE batch into one caller-owned device buffer.  ROUND 1 inflates every block of every BGZF file, the first
 * member of every ordinary gzip file and every zlib stream as the items of one xlz_inflate_batch run (one gathered upload
 * below 256 MiB, one launch sequence; items above the launch-length cap, and all of them in deflate mode 2, on host
 * threads); round k inflates member k of the ordinary gzip files that still have one -- it begins where member k - 1
 * ended, so a file of m ordinary members costs m rounds.  With verify on, the CRC32 of every gzip member goes through the
 * check kernels and the Adler-32 of every zlib stream through xlz_adler32_device's kernels, over the destination: only
 * digests leave the device.  results[i] is what file i gets when it is passed alone; one bad file never fails the call,
 * which returns XLZ_OK whenever it ran.  Like xlz_inflate_batch the call does not look at whether the deflate mode is 0.
 * XLZ_ERR_BAD_ARG, with nothing written: NULL arguments with n > 0; a file without a pointer to its length; a window that
 * does not fit dst_cap, two windows that share a byte; an unknown format; d_dst is not device memory of the context's
 * device.  n = 0 is XLZ_OK.  Nothing outside the files' windows is written.                                          */
int xlz_gz_decode_many_device(xlz_ctx *ctx, const xlz_gz_file *files, size_t n, void *d_dst, size_t dst_cap, int verify, xlz_gz_result *results);
/* The same into host memory: the windows lie back to back in one staging block of the context's pool, which comes down
 * in ONE copy; only the good files are scattered into dst.                                                           */
int xlz_gz_decode_many(xlz_ctx *ctx, const xlz_gz_file *files, size_t n, uint8_t *dst, size_t dst_cap, int verify, xlz_gz_result *results);
/* Of the most recent xlz_gz_decode_many / xlz_gz_decode_many_device on `ctx` that ran.                                */
typedef struct xlz_gz_stats {
    uint64_t files, failed_files, bgzf_files;
    uint64_t members;                  /* members and BGZF blocks inflated                                        */
    uint64_t device_items, host_items; /* by the kernel; on host threads                                          */
    uint64_t crc_ranges, adler_ranges; /* members / streams whose digest was formed (verify on; an empty one's on the host) */
    uint32_t rounds, uploads;          /* inflate runs; transfers of gathered inputs                              */
    double adler_kernel_ms;
} xlz_gz_stats;
int xlz_ctx_last_gz_stats(xlz_ctx *ctx, xlz_gz_stats *out);

/* ---- .bz2 files as one batch (lzma_amd/csrc/xlz_bz2_dev.h, xlz_bz2.h, xlz_bz2.hip) ----
 * A .bz2 file is one or more streams, each a chain of independent blocks of at most level x 100 000 bytes; every block
 * opens with a 48-bit magic that is found at any bit offset without decoding anything, so ONE large file is a batch of
 * blocks, as many files are.  The format, the lane scheme and which defect is which status are at the head of
 * xlz_bz2_dev.h; the scan, the chain rule and the verdict at the head of xlz_bz2.h.  A file's outcome is that of a serial
 * reader which joins concatenated streams:
 *   XLZ_ERR_RESULT          a defect in the first stream: a bad header, a damaged block, a CRC that differs
 *   XLZ_ERR_UNSUPPORTED     a randomised block in the first stream
 *   XLZ_ERR_UNEXPECTED_EOF  the input ends inside a stream with no defect in front of the end
 *   XLZ_ERR_OUT_CAP         the file decodes to more than its dst_cap: out_len is then THE TRUE DECODED SIZE (a .bz2 file
 *                           does not state it), nothing of the file was written in a call of one round, and the caller
 *                           retries once with exact room
 *   XLZ_OK                  also when, behind at least one complete stream, a stream with a defect was IGNORED together
 *                           with everything behind it: in_consumed is the end of the last good stream and shows it
 * WHAT THIS MAKES FAST, and what not: every block is decoded by ONE wave, and a lone wave is much slower than a host core.
 * Files of many blocks and batches of many files fill the device; a file of a few blocks is the host's job.            */
typedef struct xlz_bz2_info {
    uint32_t level, reserved; /* of the first stream: '1'..'9'                                                        */
    uint64_t candidates;      /* block magics found, at any bit offset: an upper bound of the blocks                   */
    uint64_t streams;         /* end magics found                                                                     */
    uint64_t size_hint;       /* candidates x level x 100 000: what the file decodes to at most when no run was folded  */
    uint64_t size_bound;      /* what it can decode to at all: every block all runs of 255 + 4                          */
} xlz_bz2_info;
/* Host only: the first header and the scan, nothing decoded.  -> XLZ_OK, XLZ_ERR_UNEXPECTED_EOF (fewer than 4 bytes),
 * XLZ_ERR_RESULT (no "BZh1".."BZh9"); XLZ_ERR_BAD_ARG: out is NULL, in is NULL with in_len > 0.                        */
int xlz_bz2_probe(const uint8_t *in, size_t in_len, xlz_bz2_info *out);
typedef struct xlz_bz2_file {
    const uint8_t *in; /* host memory: the file                                                                       */
    uint64_t in_len;
    uint64_t dst_off;  /* its window in the destination                                                               */
    uint64_t dst_cap;
} xlz_bz2_file;
typedef struct xlz_bz2_result {
    int32_t status;
    uint32_t blocks;      /* blocks of the kept streams                                                               */
    uint64_t out_len;     /* bytes at dst_off (XLZ_OK); the true decoded size (XLZ_ERR_OUT_CAP); else 0                */
    uint64_t in_consumed; /* where the last kept stream ended; 0 unless status == XLZ_OK                              */
    uint32_t streams;     /* kept streams                                                                             */
    uint32_t reserved;
} xlz_bz2_result;
/* Host only, the serial twin: one file into host memory.  The call returns XLZ_OK whenever it ran, the file's outcome is
 * *r.  XLZ_ERR_BAD_ARG: r is NULL, a NULL pointer with a length behind it.                                             */
int xlz_bz2_decode_host(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap, int verify, xlz_bz2_result *r);
/* Many files as ONE batch into one caller-owned device buffer: one gathered upload of the file images; the block
 * candidates of ALL files are one run of the symbol and the walk kernels (rounds of it when their scratch, about 6 bytes
 * per block byte, exceeds xlz_ctx_set_bz2_scratch); after one small download the host settles every file's chain and the
 * blocks' offsets; one launch expands the chain's blocks straight into the windows and one forms their CRCs over the
 * destination.  Only statuses, lengths and digests leave the device.  Blocks above the launch-length cap, and every block
 * in bz2 mode 2, are decoded on host threads and uploaded.  results[i] is what file i gets when it is passed alone; one bad
 * file never fails the call, which returns XLZ_OK whenever it ran.  The call does not look at whether the bz2 mode is 0.
 * XLZ_ERR_BAD_ARG, with nothing written: NULL arguments with n > 0; a file without a pointer to its length; a window that
 * does not fit dst_cap, two windows that share a byte; d_dst is not device memory of the context's device.  n = 0 is
 * XLZ_OK.  Nothing outside the files' windows is written.                                                             */
int xlz_bz2_decode_many_device(xlz_ctx *ctx, const xlz_bz2_file *files, size_t n, void *d_dst, size_t dst_cap, int verify, xlz_bz2_result *results);
/* The same into host memory: the windows lie back to back in one staging block of the context's pool, which comes down
 * in ONE copy; only the good files are scattered into dst.                                                           */
int xlz_bz2_decode_many(xlz_ctx *ctx, const xlz_bz2_file *files, size_t n, uint8_t *dst, size_t dst_cap, int verify, xlz_bz2_result *results);
/* Of the most recent xlz_bz2_decode_many / xlz_bz2_decode_many_device on `ctx` that ran.                              */
typedef struct xlz_bz2_stats {
    uint64_t files, failed_files;
    uint64_t candidates, chain_blocks, discarded_blocks; /* block magics; of them on a chain; decoded for nothing       */
    uint64_t device_blocks, host_blocks;                 /* chain blocks expanded by the kernels; decoded on host threads */
    uint64_t device_bytes, host_bytes;                   /* what they expanded to                                        */
    uint32_t rounds, uploads;                            /* runs of the symbol and walk kernels; transfers of gathered inputs */
    double symbols_ms, walk_ms, expand_ms, crc_ms;       /* the kernels' time by phase                                   */
} xlz_bz2_stats;
int xlz_ctx_last_bz2_stats(xlz_ctx *ctx, xlz_bz2_stats *out);
/* 1: on the device (the default), 2: every block on host threads.  Mode 0 is accepted and means 1 to the many-calls.    */
int xlz_ctx_set_bz2_mode(xlz_ctx *ctx, int mode);
int xlz_ctx_bz2_mode(const xlz_ctx *ctx);
/* The scratch one round of candidates may take, in bytes (0: the default, 6 GiB -- what the 1024 level-9 blocks take that
 * a device of 256 CUs at four one-wave workgroups per CU has in flight at once).  A candidate's scratch always fits.    */
int xlz_ctx_set_bz2_scratch(xlz_ctx *ctx, uint64_t bytes);
/* Host only.  CRC-32/BZIP2 (polynomial 0x04C11DB7, not reflected) of `crc`'s bytes followed by p[0 .. n); crc = 0: of p. */
uint32_t xlz_crc32_bzip2_host(uint32_t crc, const uint8_t *p, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* XLZ_H */
