// xlz_check_host.h -- what the container front-ends (xlz_xz.hip, xlz_7z.hip) use of the post-decode stage in
// xlz_host.hip.  Not part of the C ABI.
#pragma once
#include <cstring>
#include <vector>

#include "../../include/xlz.h"
#include "xlz_post.h"

// fresh statistics for a front-end call: of the checks (check mode 1 and 2), of the filters (filter mode 1) and of
// SHA-256 (check mode 2).  The batches the call makes with PostWork::accumulate, and the ranges it checks on the host
// itself (SHA-256 blocks in mode 1, Copy folders), add to them.
void xlz_internal_check_stats_reset(xlz_ctx *ctx);
void xlz_internal_check_stats_host(xlz_ctx *ctx, uint64_t ranges, uint64_t bytes);
void xlz_internal_filter_stats_reset(xlz_ctx *ctx);
void xlz_internal_sha256_stats_reset(xlz_ctx *ctx);
void xlz_internal_pack_stats_reset(xlz_ctx *ctx);
// what xlz_ctx_last_xz_read_stats reports: set by every xlz_xz_read / xlz_xz_read_device
void xlz_internal_xz_read_stats_set(xlz_ctx *ctx, const xlz_xz_read_stats &s);
// what xlz_ctx_last_xz_many_stats reports: set by every xlz_xz_decode_many / xlz_xz_decode_many_device that ran
void xlz_internal_xz_many_stats_set(xlz_ctx *ctx, const xlz_xz_many_stats &s);
// what xlz_ctx_last_7z_extract_stats reports: set by every xlz_7z_extract / xlz_7z_extract_device that ran
void xlz_internal_7z_extract_stats_set(xlz_ctx *ctx, const xlz_7z_extract_stats &s);
// what xlz_ctx_last_zip_extract_stats reports: set by every xlz_zip_extract / xlz_zip_extract_device that ran
void xlz_internal_zip_extract_stats_set(xlz_ctx *ctx, const xlz_zip_extract_stats &s);
// what xlz_ctx_last_gz_stats reports: set by every xlz_gz_decode_many / xlz_gz_decode_many_device that ran
void xlz_internal_gz_stats_set(xlz_ctx *ctx, const xlz_gz_stats &s);
// what xlz_ctx_last_bz2_stats reports: set by every xlz_bz2_decode_many / xlz_bz2_decode_many_device that ran
void xlz_internal_bz2_stats_set(xlz_ctx *ctx, const xlz_bz2_stats &s);
// what xlz_bz2.hip needs of the context: its device, its stream (void *: a hipStream_t), the bz2 mode and scratch budget
struct Bz2Env {
    int device, num_cus, mode;
    void *stream;
    uint64_t scratch;
};
int xlz_internal_bz2_env(xlz_ctx *ctx, Bz2Env *env);
// the context's mutex, held around the device work of a round (not around the calls above and below, which take it)
void xlz_internal_ctx_lock(xlz_ctx *ctx);
void xlz_internal_ctx_unlock(xlz_ctx *ctx);
// xlz_adler32_device behind its argument tests of the context and the pointer (the ranges lie inside buf_len); *ms
// (optional) += the kernels' time
int xlz_internal_adler_run(xlz_ctx *ctx, const void *d_buf, size_t buf_len, const xlz_adler_range *ranges, size_t n, uint32_t *digests, double *ms);
// the device steps of xlz_tar_scan_device (xlz_tar_dev.hip) on the context's stream: the flags of the image's complete
// 512-byte blocks -> flags_out, and blocks idx[0 .. n) dense -> out_host; *ms = the kernel's time.  What
// xlz_ctx_last_tar_stats reports is set by every scan that ran.
extern "C" int xlz_internal_tar_classify_device(xlz_ctx *ctx, const void *d_image, uint64_t len, uint8_t *flags_out, double *ms);
int xlz_internal_tar_gather_device(xlz_ctx *ctx, const void *d_image, uint64_t len, const uint64_t *idx, size_t n, uint8_t *out_host, double *ms);
void xlz_internal_tar_stats_set(xlz_ctx *ctx, const xlz_tar_stats &s);
// xlz_decode_batch with what `post` asks for behind it: xlz_decode_batch_checked, _filtered and _digests are this
int xlz_internal_decode_batch(xlz_ctx *ctx, const xlz_stream_desc *streams, size_t n, xlz_result *results, const PostWork &post);

// Where xlz_xz_decode_device / xlz_7z_decode_device want the decoded bytes: stream i of the call must produce exactly
// want_out[i] bytes (and, where want_in is given, use exactly want_in[i] bytes of input), which go to d_dst + dst_off[i];
// copies: bytes that go there from the host as they are (.7z Copy folders).  items (xlz_xz_read_device): the pack's table
// spelled out -- any ranges of the streams, as xlz_batch_pack takes them -- instead of one whole stream per dst_off[i],
// which is then not looked at.
struct DeviceCopy {
    uint64_t dst_off;
    const uint8_t *src;
    uint64_t len;
};
struct DeviceDest {
    void *d_dst = nullptr;
    size_t cap = 0;
    const uint64_t *want_out = nullptr, *want_in = nullptr, *dst_off = nullptr;
    const DeviceCopy *copies = nullptr;
    size_t n_copies = 0;
    const xlz_pack_item *items = nullptr;
    size_t n_items = 0;
    bool have_items = false;
    // .7z BCJ2 folders (bcj2 mode 1 / 2): no_pack[i] != 0 -- stream i is a sub-stream of one, it must still produce
    // want_out[i] bytes but is not packed; the folders are merged into d_dst behind the pack (items as xlz_batch_bcj2 takes
    // them, bcj2_res[] their outcomes, bcj2_mode 1: on the device, 2: on host threads)
    const uint8_t *no_pack = nullptr;
    const xlz_bcj2_item *bcj2 = nullptr;
    size_t n_bcj2 = 0;
    xlz_bcj2_result *bcj2_res = nullptr;
    int bcj2_mode = 1;
    // tolerant (xlz_xz_decode_many_device: ONE batch over the blocks of many files): a stream that failed, or that did not
    // produce want_out[i] / use want_in[i], does not end the call.  It is left out of post.steps, of post.ranges (whose
    // outputs stay as the caller set them) and of the pack; the caller reads results[] and folds them into its files.
    // With items: every item of such a stream is left out.  Not with no_pack or bcj2.
    bool tolerant = false;
    // what a stream must end in (tolerant only, xlz_7z_extract: folders that are cut on purpose).  Absent, or XLZ_OK for
    // stream i: as above -- any status >= 0.  A negative want_status[i]: exactly that status, with want_out[i] bytes
    // and, where want_in is given and want_in[i] is not kAnyInput, want_in[i] bytes of input used.
    const int32_t *want_status = nullptr;
    static constexpr uint64_t kAnyInput = ~(uint64_t)0;
    // gather_copies (xlz_zip_extract: thousands of stored entries, and every small copy costs the stack some 12 us): the
    // copies do not go up one by one behind everything else.  Host threads gather them into a pinned block of the
    // context's pool, each at an offset congruent to its destination modulo 16, the block goes up in ONE transfer with
    // its item table in front, and the pack kernel scatters it with the block as its source -- BEFORE the digests of the
    // ranges over the destination, which may therefore cover copied bytes.  A block holds at most kGatherBlockBytes of
    // copies (a longer copy has one to itself); *copy_uploads (optional) = the transfers made.  n may then be 0.
    bool gather_copies = false;
    uint32_t *copy_uploads = nullptr;
    static constexpr uint64_t kGatherBlockBytes = 256ull << 20;
    // raw deflate streams (xlz_zip_extract in deflate mode 1 / 2; with gather_copies only): items as xlz_inflate_batch takes
    // them, inflated into d_dst behind the scatter of the copies and in front of the digests of the ranges over the
    // destination, which may therefore cover them; inflate_res[] their outcomes, inflate_mode 1: on the device, 2: on host
    // threads.  One that failed does not end the call.  n may then be 0.
    const xlz_inflate_item *inflate = nullptr;
    size_t n_inflate = 0;
    xlz_inflate_result *inflate_res = nullptr;
    int inflate_mode = 1;
};
// a device block of at least `bytes` from the context's pool (xlz_7z_decode with a BCJ2 folder decodes into one), its
// download into host memory once the context's stream has drained, and its return
int xlz_internal_device_block(xlz_ctx *ctx, size_t bytes, void **p);
int xlz_internal_device_block_download(xlz_ctx *ctx, const void *p, uint8_t *dst, size_t bytes);
void xlz_internal_device_block_release(xlz_ctx *ctx, void *p);
// The host form of a device-destination call (xlz_xz_read, xlz_7z_extract, xlz_zip_extract): what the call wants lies back
// to back in ONE such block -- add() while planning, acquire() (no block where nothing was added), d_dst() / cap() for
// DeviceDest --, comes down in one copy and is scattered on the host.  The block goes back behind the download, and
// at the latest when the object goes.
class HostStaging {
public:
    struct Piece { // block bytes [staged, staged + len) -> out + dst_off
        uint64_t staged, dst_off, len;
    };
    explicit HostStaging(xlz_ctx *ctx) : ctx_(ctx) {}
    HostStaging(const HostStaging &) = delete;
    HostStaging &operator=(const HostStaging &) = delete;
    ~HostStaging() { xlz_internal_device_block_release(ctx_, block_); }
    uint64_t add(uint64_t len) // -> where these bytes lie in the block (no wrap: disjoint windows of a size_t capacity hold them)
    {
        size_ += len;
        return size_ - len;
    }
    int acquire() { return size_ ? xlz_internal_device_block(ctx_, (size_t)size_, &block_) : (int)XLZ_OK; }
    void *d_dst() const { return block_; }
    size_t cap() const { return (size_t)size_; }
    // ONE copy of the block: straight into `out` where one piece is all of it, else through a bounce buffer
    int download(uint8_t *out, const std::vector<Piece> &pieces)
    {
        int st = XLZ_OK;
        if (pieces.size() == 1 && pieces[0].staged == 0 && pieces[0].len == size_)
            st = xlz_internal_device_block_download(ctx_, block_, out + pieces[0].dst_off, (size_t)size_);
        else if (!pieces.empty()) {
            std::vector<uint8_t> bounce((size_t)size_);
            st = xlz_internal_device_block_download(ctx_, block_, bounce.data(), bounce.size());
            for (size_t j = 0; j < pieces.size() && st == XLZ_OK; j++) memcpy(out + pieces[j].dst_off, bounce.data() + pieces[j].staged, (size_t)pieces[j].len);
        }
        xlz_internal_device_block_release(ctx_, block_);
        block_ = nullptr;
        return st;
    }

private:
    xlz_ctx *ctx_;
    uint64_t size_ = 0;
    void *block_ = nullptr;
};
// The end of xlz_7z_extract / xlz_zip_extract: st = what the batch said; v[i] = want i's verdict, whose bytes -- where it is
// XLZ_OK -- lie at dst[i] of the staging block (if there is one) and go to out + wants[i].dst_off.  results[] = the
// verdicts, or the call's failure for every want; xs counts the failed and the copied.  -> the call's status
template <class Want, class Result, class Stats>
int xlz_internal_extract_finish(HostStaging &staging, int st, const Want *wants, const uint64_t *dst, const std::vector<Result> &v, uint8_t *out,
                                Result *results, Stats &xs)
{
    if (st == XLZ_OK && staging.d_dst()) {
        std::vector<HostStaging::Piece> good;
        for (size_t i = 0; i < v.size(); i++)
            if (v[i].status == XLZ_OK && v[i].out_len) good.push_back({dst[i], wants[i].dst_off, v[i].out_len});
        st = staging.download(out, good);
    }
    for (size_t i = 0; i < v.size(); i++) {
        results[i] = st == XLZ_OK ? v[i] : Result{st, 0, 0};
        xs.failed_entries += results[i].status != XLZ_OK, xs.copied_bytes += results[i].out_len;
    }
    return st;
}
// XLZ_OK: [p, p + cap) is device memory of the context's device, as far as the runtime tells (what xlz_batch_pack asks of d_dst)
int xlz_internal_device_dst_ok(xlz_ctx *ctx, const void *p, size_t cap);
void xlz_internal_bcj2_stats_reset(xlz_ctx *ctx);
// The device-destination form of xlz_internal_decode_batch (streams[i].out is NULL): one batch -- create, run, results,
// the size checks above (a stream's own failure, then XLZ_ERR_RESULT) -- and behind it, all on the context's stream:
// post.steps; the digests of post.ranges that name a stream; the pack into dest; the BCJ2 merges; the digests of
// post.ranges that name the destination; the copies; a wait.  post.ranges is ONE list (exactly one of crc_out / digest_out
// when it is not empty, indexed like it): a range whose stream is xlzpost::kDestStream means bytes [off, off + len) of
// d_dst -- where alone a merged BCJ2 folder ever lies; CRC32 / CRC64, inside dest.cap.  The statistics always
// accumulate, but the pack's, which are this call's.  XLZ_ERR_UNSUPPORTED for a stream of 4 GiB and more.
int xlz_internal_decode_device(xlz_ctx *ctx, const xlz_stream_desc *streams, size_t n, xlz_result *results, const PostWork &post,
                               const DeviceDest &dest);
