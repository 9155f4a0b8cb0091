// xlz_xz.hip -- .xz container front-end: block index -> batch of raw LZMA2 streams.
//
// SURVEY.md section 8(f) rank 3.  The reference has no container code (ReadMe.md:6 sends 7z
// users to bodgit/sevenzip); what it offers a container is NewReader2(in, dictSize)
// (reader2.go:26-41) for ONE raw LZMA2 stream.  An .xz file is a list of blocks, each of which is
// exactly such a stream with its own dictionary -- independent by construction -- so the whole
// file is ONE call of the batch engine: block i = stream i, every block further cut into
// dictionary-reset units by scan_lzma2 (xlz_host.hip).
//
// Host-only code (no kernels here).  Format: "The .xz File Format" 1.0.4 (tukaani.org), restated
// from the published specification; nothing of it exists in the reference.  Only what feeds the
// LZMA2 path is implemented: a block is one LZMA2 filter, or -- xlz_xz_index_chains, and xlz_xz_decode in
// filter mode 1 -- one to three Delta / BCJ filters in front of it, which become filter steps of the
// batch (xlz_filter_dev.hip).  ARM64, RISC-V and every other filter id: XLZ_ERR_UNSUPPORTED.
// At the end: byte ranges of a file (xlz_xz_open / xlz_xz_read), a batch of the blocks that hold them (xlz_xz_cover.h); and
// many files as one batch with a status per file (xlz_xz_decode_many, xlz_xz_many.h).
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/xlz.h"
#include "xlz_check.h"
#include "xlz_check_host.h"
#include "xlz_filter_dev.h"
#include "xlz_xz_cover.h"
#include "xlz_xz_many.h"

namespace {

using xlzcheck::crc32;
using xlzcheck::crc64;

uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// variable-length integer (spec 1.2): 7 bits per byte, at most 9 bytes, no trailing zero byte
bool vli(const uint8_t *p, size_t n, size_t &pos, uint64_t &v)
{
    v = 0;
    for (unsigned i = 0; i < 9; i++) {
        if (pos >= n) return false;
        const uint8_t b = p[pos++];
        v |= (uint64_t)(b & 0x7F) << (7 * i);
        if (!(b & 0x80)) return !(b == 0 && i != 0);
    }
    return false;
}

const uint8_t kHeadMagic[6] = {0xFD, '7', 'z', 'X', 'Z', 0x00};
const uint8_t kFootMagic[2] = {'Y', 'Z'};

unsigned check_size(unsigned type) { return type == 0 ? 0 : type <= 3 ? 4 : type <= 6 ? 8 : type <= 9 ? 16 : type <= 12 ? 32 : 64; }

// DecodeDictSize2 of the reference (reader2.go:296-298) stops at 40; the .xz filter flag allows
// 0..40 with 40 = 4 GiB - 1 (spec 5.3.1)
bool xz_dict_size(uint8_t b, uint32_t &d)
{
    if (b > 40) return false;
    d = b == 40 ? 0xFFFFFFFFu : (2u | (b & 1u)) << (b / 2 + 11);
    return true;
}

struct Stream {
    size_t start = 0, end = 0; // [start, end) of the stream inside the file, padding excluded
    size_t index_start = 0;    // blocks live in [start + 12, index_start)
    unsigned check = 0;
    std::vector<std::pair<uint64_t, uint64_t>> records; // (unpadded size, uncompressed size)
};

// one stream, located from its end (footer -> index -> header); spec 2.1
int parse_stream_backwards(const uint8_t *f, size_t end, Stream &s)
{
    if (end < 32) return XLZ_ERR_UNEXPECTED_EOF;
    const uint8_t *ft = f + end - 12;
    if (memcmp(ft + 10, kFootMagic, 2) != 0) return XLZ_ERR_RESULT;
    if (crc32(ft + 4, 6) != le32(ft)) return XLZ_ERR_RESULT;
    if (ft[8] != 0 || (ft[9] & 0xF0)) return XLZ_ERR_UNSUPPORTED;
    s.check = ft[9] & 0x0F;
    const uint64_t index_size = ((uint64_t)le32(ft + 4) + 1) * 4;
    if (index_size + 24 > end) return XLZ_ERR_RESULT;
    const size_t ix = end - 12 - (size_t)index_size; // where the index starts
    s.index_start = ix;
    const uint8_t *ip = f + ix;
    if (crc32(ip, (size_t)index_size - 4) != le32(ip + index_size - 4)) return XLZ_ERR_RESULT;
    if (ip[0] != 0x00) return XLZ_ERR_RESULT;
    size_t pos = 1;
    uint64_t nrec;
    if (!vli(ip, (size_t)index_size - 4, pos, nrec)) return XLZ_ERR_RESULT;
    if (nrec > index_size / 2) return XLZ_ERR_RESULT;
    uint64_t blocks_total = 0;
    s.records.clear();
    for (uint64_t r = 0; r < nrec; r++) {
        uint64_t unpadded, uncomp;
        if (!vli(ip, (size_t)index_size - 4, pos, unpadded) || !vli(ip, (size_t)index_size - 4, pos, uncomp)) return XLZ_ERR_RESULT;
        // every block lies between the 12-byte stream header and the index: a record that does not
        // fit what is left there is rejected before it is added (no 64-bit wrap of the sum)
        if (unpadded < 5 || ix < 12 || unpadded > (uint64_t)ix - 12 - blocks_total) return XLZ_ERR_RESULT;
        const uint64_t padded = (unpadded + 3) & ~3ull;
        if (padded > (uint64_t)ix - 12 - blocks_total) return XLZ_ERR_RESULT;
        if (uncomp > (1ull << 62)) return XLZ_ERR_RESULT;
        s.records.emplace_back(unpadded, uncomp);
        blocks_total += padded;
    }
    while (pos < index_size - 4)
        if (ip[pos++] != 0) return XLZ_ERR_RESULT; // index padding
    if (blocks_total + 12 > ix) return XLZ_ERR_RESULT;
    s.start = ix - (size_t)blocks_total - 12;
    s.end = end;
    const uint8_t *hd = f + s.start;
    if (memcmp(hd, kHeadMagic, 6) != 0) return XLZ_ERR_RESULT;
    if (crc32(hd + 6, 2) != le32(hd + 8)) return XLZ_ERR_RESULT;
    if (hd[6] != ft[8] || hd[7] != ft[9]) return XLZ_ERR_RESULT;
    return XLZ_OK;
}

// block header (spec 3.1).  chain == nullptr: only "one LZMA2 filter" chains are accepted.  Otherwise up to three Delta /
// BCJ filters may precede the LZMA2 filter; they are returned in the order the header lists them (the encoder's: the
// decoder undoes them last to first).  What liblzma refuses is refused: a property size that is not the filter's, a start
// offset that is not a multiple of the filter's alignment, LZMA2 anywhere but last, anything else last.
int parse_block_header(const uint8_t *p, size_t avail, size_t &hdr_size, uint32_t &dict, uint64_t &comp_size,
                       uint64_t &uncomp_size, std::vector<std::pair<uint32_t, uint32_t>> *chain = nullptr)
{
    if (avail < 8 || p[0] == 0) return XLZ_ERR_RESULT;
    hdr_size = ((size_t)p[0] + 1) * 4;
    if (hdr_size > avail) return XLZ_ERR_UNEXPECTED_EOF;
    if (crc32(p, hdr_size - 4) != le32(p + hdr_size - 4)) return XLZ_ERR_RESULT;
    const uint8_t flags = p[1];
    if (flags & 0x3C) return XLZ_ERR_UNSUPPORTED;
    const unsigned nfilters = (flags & 3) + 1;
    size_t pos = 2;
    comp_size = uncomp_size = ~0ull;
    if ((flags & 0x40) && !vli(p, hdr_size - 4, pos, comp_size)) return XLZ_ERR_RESULT;
    if ((flags & 0x80) && !vli(p, hdr_size - 4, pos, uncomp_size)) return XLZ_ERR_RESULT;
    bool have_lzma2 = false;
    for (unsigned k = 0; k < nfilters; k++) {
        uint64_t id, psz;
        if (!vli(p, hdr_size - 4, pos, id) || !vli(p, hdr_size - 4, pos, psz)) return XLZ_ERR_RESULT;
        if (pos + psz > hdr_size - 4) return XLZ_ERR_RESULT;
        if (id == 0x21 && psz == 1 && k + 1 == nfilters) {
            if (!xz_dict_size(p[pos], dict)) return XLZ_ERR_RESULT;
            have_lzma2 = true;
        } else if (chain && k + 1 < nfilters && id == XLZ_FILTER_DELTA && psz == 1) {
            chain->emplace_back((uint32_t)id, (uint32_t)p[pos] + 1);
        } else if (chain && k + 1 < nfilters && id >= XLZ_FILTER_X86 && id <= XLZ_FILTER_SPARC && (psz == 0 || psz == 4)) {
            const uint32_t start = psz ? le32(p + pos) : 0;
            if (xlzflt::bad_step((uint32_t)id, start)) return XLZ_ERR_UNSUPPORTED;
            chain->emplace_back((uint32_t)id, start);
        } else {
            return XLZ_ERR_UNSUPPORTED; // BCJ / delta / anything else in the chain
        }
        pos += (size_t)psz;
    }
    while (pos < hdr_size - 4)
        if (p[pos++] != 0) return XLZ_ERR_RESULT;
    return have_lzma2 && (nfilters == 1 || chain) ? XLZ_OK : XLZ_ERR_UNSUPPORTED;
}

int xz_index(const uint8_t *file, size_t len, xlz_xz_block *blocks, size_t max_blocks, size_t *n_blocks, xlz_filter_step *steps,
             size_t max_steps, size_t *n_steps, uint64_t *total_uncompressed, bool chains);

} // namespace

// Every block of every stream of an .xz file, in file order (spec 2: concatenated streams and
// stream padding allowed).  Pure host parse; no device needed.
extern "C" int xlz_xz_index(const uint8_t *file, size_t len, xlz_xz_block *blocks, size_t max_blocks, size_t *n_blocks,
                            uint64_t *total_uncompressed)
{
    return xz_index(file, len, blocks, max_blocks, n_blocks, nullptr, 0, nullptr, total_uncompressed, false);
}

// The same for files whose blocks may carry filter chains: the filters in front of a block's LZMA2 filter come back as
// steps in the order a decoder applies them (the reverse of the header's), step.stream = the block's index.
extern "C" int xlz_xz_index_chains(const uint8_t *file, size_t len, xlz_xz_block *blocks, size_t max_blocks, size_t *n_blocks,
                                   xlz_filter_step *steps, size_t max_steps, size_t *n_steps, uint64_t *total_uncompressed)
{
    if (!n_steps || (!steps && max_steps)) return XLZ_ERR_BAD_ARG;
    return xz_index(file, len, blocks, max_blocks, n_blocks, steps, max_steps, n_steps, total_uncompressed, true);
}

namespace {
int xz_index(const uint8_t *file, size_t len, xlz_xz_block *blocks, size_t max_blocks, size_t *n_blocks, xlz_filter_step *steps,
             size_t max_steps, size_t *n_steps, uint64_t *total_uncompressed, bool chains)
{
    if (!file || !n_blocks || (!blocks && max_blocks)) return XLZ_ERR_BAD_ARG;
    *n_blocks = 0;
    if (n_steps) *n_steps = 0;
    size_t ns = 0;
    std::vector<std::pair<uint32_t, uint32_t>> chain;
    if (total_uncompressed) *total_uncompressed = 0;
    std::vector<Stream> streams;
    size_t end = len;
    while (end > 0) {
        while (end >= 4 && le32(file + end - 4) == 0) end -= 4; // stream padding
        if (end == 0) break;
        if (end & 3) return XLZ_ERR_RESULT;
        Stream s;
        const int st = parse_stream_backwards(file, end, s);
        if (st != XLZ_OK) return st;
        streams.push_back(std::move(s));
        end = streams.back().start;
    }
    if (streams.empty()) return XLZ_ERR_UNEXPECTED_EOF;
    std::reverse(streams.begin(), streams.end());
    uint64_t uoff = 0;
    size_t nb = 0;
    for (const Stream &s : streams) {
        size_t pos = s.start + 12;
        for (const auto &rec : s.records) {
            size_t hdr;
            uint32_t dict = 0;
            uint64_t csz, usz;
            const uint64_t padded = (rec.first + 3) & ~3ull;
            if (pos > s.index_start || padded > s.index_start - pos) return XLZ_ERR_RESULT; // block inside the stream
            chain.clear();
            const int st = parse_block_header(file + pos, s.index_start - pos, hdr, dict, csz, usz, chains ? &chain : nullptr);
            if (st != XLZ_OK) return st;
            for (size_t k = chain.size(); k-- > 0; ns++)
                if (ns < max_steps) {
                    memset(&steps[ns], 0, sizeof steps[ns]);
                    steps[ns].stream = nb, steps[ns].id = chain[k].first, steps[ns].param = chain[k].second;
                }
            const unsigned chk = check_size(s.check);
            if (rec.first < hdr + chk) return XLZ_ERR_RESULT;
            const uint64_t comp = rec.first - hdr - chk;
            if (csz != ~0ull && csz != comp) return XLZ_ERR_RESULT;
            if (usz != ~0ull && usz != rec.second) return XLZ_ERR_RESULT;
            for (uint64_t k = comp; k < ((comp + 3) & ~3ull); k++) // Block Padding: null bytes (liblzma refuses others)
                if (file[pos + hdr + k] != 0) return XLZ_ERR_RESULT;
            if (nb < max_blocks) {
                xlz_xz_block &b = blocks[nb];
                b.comp_off = pos + hdr;
                b.comp_len = comp;
                b.uncomp_off = uoff;
                b.uncomp_len = rec.second;
                b.dict_size = dict;
                b.check_type = s.check;
                b.check_off = pos + hdr + ((comp + 3) & ~3ull);
            }
            nb++;
            if (rec.second > ~0ull - uoff) return XLZ_ERR_RESULT;
            uoff += rec.second;
            pos += (size_t)padded;
        }
    }
    *n_blocks = nb;
    if (n_steps) *n_steps = ns;
    if (total_uncompressed) *total_uncompressed = uoff;
    return (nb > max_blocks && max_blocks) || (ns > max_steps && max_steps) ? XLZ_ERR_OUT_CAP : XLZ_OK;
}

// ---------------------------------------------------------------- a block as a stream of the batch ----
// What xz_decode, xz_read and xz_many share.  The block's descriptor: a raw LZMA2 stream (reader2.go:26-41) that decodes
// to `out` (NULL: the call has a device destination)
xlz_stream_desc block_desc(const uint8_t *file, const xlz_xz_block &b, uint8_t *out)
{
    xlz_stream_desc d;
    memset(&d, 0, sizeof d);
    d.in = file + b.comp_off, d.in_len = (size_t)b.comp_len;
    d.out = out, d.out_cap = (size_t)b.uncomp_len;
    d.format = XLZ_FMT_LZMA2_RAW, d.dict_size = b.dict_size;
    return d;
}

// The checks the device computes for streams [0, n) under a check mode (xlz_ctx_set_check_mode): 0 none, 1 the CRC32 /
// CRC64 blocks, 2 the SHA-256 blocks too.  Mode 2 asks for the 32-byte form only where a block needs it (the SHA-256
// statistics are that form's alone); a CRC then lies little-endian in its first bytes.
constexpr size_t kNoRange = ~(size_t)0;
struct BlockChecks {
    std::vector<xlz_check_range> cr;
    std::vector<size_t> range_of; // stream -> its range in cr, or kNoRange
    bool sha = false;             // the digests come as xgot, not as got
    std::vector<uint64_t> got;
    std::vector<xlz_digest> xgot;
    PostWork work(const xlz_filter_step *steps, size_t n_steps) { return {steps, n_steps, cr.data(), cr.size(), sha ? nullptr : got.data(), sha ? xgot.data() : nullptr, true}; }
    void digest(size_t q, uint8_t dg[32]) const // the bytes of range q as the file's check field holds them
    {
        if (sha)
            memcpy(dg, xgot[q].b, 32);
        else
            for (int j = 0; j < 8; j++) dg[j] = (uint8_t)(got[q] >> (8 * j));
    }
};
template <class BlockOf> BlockChecks block_checks(size_t n, int cmode, BlockOf block_of) // block_of(s): the block of stream s
{
    BlockChecks c;
    c.range_of.assign(n, kNoRange);
    for (size_t s = 0; s < n && cmode == 2; s++) c.sha |= block_of(s).check_type == 10;
    for (size_t s = 0; s < n && (cmode == 1 || cmode == 2); s++) {
        const xlz_xz_block &b = block_of(s);
        if (b.check_type != 1 && b.check_type != 4 && !(c.sha && b.check_type == 10)) continue;
        xlz_check_range r;
        memset(&r, 0, sizeof r);
        r.stream = s, r.off = 0, r.len = b.uncomp_len, r.kind = b.check_type;
        c.range_of[s] = c.cr.size(), c.cr.push_back(r);
    }
    c.got.assign(c.sha ? 0 : c.cr.size(), 0), c.xgot.assign(c.sha ? c.cr.size() : 0, xlz_digest{});
    return c;
}

// What the check field of the block of stream s says of its decoded bytes: the device's digest where c has one, else the
// host's over p (NULL: a device destination, where every check is the device's).  A reserved check type is not verified.
uint8_t block_check(const uint8_t *file, const xlz_xz_block &b, const BlockChecks &c, size_t s, const uint8_t *p)
{
    if (b.check_type != 1 && b.check_type != 4 && b.check_type != 10) return b.check_type ? xlzmany::kCheckUnverified : xlzmany::kCheckGood;
    uint8_t dg[32] = {};
    if (c.range_of[s] != kNoRange)
        c.digest(c.range_of[s], dg);
    else if (b.check_type == 1)
        for (uint32_t v = crc32(p, (size_t)b.uncomp_len), j = 0; j < 4; j++) dg[j] = (uint8_t)(v >> (8 * j));
    else if (b.check_type == 4)
        for (uint64_t v = crc64(p, (size_t)b.uncomp_len), j = 0; j < 8; j++) dg[j] = (uint8_t)(v >> (8 * j));
    else
        xlzcheck::sha256(p, (size_t)b.uncomp_len, dg);
    return memcmp(dg, file + b.check_off, check_size(b.check_type)) != 0 ? xlzmany::kCheckFailed : xlzmany::kCheckGood;
}
} // namespace

// Whole file: index, one batch (block = raw LZMA2 stream, reader2.go:26-41), optional integrity
// check of every block (CRC32 / CRC64 on host threads; other check types are left unverified
// and reported through *unverified).
// d_out: the device-destination form (xlz_xz_decode_device; one context, out == NULL): the decoded file goes to d_out
static int xz_decode(xlz_ctx *const *ctxs, size_t n_ctx, const uint8_t *file, size_t len, uint8_t *out, size_t out_cap,
                     uint64_t *out_len, int verify, size_t *unverified, void *d_out = nullptr);

extern "C" int xlz_xz_decode(xlz_ctx *ctx, const uint8_t *file, size_t len, uint8_t *out, size_t out_cap, uint64_t *out_len,
                             int verify, size_t *unverified)
{
    return xz_decode(&ctx, 1, file, len, out, out_cap, out_len, verify, unverified);
}

// several contexts (one per GPU): the blocks, and the units inside large blocks, are dealt by xlz_decode_batch_multi
extern "C" int xlz_xz_decode_multi(xlz_ctx *const *ctxs, size_t n_ctx, const uint8_t *file, size_t len, uint8_t *out,
                                   size_t out_cap, uint64_t *out_len, int verify, size_t *unverified)
{
    if (!ctxs || !n_ctx) return XLZ_ERR_BAD_ARG;
    return xz_decode(ctxs, n_ctx, file, len, out, out_cap, out_len, verify, unverified);
}

// Into device memory: the same parse, the same batch and the same comparisons as xlz_xz_decode; the checks always come
// from the device (as in check mode 2), and a pack puts the blocks side by side in d_out (xlz_internal_decode_device).
extern "C" int xlz_xz_decode_device(xlz_ctx *ctx, const uint8_t *file, size_t len, void *d_out, size_t out_cap, uint64_t *out_len,
                                    int verify, size_t *unverified)
{
    if (!ctx || (!d_out && out_cap)) return XLZ_ERR_BAD_ARG;
    uint8_t none = 0; // (an empty file needs no destination)
    const int st = xz_decode(&ctx, 1, file, len, nullptr, out_cap, out_len, verify, unverified, d_out ? d_out : &none);
    if (st != XLZ_OK && out_len) *out_len = 0;
    return st;
}

static int xz_decode(xlz_ctx *const *ctxs, size_t n_ctx, const uint8_t *file, size_t len, uint8_t *out, size_t out_cap,
                     uint64_t *out_len, int verify, size_t *unverified, void *d_out)
{
    for (size_t c = 0; c < n_ctx; c++)
        if (!ctxs[c]) return XLZ_ERR_BAD_ARG;
    if (!file || (!out && out_cap && !d_out) || !out_len) return XLZ_ERR_BAD_ARG;
    *out_len = 0;
    if (unverified) *unverified = 0;
    size_t nb = 0, nfs = 0;
    uint64_t total = 0;
    // filter mode 1 (xlz_ctx_set_filter_mode; one context): blocks may carry Delta / BCJ filters; fs = their steps
    const bool chains = n_ctx == 1 && xlz_ctx_filter_mode(ctxs[0]) == 1;
    int st = xz_index(file, len, nullptr, 0, &nb, nullptr, 0, &nfs, &total, chains);
    if (st != XLZ_OK) return st;
    if (total > out_cap) return XLZ_ERR_OUT_CAP;
    std::vector<xlz_xz_block> blk(nb);
    std::vector<xlz_filter_step> fs(nfs);
    st = xz_index(file, len, blk.data(), nb, &nb, fs.data(), nfs, &nfs, &total, chains);
    if (st != XLZ_OK) return st;
    std::vector<xlz_stream_desc> d(nb);
    std::vector<xlz_result> r(nb);
    for (size_t i = 0; i < nb; i++) d[i] = block_desc(file, blk[i], out ? out + blk[i].uncomp_off : nullptr);
    // check mode 1 (xlz_ctx_set_check_mode; one context): the CRC32 / CRC64 of every block comes from the device with the
    // batch's results; the other check types stay with the host threads below
    // check mode 2: the SHA-256 blocks join the range list (the device's or the host's, as xlz_sha256_plan splits them)
    // (a device destination: there are no bytes on the host to check, so as mode 2 whatever the context's mode says)
    const int cmode = !verify ? 0 : d_out ? 2 : n_ctx == 1 ? xlz_ctx_check_mode(ctxs[0]) : 0;
    std::vector<uint64_t> want_out(d_out ? nb : 0), want_in(d_out ? nb : 0), dst_off(d_out ? nb : 0);
    for (size_t i = 0; i < nb && d_out; i++) want_out[i] = blk[i].uncomp_len, want_in[i] = blk[i].comp_len, dst_off[i] = blk[i].uncomp_off;
    DeviceDest dest;
    dest.d_dst = d_out, dest.cap = out_cap, dest.want_out = want_out.data(), dest.want_in = want_in.data(), dest.dst_off = dst_off.data();
    auto decode = [&](const PostWork &w) {
        return d_out ? xlz_internal_decode_device(ctxs[0], d.data(), nb, r.data(), w, dest) : xlz_internal_decode_batch(ctxs[0], d.data(), nb, r.data(), w);
    };
    const bool dev = cmode == 1 || cmode == 2;
    if (cmode == 2) xlz_internal_sha256_stats_reset(ctxs[0]); // (the statistics of THIS call, also when it has no SHA-256 block)
    BlockChecks ck = block_checks(nb, cmode, [&](size_t i) -> const xlz_xz_block & { return blk[i]; });
    if (dev) {
        xlz_internal_check_stats_reset(ctxs[0]);
        if (chains) xlz_internal_filter_stats_reset(ctxs[0]);
        st = decode(ck.work(fs.data(), nfs));
    } else if (chains) { // (the digests, if any, on host threads below: over the filtered bytes)
        xlz_internal_filter_stats_reset(ctxs[0]);
        st = decode(PostWork{fs.data(), nfs, nullptr, 0, nullptr, nullptr, true});
    } else if (d_out)
        st = decode(PostWork{});
    else
        st = n_ctx > 1 ? xlz_decode_batch_multi(ctxs, n_ctx, d.data(), nb, r.data()) : xlz_decode_batch(ctxs[0], d.data(), nb, r.data());
    if (st != XLZ_OK) return st;
    for (size_t i = 0; i < nb; i++) {
        if (r[i].status < 0) return r[i].status;
        // a block must produce exactly what the index says and use its whole payload
        if (r[i].out_len != blk[i].uncomp_len || r[i].in_consumed != blk[i].comp_len) return XLZ_ERR_RESULT;
    }
    if (verify) {
        std::vector<uint8_t> check(nb);
        xlzpost::parallel_for(nb, xlzpost::host_thread_cap(16),
                              [&](size_t i) { check[i] = block_check(file, blk[i], ck, i, out ? out + blk[i].uncomp_off : nullptr); });
        if (dev && !ck.sha)
            for (size_t i = 0; i < nb; i++)
                if (blk[i].check_type == 10) xlz_internal_check_stats_host(ctxs[0], 1, blk[i].uncomp_len);
        size_t nu = 0;
        for (size_t i = 0; i < nb; i++) {
            if (check[i] == xlzmany::kCheckFailed) return XLZ_ERR_RESULT;
            nu += check[i] == xlzmany::kCheckUnverified;
        }
        if (unverified) *unverified = nu;
    }
    *out_len = total;
    return XLZ_OK;
}

// ---------------------------------------------------------------- byte ranges of a file ----
// The index parsed once (xlz_xz_open); a read (xlz_xz_read / xlz_xz_read_device) is ONE batch of the blocks that hold the
// ranges' bytes -- xlz_xz_cover.h says which, and how every range is cut into pack items over them -- and behind it the
// device's post-decode stage with that item list (xlz_internal_decode_device): filters, digests, pack.
struct xlz_xz_file {
    const uint8_t *file = nullptr; // borrowed: the caller keeps it alive
    uint64_t size = 0;             // of the decoded file
    std::vector<xlz_xz_block> blk;
    std::vector<xlz_filter_step> steps; // ascending by stream (= block index), as xz_index lists them
    std::vector<xlzcover::Extent> ext;  // (uncomp_off, uncomp_len) of blk[]
};

extern "C" int xlz_xz_open(const uint8_t *file, size_t len, xlz_xz_file **f)
{
    if (!f) return XLZ_ERR_BAD_ARG;
    *f = nullptr;
    size_t nb = 0, ns = 0;
    uint64_t total = 0;
    int st = xz_index(file, len, nullptr, 0, &nb, nullptr, 0, &ns, &total, true);
    if (st != XLZ_OK) return st;
    xlz_xz_file *h = new (std::nothrow) xlz_xz_file;
    if (!h) return XLZ_ERR_DEVICE;
    h->blk.resize(nb), h->steps.resize(ns);
    st = xz_index(file, len, h->blk.data(), nb, &nb, h->steps.data(), ns, &ns, &total, true);
    if (st != XLZ_OK) {
        delete h;
        return st;
    }
    h->file = file, h->size = total;
    for (const xlz_xz_block &b : h->blk) h->ext.push_back(xlzcover::Extent{b.uncomp_off, b.uncomp_len});
    *f = h;
    return XLZ_OK;
}

extern "C" void xlz_xz_close(xlz_xz_file *f) { delete f; }

extern "C" int xlz_xz_file_info(const xlz_xz_file *f, uint64_t *size, size_t *n_blocks, size_t *n_steps)
{
    if (!f) return XLZ_ERR_BAD_ARG;
    if (size) *size = f->size;
    if (n_blocks) *n_blocks = f->blk.size();
    if (n_steps) *n_steps = f->steps.size();
    return XLZ_OK;
}

extern "C" int xlz_xz_file_blocks(const xlz_xz_file *f, xlz_xz_block *blocks, size_t max_blocks)
{
    if (!f || (!blocks && max_blocks)) return XLZ_ERR_BAD_ARG;
    std::copy_n(f->blk.begin(), std::min(max_blocks, f->blk.size()), blocks);
    return f->blk.size() > max_blocks ? XLZ_ERR_OUT_CAP : XLZ_OK;
}

extern "C" int xlz_xz_cover(const xlz_xz_file *f, const xlz_xz_range *ranges, size_t n, size_t *blocks, size_t max_blocks, size_t *n_blocks)
{
    if (!f || (!ranges && n) || !n_blocks || (!blocks && max_blocks)) return XLZ_ERR_BAD_ARG;
    std::vector<size_t> c;
    xlzcover::cover(f->ext.data(), f->ext.size(), f->size, ranges, n, c);
    *n_blocks = c.size();
    std::copy_n(c.begin(), std::min(max_blocks, c.size()), blocks);
    return c.size() > max_blocks && max_blocks ? XLZ_ERR_OUT_CAP : XLZ_OK;
}

// out: the host form (d_out == NULL) -- the pack goes to a staging block of the context's pool, where the ranges lie one
// behind the other in the order of their destinations, and comes down from there in one copy
static int xz_read(xlz_ctx *ctx, const xlz_xz_file *f, const xlz_xz_range *ranges, size_t n, uint8_t *out, void *d_out, size_t out_cap,
                   uint64_t *copied, int verify, size_t *unverified)
{
    // ---- the arguments: all of them before the context is used
    if (!f || (!ranges && n)) return XLZ_ERR_BAD_ARG;
    for (size_t i = 0; i < n && copied; i++) copied[i] = 0;
    if (unverified) *unverified = 0;
    xlzcover::Plan p;
    if (!xlzcover::plan(f->ext.data(), f->ext.size(), f->size, ranges, n, out_cap, p)) return XLZ_ERR_BAD_ARG;
    if (!ctx || (p.total && !out && !d_out)) return XLZ_ERR_BAD_ARG;
    HostStaging staging(ctx);
    std::vector<HostStaging::Piece> runs; // host form: the ranges whose destinations touch come down as one piece
    if (!d_out) {
        std::vector<size_t> by_dst;
        for (size_t i = 0; i < n; i++)
            if (p.lens[i]) by_dst.push_back(i);
        std::sort(by_dst.begin(), by_dst.end(), [&](size_t a, size_t b) { return ranges[a].dst_off < ranges[b].dst_off; });
        std::vector<xlz_xz_range> staged(ranges, ranges + n);
        for (size_t i : by_dst) {
            staged[i].dst_off = staging.add(p.lens[i]);
            if (!runs.empty() && runs.back().dst_off + runs.back().len == ranges[i].dst_off)
                runs.back().len += p.lens[i];
            else
                runs.push_back({staged[i].dst_off, ranges[i].dst_off, p.lens[i]});
        }
        if (!xlzcover::plan(f->ext.data(), f->ext.size(), f->size, staged.data(), n, p.total, p)) return XLZ_ERR_BAD_ARG;
    }
    const size_t nc = p.blocks.size();
    // what else refuses the call before anything is launched -- and before its statistics are made: a destination that is
    // not the device's, a filter chain on a covering block in filter mode 0 (fs: the covering blocks' steps, stream = k)
    if (d_out && p.total) {
        const int ok = xlz_internal_device_dst_ok(ctx, d_out, out_cap);
        if (ok != XLZ_OK) return ok;
    }
    std::vector<xlz_filter_step> fs;
    for (size_t k = 0; k < nc; k++) {
        auto it = std::lower_bound(f->steps.begin(), f->steps.end(), p.blocks[k], [](const xlz_filter_step &s, size_t b) { return s.stream < b; });
        for (; it != f->steps.end() && it->stream == p.blocks[k]; ++it) fs.push_back(*it), fs.back().stream = k;
    }
    if (!fs.empty() && xlz_ctx_filter_mode(ctx) != 1) return XLZ_ERR_UNSUPPORTED;
    xlz_xz_read_stats rs = {};
    rs.ranges = n, rs.blocks = nc;
    for (size_t i = 0; i < n; i++) rs.empty_ranges += !p.lens[i];
    for (size_t k : p.blocks) rs.comp_bytes += f->blk[k].comp_len, rs.decoded_bytes += f->blk[k].uncomp_len;
    xlz_internal_check_stats_reset(ctx), xlz_internal_sha256_stats_reset(ctx), xlz_internal_filter_stats_reset(ctx);
    xlz_internal_pack_stats_reset(ctx), xlz_internal_xz_read_stats_set(ctx, rs);
    if (!nc) return XLZ_OK; // (every range is empty)
    // ---- the batch: the covering blocks, stream k = block p.blocks[k]; their checks
    std::vector<xlz_stream_desc> d(nc);
    std::vector<xlz_result> r(nc);
    std::vector<uint64_t> want_out(nc), want_in(nc);
    const auto block_of = [&](size_t k) -> const xlz_xz_block & { return f->blk[p.blocks[k]]; };
    for (size_t k = 0; k < nc; k++) {
        d[k] = block_desc(f->file, block_of(k), nullptr);
        want_out[k] = block_of(k).uncomp_len, want_in[k] = block_of(k).comp_len;
    }
    BlockChecks ck = block_checks(nc, verify ? 2 : 0, block_of); // (as xlz_xz_decode_device: every check is the device's)
    const PostWork w = ck.work(fs.data(), fs.size());
    int st = staging.acquire();
    if (st != XLZ_OK) return st;
    DeviceDest dest;
    dest.d_dst = d_out ? d_out : staging.d_dst(), dest.cap = d_out ? out_cap : staging.cap();
    dest.want_out = want_out.data(), dest.want_in = want_in.data();
    dest.items = p.items.data(), dest.n_items = p.items.size(), dest.have_items = true;
    st = xlz_internal_decode_device(ctx, d.data(), nc, r.data(), w, dest);
    size_t nu = 0;
    for (size_t k = 0; k < nc && st == XLZ_OK && verify; k++) {
        const uint8_t check = block_check(f->file, block_of(k), ck, k, nullptr);
        if (check == xlzmany::kCheckFailed) st = XLZ_ERR_RESULT;
        nu += check == xlzmany::kCheckUnverified;
    }
    if (st == XLZ_OK) st = staging.download(out, runs); // (the destinations touch: ONE run, straight into the caller's buffer)
    if (st != XLZ_OK) return st;
    for (size_t i = 0; i < n && copied; i++) copied[i] = p.lens[i];
    if (unverified) *unverified = nu;
    rs.copied_bytes = p.total;
    xlz_internal_xz_read_stats_set(ctx, rs);
    return XLZ_OK;
}

extern "C" int xlz_xz_read(xlz_ctx *ctx, const xlz_xz_file *f, const xlz_xz_range *ranges, size_t n, uint8_t *out, size_t out_cap,
                           uint64_t *copied, int verify, size_t *unverified)
{
    uint8_t none = 0; // (a read of nothing needs no destination)
    return xz_read(ctx, f, ranges, n, out ? out : &none, nullptr, out ? out_cap : 0, copied, verify, unverified);
}

extern "C" int xlz_xz_read_device(xlz_ctx *ctx, const xlz_xz_file *f, const xlz_xz_range *ranges, size_t n, void *d_out, size_t out_cap,
                                  uint64_t *copied, int verify, size_t *unverified)
{
    if (!d_out && out_cap) return XLZ_ERR_BAD_ARG;
    uint8_t none = 0;
    return xz_read(ctx, f, ranges, n, nullptr, d_out ? d_out : &none, d_out ? out_cap : 0, copied, verify, unverified);
}

// ---------------------------------------------------------------- many files, one batch ----
// What xz writes by default is ONE block per file: a directory of small files is a batch only across files.  Every file is
// parsed as xz_decode parses it; the blocks of all files that got that far are the streams of ONE call of the batch engine
// (xlz_xz_many.h says which stream a (file, block) is), and what comes back per stream is folded into a verdict per file
// -- the one xz_decode gives for that file alone --, so that a damaged file costs nobody else anything.
extern "C" int xlz_xz_many_layout(xlz_xz_many_file *files, size_t n, int chains, uint64_t align, xlz_xz_many_result *results, uint64_t *total)
{
    if (!total || !align || ((!files || !results) && n)) return XLZ_ERR_BAD_ARG;
    *total = 0;
    std::vector<uint64_t> sizes(n, 0), off(n, 0);
    for (size_t i = 0; i < n; i++) {
        size_t nb = 0, ns = 0;
        uint64_t t = 0;
        memset(&results[i], 0, sizeof results[i]);
        results[i].status = xz_index(files[i].file, files[i].len, nullptr, 0, &nb, nullptr, 0, &ns, &t, chains != 0);
        if (results[i].status == XLZ_OK) sizes[i] = t;
    }
    if (!xlzmany::layout(sizes.data(), n, align, off.data(), total)) {
        *total = 0;
        return XLZ_ERR_OUT_CAP;
    }
    for (size_t i = 0; i < n; i++) files[i].dst_off = off[i], files[i].dst_cap = sizes[i];
    return XLZ_OK;
}

// out: the host form (every block's stream writes inside its file's window); d_out: the device form
static int xz_many(xlz_ctx *ctx, const xlz_xz_many_file *files, size_t n, uint8_t *out, void *d_out, bool device, size_t out_cap, int verify,
                   xlz_xz_many_result *results)
{
    // ---- the arguments: all of them before the context is used, but the last
    if (!n) return XLZ_OK;
    if (!ctx || !files || !results || (out_cap && !(device ? d_out != nullptr : out != nullptr))) return XLZ_ERR_BAD_ARG;
    if (!xlzmany::windows_ok(files, n, out_cap)) return XLZ_ERR_BAD_ARG;
    if (device && out_cap) {
        const int ok = xlz_internal_device_dst_ok(ctx, d_out, out_cap);
        if (ok != XLZ_OK) return ok;
    }
    // ---- the files: index, room, (device form) blocks a unit cannot hold; what is left is the batch, stream = position in blk
    const bool chains = xlz_ctx_filter_mode(ctx) == 1;
    std::vector<xlz_xz_block> blk;
    std::vector<xlz_filter_step> fs;
    std::vector<uint8_t> in_batch(n, 0);
    std::vector<size_t> n_blocks(n, 0);
    std::vector<uint64_t> totals(n, 0);
    xlz_xz_many_stats ms = {};
    ms.files = n;
    for (size_t i = 0; i < n; i++) {
        const xlz_xz_many_file &f = files[i];
        memset(&results[i], 0, sizeof results[i]);
        size_t nb = 0, nfs = 0;
        uint64_t total = 0;
        int st = xz_index(f.file, f.len, nullptr, 0, &nb, nullptr, 0, &nfs, &total, chains);
        if (st == XLZ_OK && total > f.dst_cap) st = XLZ_ERR_OUT_CAP;
        if (st == XLZ_OK) {
            const size_t b0 = blk.size(), s0 = fs.size();
            blk.resize(b0 + nb), fs.resize(s0 + nfs);
            st = xz_index(f.file, f.len, blk.data() + b0, nb, &nb, fs.data() + s0, nfs, &nfs, &total, chains);
            for (size_t k = b0; k < blk.size() && st == XLZ_OK && device; k++) // (xlz_decode_batch decodes these as sessions, into host memory)
                if (blk[k].comp_len > xlzmany::kMaxDeviceBlock || blk[k].uncomp_len > xlzmany::kMaxDeviceBlock) st = XLZ_ERR_UNSUPPORTED;
            if (st != XLZ_OK) {
                blk.resize(b0), fs.resize(s0);
            } else {
                for (size_t k = s0; k < fs.size(); k++) fs[k].stream += b0; // (block of the file -> stream of the batch)
                in_batch[i] = 1, n_blocks[i] = nb, totals[i] = total;
                results[i].blocks = nb;
                for (size_t k = b0; k < blk.size(); k++) results[i].comp_bytes += blk[k].comp_len;
                ms.blocks += nb, ms.comp_bytes += results[i].comp_bytes;
            }
        }
        results[i].status = st;
    }
    const xlzmany::Map m = xlzmany::map_streams(in_batch.data(), n_blocks.data(), n);
    const size_t S = blk.size(); // == m.file_of.size()
    xlz_internal_check_stats_reset(ctx), xlz_internal_sha256_stats_reset(ctx), xlz_internal_filter_stats_reset(ctx);
    xlz_internal_pack_stats_reset(ctx);
    // ---- the batch: as xz_decode makes it for one file; where the checks come from as there (cmode)
    std::vector<xlz_stream_desc> d(S);
    std::vector<xlz_result> r(S);
    std::vector<uint64_t> want_out(device ? S : 0), want_in(device ? S : 0), dst_off(device ? S : 0);
    for (size_t s = 0; s < S; s++) {
        // (inside the window: the index's total fits dst_cap; a block of no bytes has no place -- its window may be one of no
        //  bytes, which may point anywhere)
        const uint64_t at = blk[s].uncomp_len ? files[m.file_of[s]].dst_off + blk[s].uncomp_off : 0;
        memset(&r[s], 0, sizeof r[s]);
        d[s] = block_desc(files[m.file_of[s]].file, blk[s], device ? nullptr : out + at);
        if (device) want_out[s] = blk[s].uncomp_len, want_in[s] = blk[s].comp_len, dst_off[s] = at;
    }
    const int cmode = !verify ? 0 : device ? 2 : xlz_ctx_check_mode(ctx);
    const bool dev = cmode == 1 || cmode == 2;
    BlockChecks ck = block_checks(S, cmode, [&](size_t s) -> const xlz_xz_block & { return blk[s]; });
    const PostWork w = ck.work(fs.data(), fs.size());
    int st = XLZ_OK;
    if (S && device) {
        DeviceDest dest;
        dest.d_dst = d_out, dest.cap = out_cap, dest.want_out = want_out.data(), dest.want_in = want_in.data(), dest.dst_off = dst_off.data();
        dest.tolerant = true;
        st = xlz_internal_decode_device(ctx, d.data(), S, r.data(), w, dest);
    } else if (S)
        st = xlz_internal_decode_batch(ctx, d.data(), S, r.data(), w);
    if (st != XLZ_OK) { // the batch could not run: nobody has a result
        for (size_t i = 0; i < n; i++) results[i].status = st;
        ms.failed_files = n;
        xlz_internal_xz_many_stats_set(ctx, ms);
        return st;
    }
    // ---- per stream: what the block did, what its check says; per file: the fold
    std::vector<int32_t> block_st(S);
    std::vector<uint8_t> check(S, xlzmany::kCheckGood);
    for (size_t s = 0; s < S; s++) block_st[s] = xlzmany::block_status(r[s].status, r[s].out_len, r[s].in_consumed, blk[s].uncomp_len, blk[s].comp_len);
    if (verify)
        xlzpost::parallel_for(S, xlzpost::host_thread_cap(16), [&](size_t s) {
            if (block_st[s] >= 0) check[s] = block_check(files[m.file_of[s]].file, blk[s], ck, s, d[s].out); // (the device form: no out, every check is the device's)
        });
    for (size_t s = 0; s < S && verify && dev && !ck.sha; s++) // (check mode 1: the SHA-256 blocks stayed with the host threads above)
        if (blk[s].check_type == 10 && block_st[s] >= 0) xlz_internal_check_stats_host(ctx, 1, blk[s].uncomp_len);
    for (size_t i = 0; i < n; i++) {
        if (in_batch[i]) {
            const xlzmany::Verdict v = xlzmany::fold(block_st.data(), check.data(), m.first[i], m.count[i], verify != 0);
            results[i].status = v.status, results[i].unverified = v.unverified;
            if (v.status == XLZ_OK) results[i].out_len = totals[i], ms.decoded_bytes += totals[i];
        }
        ms.failed_files += results[i].status != XLZ_OK;
    }
    xlz_internal_xz_many_stats_set(ctx, ms);
    return XLZ_OK;
}

extern "C" int xlz_xz_decode_many(xlz_ctx *ctx, const xlz_xz_many_file *files, size_t n, uint8_t *out, size_t out_cap, int verify,
                                  xlz_xz_many_result *results)
{
    return xz_many(ctx, files, n, out, nullptr, false, out_cap, verify, results);
}

extern "C" int xlz_xz_decode_many_device(xlz_ctx *ctx, const xlz_xz_many_file *files, size_t n, void *d_out, size_t out_cap, int verify,
                                         xlz_xz_many_result *results)
{
    return xz_many(ctx, files, n, nullptr, d_out, true, out_cap, verify, results);
}
