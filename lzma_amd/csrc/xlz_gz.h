// xlz_gz.h -- what the gzip / BGZF / zlib front end (xlz_gz_probe / xlz_gz_decode_host / xlz_gz_decode_many, xlz_gz.hip)
// decides without a device: the member header, the zlib header, whether a file is BGZF and where its blocks lie, where the
// next member of an ordinary gzip file begins once the one before it has been inflated, which ranges are checked against
// which values, and how inflate outcomes and digests fold into a verdict per file.  decode_host() below is the serial twin
// the library exports as xlz_gz_decode_host.
// Written from RFC 1952 (gzip), RFC 1950 (zlib) and the BGZF section of the SAM specification (section 4.1).  Plain C++,
// no HIP; none of zlib's code is here, and the reference has no container code.
//
// GZIP MEMBER (RFC 1952).  ID1 ID2 = 1f 8b | CM (8 = deflate) | FLG | MTIME (4, little-endian) | XFL | OS -- ten bytes --,
// then, as FLG says: FEXTRA (bit 2): XLEN (2, LE) and XLEN bytes of subfields SI1 SI2 LEN (2, LE) data; FNAME (bit 3): a
// zero-terminated name; FCOMMENT (bit 4): a zero-terminated comment; FHCRC (bit 1): the low 16 bits of the CRC32 of every
// header byte in front of it (2, LE).  FTEXT (bit 0) means nothing here; bits 5 - 7 are reserved.  Then the deflate stream,
// then the trailer: CRC32 of the decoded bytes (4, LE) and ISIZE, their number mod 2^32 (4, LE).
//   wrong magic -> XLZ_ERR_RESULT; CM != 8 -> XLZ_ERR_UNSUPPORTED; a reserved FLG bit -> XLZ_ERR_UNSUPPORTED; the input
//   ends inside header or trailer -> XLZ_ERR_UNEXPECTED_EOF; with verify on, an FHCRC that differs -> XLZ_ERR_RESULT (with
//   verify off it is not compared).  The subfields of FEXTRA are only LOOKED THROUGH for "BC": one that leaves XLEN ends
//   the search and is no error.
// A FILE is one or more members.  Behind a member's trailer zero bytes are skipped; where the input then ends the file
// ends, a further 1f 8b starts the next member, and anything else fails the file with XLZ_ERR_RESULT -- what Python's
// gzip.decompress does.
// ZLIB STREAM (RFC 1950).  CMF | FLG, then the deflate stream, then the Adler-32 of the decoded bytes (4, BIG-endian).
// CMF: CM = low nibble = 8, CINFO = high nibble <= 7; (CMF * 256 + FLG) % 31 == 0; FLG bit 5 = FDICT.  Any defect of these
// is XLZ_ERR_RESULT; an otherwise sound header with FDICT is XLZ_ERR_UNSUPPORTED.  Input behind the trailer is ignored and
// in_consumed says where the stream ended -- what zlib.decompressobj does.
// BGZF.  Every block is a gzip member of at most 64 KiB of data whose FEXTRA holds the subfield 'B' 'C' of length 2:
// BSIZE, the block's total size - 1.  If the chain of BSIZE values walks from offset 0 exactly to the end of the input --
// zero bytes behind the last block allowed, as behind any member -- and every block's ISIZE (at block_end - 4) is at most
// 65536, the file is BGZF and every block is known without inflating a byte: its deflate body is [header_end,
// block_end - 8), its window is exactly ISIZE bytes behind the windows of the blocks in front of it.  Otherwise the file
// is ordinary gzip: member k + 1 begins where member k's deflate stream ended, so it is known only after member k has
// been inflated.
//
// VERDICT.  A file is XLZ_OK only if every member inflated XLZ_OK, each member produced ISIZE bytes (mod 2^32), each BGZF
// block's deflate stream used exactly its announced body, and -- with verify on -- every CRC32 / Adler-32 matches.  A
// mismatch is XLZ_ERR_RESULT, and so is ANY failure of a BGZF block (one that overflows the window its ISIZE announces
// included).  XLZ_ERR_OUT_CAP means that the FILE's dst_cap is too small.  The first defect in stream order decides: a
// member's wrong check value comes before anything a later member does.  A failed file has out_len 0, in_consumed 0.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/xlz.h"
#include "xlz_adler_dev.h"
#include "xlz_check.h"
#include "xlz_inflate_dev.h"

namespace xlzgz {

constexpr uint32_t kFtext = 1, kFhcrc = 2, kFextra = 4, kFname = 8, kFcomment = 16, kFreserved = 0xE0;
constexpr uint64_t kMaxBgzfIsize = 65536;

inline uint16_t le16(const uint8_t *p) { return (uint16_t)(p[0] | p[1] << 8); }
inline uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline uint32_t be32(const uint8_t *p) { return (uint32_t)p[3] | (uint32_t)p[2] << 8 | (uint32_t)p[1] << 16 | (uint32_t)p[0] << 24; }

struct Header {
    uint64_t end = 0;       // where the deflate stream begins (an offset into the input, like `at`)
    uint32_t flags = 0;     // XLZ_GZ_F_NAME / _COMMENT / _HCRC
    uint32_t mtime = 0, name_off = 0, name_len = 0;
    bool has_bsize = false; // a subfield 'B' 'C' of length 2
    uint32_t bsize = 0;
};

// the member header at in + at
inline int gzip_header(const uint8_t *in, uint64_t len, uint64_t at, bool verify, Header &h)
{
    h = Header{};
    const uint64_t have = len - at;
    if (have < 2) return XLZ_ERR_UNEXPECTED_EOF;
    if (in[at] != 0x1f || in[at + 1] != 0x8b) return XLZ_ERR_RESULT;
    if (have < 3) return XLZ_ERR_UNEXPECTED_EOF;
    if (in[at + 2] != 8) return XLZ_ERR_UNSUPPORTED;
    if (have < 4) return XLZ_ERR_UNEXPECTED_EOF;
    const uint32_t flg = in[at + 3];
    if (flg & kFreserved) return XLZ_ERR_UNSUPPORTED;
    if (have < 10) return XLZ_ERR_UNEXPECTED_EOF;
    h.mtime = le32(in + at + 4);
    uint64_t p = at + 10;
    if (flg & kFextra) {
        if (len - p < 2) return XLZ_ERR_UNEXPECTED_EOF;
        const uint64_t xlen = le16(in + p);
        p += 2;
        if (len - p < xlen) return XLZ_ERR_UNEXPECTED_EOF;
        for (uint64_t q = p; p + xlen - q >= 4;) { // (a subfield that leaves XLEN ends the search)
            const uint64_t sl = le16(in + q + 2);
            if (sl > p + xlen - q - 4) break;
            if (in[q] == 'B' && in[q + 1] == 'C' && sl == 2 && !h.has_bsize) h.has_bsize = true, h.bsize = le16(in + q + 4);
            q += 4 + sl;
        }
        p += xlen;
    }
    for (uint32_t f : {kFname, kFcomment}) {
        if (!(flg & f)) continue;
        const void *z = p < len ? memchr(in + p, 0, (size_t)(len - p)) : nullptr;
        if (!z) return XLZ_ERR_UNEXPECTED_EOF;
        const uint64_t zero = (uint64_t)(static_cast<const uint8_t *>(z) - in);
        if (f == kFname) h.name_off = (uint32_t)(p < 0xFFFFFFFFull ? p : 0), h.name_len = (uint32_t)(zero - p < 0xFFFFFFFFull ? zero - p : 0), h.flags |= XLZ_GZ_F_NAME;
        else h.flags |= XLZ_GZ_F_COMMENT;
        p = zero + 1;
    }
    if (flg & kFhcrc) {
        if (len - p < 2) return XLZ_ERR_UNEXPECTED_EOF;
        h.flags |= XLZ_GZ_F_HCRC;
        if (verify && (xlzcheck::crc32(in + at, (size_t)(p - at)) & 0xFFFF) != le16(in + p)) return XLZ_ERR_RESULT;
        p += 2;
    }
    h.end = p;
    return XLZ_OK;
}

// the two bytes of a zlib header
inline int zlib_header(const uint8_t *in, uint64_t len)
{
    if (len < 2) return XLZ_ERR_UNEXPECTED_EOF;
    const uint32_t cmf = in[0], flg = in[1];
    if ((cmf & 15) != 8 || (cmf >> 4) > 7 || (cmf * 256 + flg) % 31) return XLZ_ERR_RESULT;
    return flg & 0x20 ? XLZ_ERR_UNSUPPORTED : XLZ_OK;
}

// XLZ_GZ_AUTO: 1f 8b -> gzip, else a valid zlib header -> zlib (one with FDICT too: it is then refused as zlib), else
// XLZ_ERR_RESULT; fewer than two bytes decide nothing: XLZ_ERR_UNEXPECTED_EOF
inline int resolve_format(const uint8_t *in, uint64_t len, uint32_t format, uint32_t *out)
{
    *out = format;
    if (format == XLZ_GZ_GZIP || format == XLZ_GZ_ZLIB) return XLZ_OK;
    if (format != XLZ_GZ_AUTO) return XLZ_ERR_BAD_ARG;
    if (len < 2) return XLZ_ERR_UNEXPECTED_EOF;
    if (in[0] == 0x1f && in[1] == 0x8b) return *out = XLZ_GZ_GZIP, (int)XLZ_OK;
    if (zlib_header(in, len) == XLZ_ERR_RESULT) return XLZ_ERR_RESULT;
    return *out = XLZ_GZ_ZLIB, (int)XLZ_OK;
}

inline bool all_zero(const uint8_t *in, uint64_t from, uint64_t len)
{
    for (uint64_t i = from; i < len; i++)
        if (in[i]) return false;
    return true;
}

struct Block { // of a BGZF file
    uint64_t body, body_len; // the deflate stream: input offsets
    uint64_t out_off;        // where its ISIZE bytes lie in the file's window
    uint32_t isize, crc;
};
// true: the file is BGZF; blocks = its blocks, *total = the sum of their ISIZE, first = the first block's header
inline bool bgzf_blocks(const uint8_t *in, uint64_t len, bool verify, std::vector<Block> &blocks, uint64_t *total, Header &first)
{
    blocks.clear();
    *total = 0;
    for (uint64_t at = 0; at < len;) {
        if (!blocks.empty() && in[at] == 0) {
            if (all_zero(in, at, len)) break;
            return false;
        }
        Header h;
        if (gzip_header(in, len, at, verify, h) != XLZ_OK || !h.has_bsize) return false;
        const uint64_t size = (uint64_t)h.bsize + 1;
        if (size > len - at || at + size < h.end + 8) return false;
        const uint64_t end = at + size;
        Block b = {h.end, end - 8 - h.end, *total, le32(in + end - 4), le32(in + end - 8)};
        if (b.isize > kMaxBgzfIsize) return false;
        if (blocks.empty()) first = h;
        blocks.push_back(b);
        *total += b.isize, at = end;
    }
    return !blocks.empty();
}

// ---------------------------------------------------------------- one file's way through the rounds ----
struct Check { // bytes [off, off + len) of the file's window must have this digest
    uint64_t off, len;
    uint32_t want;
};
struct Item { // one deflate stream to inflate: input [in_off, in_off + in_len) into [dst_off, dst_off + dst_cap) of the window
    uint64_t in_off, in_len, dst_off, dst_cap;
};
struct File {
    const uint8_t *in = nullptr;
    uint64_t len = 0, cap = 0;
    uint32_t format = 0; // resolved: XLZ_GZ_GZIP / XLZ_GZ_ZLIB
    bool bgzf = false, verify = false;
    bool done = false;   // nothing more to inflate
    int32_t late = XLZ_OK; // the first defect that is no wrong check value (those come first, if they are there: stream order)
    uint64_t at = 0;       // ordinary gzip: where the next member may begin; zlib: where the stream ended
    uint64_t out_pos = 0, members = 0;
    uint64_t hdr_end = 0;  // of the member that is being inflated
    std::vector<Block> blocks;
    std::vector<Check> checks; // CRC32 (gzip) or Adler-32 (zlib), in stream order
    void fail(int32_t st) { late = st, done = true; }
};

// -> the file's state in front of round 1.  BGZF: items = every block (the file is then done); otherwise next_item() gives
// the first member
inline void open(File &f, const uint8_t *in, uint64_t len, uint32_t format, uint64_t cap, bool verify, std::vector<Item> &bgzf_items)
{
    f = File{};
    f.in = in, f.len = len, f.cap = cap, f.verify = verify;
    const int st = resolve_format(in, len, format, &f.format);
    if (st != XLZ_OK) return f.fail(st);
    if (f.format != XLZ_GZ_GZIP) return;
    uint64_t total;
    Header first;
    if (!bgzf_blocks(in, len, verify, f.blocks, &total, first)) return f.blocks.clear();
    f.bgzf = true, f.done = true;
    if (total > cap) return f.fail(XLZ_ERR_OUT_CAP);
    for (const Block &b : f.blocks) bgzf_items.push_back(Item{b.body, b.body_len, b.out_off, b.isize});
}
// BGZF: block k's outcome
inline void block_done(File &f, size_t k, int32_t status, uint64_t produced, uint64_t consumed)
{
    const Block &b = f.blocks[k];
    if (f.late != XLZ_OK) return; // (behind the first bad block nothing counts: the serial twin stops there)
    f.members++;
    if (status != XLZ_OK || produced != b.isize || consumed != b.body_len) return f.fail(XLZ_ERR_RESULT);
    if (f.verify) f.checks.push_back(Check{b.out_off, produced, b.crc});
    f.out_pos = b.out_off + produced;
}
// ordinary gzip and zlib: the next stream to inflate; false: there is none (the file is done, whatever its state)
inline bool next_item(File &f, Item &it)
{
    if (f.done) return false;
    if (f.format == XLZ_GZ_ZLIB) {
        if (f.members) return f.done = true, false;
        const int st = zlib_header(f.in, f.len);
        if (st != XLZ_OK) return f.fail(st), false;
        f.hdr_end = 2;
    } else {
        if (f.members) { // behind a member: zero bytes, then the end or another member
            while (f.at < f.len && f.in[f.at] == 0) f.at++;
            if (f.at == f.len) return f.done = true, false;
        }
        Header h;
        const int st = gzip_header(f.in, f.len, f.at, f.verify, h);
        if (st != XLZ_OK) return f.fail(st), false;
        f.hdr_end = h.end;
    }
    it = Item{f.hdr_end, f.len - f.hdr_end, f.out_pos, f.cap - f.out_pos};
    return true;
}
// ... and its outcome: the trailer, the check to make, where the next member may begin
inline void item_done(File &f, int32_t status, uint64_t produced, uint64_t consumed)
{
    if (status != XLZ_OK) return f.fail(status);
    const uint64_t t = f.hdr_end + consumed, need = f.format == XLZ_GZ_ZLIB ? 4 : 8;
    if (f.len - t < need) return f.fail(XLZ_ERR_UNEXPECTED_EOF);
    if (f.verify) f.checks.push_back(Check{f.out_pos, produced, f.format == XLZ_GZ_ZLIB ? be32(f.in + t) : le32(f.in + t)});
    f.members++, f.out_pos += produced, f.at = t + need;
    if (f.format == XLZ_GZ_GZIP && le32(f.in + t + 4) != (uint32_t)produced) return f.fail(XLZ_ERR_RESULT); // (behind its CRC32 in stream order)
}
// got[k]: the digest of f.checks[k] (only looked at with verify on) -> the file's result
inline xlz_gz_result verdict(const File &f, const uint32_t *got)
{
    xlz_gz_result r = {};
    r.status = f.late;
    for (size_t k = 0; k < f.checks.size(); k++)
        if (got[k] != f.checks[k].want) {
            r.status = XLZ_ERR_RESULT;
            break;
        }
    r.members = (uint32_t)(f.members < 0xFFFFFFFFull ? f.members : 0xFFFFFFFFull);
    if (r.status == XLZ_OK) r.out_len = f.out_pos, r.in_consumed = f.format == XLZ_GZ_ZLIB ? f.at : f.len;
    return r;
}

// ---------------------------------------------------------------- the serial twin ----
inline int decode_host(const uint8_t *in, uint64_t len, uint32_t format, uint8_t *out, uint64_t out_cap, bool verify, xlz_gz_result *r)
{
    File f;
    std::vector<Item> items;
    open(f, in, len, format, out_cap, verify, items);
    auto inflate = [&](const Item &it, int32_t *st, uint64_t *produced, uint64_t *consumed) {
        size_t p = 0, c = 0;
        *st = xlzinf::host_inflate(in + it.in_off, (size_t)it.in_len, out + it.dst_off, (size_t)it.dst_cap, &p, &c);
        *produced = p, *consumed = c;
    };
    int32_t st;
    uint64_t produced, consumed;
    for (size_t k = 0; k < items.size() && f.late == XLZ_OK; k++) {
        inflate(items[k], &st, &produced, &consumed);
        block_done(f, k, st, produced, consumed);
    }
    for (Item it; next_item(f, it);) {
        inflate(it, &st, &produced, &consumed);
        item_done(f, st, produced, consumed);
    }
    std::vector<uint32_t> got(f.checks.size());
    for (size_t k = 0; k < got.size(); k++) {
        const Check &c = f.checks[k];
        got[k] = f.format == XLZ_GZ_ZLIB ? xlzadl::host_update(1, out + c.off, (size_t)c.len) : c.len ? xlzcheck::crc32(out + c.off, (size_t)c.len) : 0;
    }
    *r = verdict(f, got.data());
    return XLZ_OK;
}

// ---------------------------------------------------------------- xlz_gz_probe ----
inline int probe(const uint8_t *in, uint64_t len, uint32_t format, xlz_gz_info *out)
{
    *out = xlz_gz_info{};
    uint32_t fmt;
    int st = resolve_format(in, len, format, &fmt);
    if (st != XLZ_OK) return st;
    out->format = fmt;
    if (fmt == XLZ_GZ_ZLIB) return zlib_header(in, len);
    Header h;
    std::vector<Block> blocks;
    uint64_t total;
    if (bgzf_blocks(in, len, false, blocks, &total, h)) {
        out->flags = h.flags | XLZ_GZ_F_BGZF, out->members = blocks.size(), out->size_hint = total;
    } else {
        st = gzip_header(in, len, 0, false, h);
        if (st != XLZ_OK) return st;
        out->flags = h.flags;
        out->size_hint = len - h.end >= 8 ? le32(in + len - 4) : 0;
    }
    out->mtime = h.mtime, out->name_off = h.name_off, out->name_len = h.name_len;
    return XLZ_OK;
}

} // namespace xlzgz
