// xlz_zip.h -- what the table of a .zip archive and the extraction of chosen entries (xlz_zip_open / xlz_zip_extract,
// xlz_zip.hip) decide without a device: where the end record is, the ZIP64 end record behind its locator, how far the
// archive is shifted by bytes in front of it, the central directory walked into a table, every entry resolved against
// its LOCAL header and classed (supported / unsupported / bad), whether the windows in the destination are well formed
// and how they are laid out, the batch streams, the stored spans, the pack items, the check ranges, and how stream
// outcomes and digests fold into a verdict per wanted entry.
// Written from PKWARE's APPNOTE.TXT (sections 4.3 - 4.5; method 14: section 5.8).  Plain C++, no HIP and no library calls
// (tests/c/zip_selftest.cpp runs it without a GPU); not part of the C ABI.
//
// Every entry of a ZIP archive is a stream of its own: nothing here looks for parallelism, it is there by construction.
//
// Names are handed out AS STORED in the archive, each NUL-terminated in one pool: no separator is normalised, no ".."
// removed, no code page applied.  The library writes no files; a caller that does must not trust a name as a path.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/xlz.h"
#include "xlz_windows.h"

namespace xlzzip {

constexpr size_t kEndLen = 22, kLocatorLen = 20, kEnd64Len = 56, kCentralLen = 46, kLocalLen = 30;
constexpr size_t kEndSearch = kEndLen + 65535; // the end record and the longest comment: where the search ends
constexpr uint32_t kSigEnd = 0x06054b50, kSigLocator = 0x07064b50, kSigEnd64 = 0x06064b50, kSigCentral = 0x02014b50, kSigLocal = 0x04034b50;
constexpr uint16_t kStored = 0, kDeflate = 8, kLzma = 14;
constexpr size_t kLzmaHead = 9; // method 14: version (2), property size (2) = 5, lc/lp/pb (1), dictionary size (4)
constexpr uint64_t kMaxDeviceEntry = 0xFFFF0000ull; // what a unit's 32-bit counters hold (xlz_7z_files.h: kMaxDeviceFolder)
constexpr uint64_t kDestStream = ~(uint64_t)0;      // xlz_post.h: a check range over the destination

inline uint16_t le16(const uint8_t *p) { return (uint16_t)(p[0] | p[1] << 8); }
inline uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline uint64_t le64(const uint8_t *p) { return (uint64_t)le32(p) | (uint64_t)le32(p + 4) << 32; }

// ---------------------------------------------------------------- the end record ----
// The last PK\5\6 at a position p of the last kEndSearch bytes with p + 22 + comment_len <= len: bytes behind the comment
// are tolerated.  false: there is none.
inline bool find_end(const uint8_t *f, size_t len, size_t *pos)
{
    if (len < kEndLen) return false;
    const size_t lowest = len > kEndSearch ? len - kEndSearch : 0;
    for (size_t p = len - kEndLen + 1; p-- > lowest;)
        if (le32(f + p) == kSigEnd && (size_t)le16(f + p + 20) <= len - kEndLen - p) {
            *pos = p;
            return true;
        }
    return false;
}

struct End {
    uint64_t n_entries = 0, cd_size = 0, cd_off = 0; // as declared
    uint64_t cd_pos = 0;                             // where the central directory was found
    uint64_t shift = 0;                              // cd_pos - cd_off: the bytes in front of the archive
    bool zip64 = false;
};

// XLZ_OK; XLZ_ERR_UNEXPECTED_EOF: the file is shorter than an end record, or the central directory is cut (it is longer
// than what lies in front of the end record); XLZ_ERR_RESULT: no end record, a locator that leads to no ZIP64 end record,
// a directory that would begin in front of its declared offset; XLZ_ERR_UNSUPPORTED: a multi-disk archive.
// The central directory is taken to END where the end record (the ZIP64 one, where there is one) begins, as Python's
// zipfile takes it: that is what makes prepended bytes (self-extractor stubs) harmless.
inline int read_end(const uint8_t *f, size_t len, End &e)
{
    e = End{};
    if (len < kEndLen) return XLZ_ERR_UNEXPECTED_EOF;
    size_t p;
    if (!find_end(f, len, &p)) return XLZ_ERR_RESULT;
    uint64_t disk = le16(f + p + 4), cd_disk = le16(f + p + 6), n_here = le16(f + p + 8), n_all = le16(f + p + 10);
    e.cd_size = le32(f + p + 12), e.cd_off = le32(f + p + 16);
    uint64_t dir_end = p;
    if (p >= kLocatorLen && le32(f + p - kLocatorLen) == kSigLocator) {
        const uint8_t *l = f + p - kLocatorLen;
        if (le32(l + 4) != 0 || le32(l + 16) > 1) return XLZ_ERR_UNSUPPORTED;
        // the ZIP64 end record: where the locator says, else (bytes in front of the archive) right in front of the locator
        const uint64_t declared = le64(l + 8), room = p - kLocatorLen;
        uint64_t q = ~(uint64_t)0;
        if (declared <= room && room - declared >= kEnd64Len && le32(f + declared) == kSigEnd64)
            q = declared;
        else if (room >= kEnd64Len && le32(f + room - kEnd64Len) == kSigEnd64)
            q = room - kEnd64Len;
        if (q == ~(uint64_t)0) return XLZ_ERR_RESULT;
        const uint8_t *z = f + q;
        disk = le32(z + 16), cd_disk = le32(z + 20), n_here = le64(z + 24), n_all = le64(z + 32);
        e.cd_size = le64(z + 40), e.cd_off = le64(z + 48);
        e.zip64 = true, dir_end = q;
    }
    if (disk || cd_disk || n_here != n_all) return XLZ_ERR_UNSUPPORTED;
    e.n_entries = n_all;
    if (e.cd_size > dir_end) return XLZ_ERR_UNEXPECTED_EOF;
    e.cd_pos = dir_end - e.cd_size;
    // (Info-ZIP's zip -fz writes an all-ones offset and no ZIP64 end record to hold the real one: the offset is not told,
    //  the directory is where it was found and nothing is taken to lie in front of the archive)
    if (!e.zip64 && e.cd_off == 0xFFFFFFFFull) e.cd_off = e.cd_pos;
    if (e.cd_off > e.cd_pos) return XLZ_ERR_RESULT;
    e.shift = e.cd_pos - e.cd_off;
    return XLZ_OK;
}

// ---------------------------------------------------------------- the entries ----
inline bool is_dir(const xlz_zip_entry &x) { return (x.flags & XLZ_ZIP_ENTRY_IS_DIR) != 0; }
inline bool has_bytes(const xlz_zip_entry &x) { return !is_dir(x) && x.size != 0; }
// what the library does not decode, by the central directory's fields alone
inline bool unsupported(const xlz_zip_entry &x)
{
    if (x.method != kStored && x.method != kLzma) return true;
    if (x.gp_flags & (1u | 1u << 5 | 1u << 6)) return true; // encrypted, patched data, strong encryption
    if (x.method == kStored && x.comp_size != x.size) return true;
    return x.size > kMaxDeviceEntry || x.comp_size > kMaxDeviceEntry;
}

// The ZIP64 extended information (0x0001) among a central record's extra fields: the values that are all-ones in the
// record, in the fixed order size, compressed size, offset.  -> 0: there is no such field; 1: read; -1: it is too short
// for the values it must hold.  A field list that overruns its span ends the search.
inline int zip64_extra(const uint8_t *x, size_t m, uint64_t &size, uint64_t &comp, uint64_t &off)
{
    for (size_t at = 0; at + 4 <= m;) {
        const uint16_t id = le16(x + at), n = le16(x + at + 2);
        if (n > m - at - 4) return 0;
        if (id != 0x0001) {
            at += 4 + (size_t)n;
            continue;
        }
        const uint8_t *v = x + at + 4;
        size_t k = 0;
        for (uint64_t *field : {&size, &comp, &off}) {
            if (*field != 0xFFFFFFFFull) continue;
            if (k + 8 > n) return -1;
            *field = le64(v + k), k += 8;
        }
        return 1;
    }
    return 0;
}

// One PK\1\2 record at f + pos, inside [pos, end): its fields -> x, its name -> the pool.  *next: the record behind it.
// XLZ_ERR_UNEXPECTED_EOF: it does not fit in front of `end`; XLZ_ERR_RESULT: another signature.
inline int read_central(const uint8_t *f, uint64_t pos, uint64_t end, xlz_zip_entry &x, std::vector<char> &names, uint64_t *next, bool *bad64)
{
    if (end - pos < kCentralLen) return XLZ_ERR_UNEXPECTED_EOF;
    const uint8_t *c = f + pos;
    if (le32(c) != kSigCentral) return XLZ_ERR_RESULT;
    const uint64_t n = le16(c + 28), m = le16(c + 30), k = le16(c + 32);
    if (end - pos - kCentralLen < n + m + k) return XLZ_ERR_UNEXPECTED_EOF;
    memset(&x, 0, sizeof x);
    x.gp_flags = le16(c + 8), x.method = le16(c + 10);
    x.dos_time_date = (uint32_t)le16(c + 12) | (uint32_t)le16(c + 14) << 16;
    x.crc = le32(c + 16), x.comp_size = le32(c + 20), x.size = le32(c + 24);
    x.external_attr = le32(c + 38), x.header_off = le32(c + 42);
    const int z = zip64_extra(c + kCentralLen + n, (size_t)m, x.size, x.comp_size, x.header_off);
    *bad64 = z < 0;
    if (z) x.flags |= XLZ_ZIP_ENTRY_ZIP64;
    x.name_off = names.size(), x.name_len = (uint32_t)n;
    names.insert(names.end(), (const char *)c + kCentralLen, (const char *)c + kCentralLen + n);
    names.push_back('\0');
    if (n && c[kCentralLen + n - 1] == '/') x.flags |= XLZ_ZIP_ENTRY_IS_DIR;
    if (x.gp_flags & 1u << 11) x.flags |= XLZ_ZIP_ENTRY_UTF8;
    if (x.gp_flags & (1u | 1u << 6)) x.flags |= XLZ_ZIP_ENTRY_ENCRYPTED;
    if (x.gp_flags & 1u << 3) x.flags |= XLZ_ZIP_ENTRY_HAS_DESCRIPTOR;
    if (x.method == kLzma && (x.gp_flags & 1u << 1)) x.flags |= XLZ_ZIP_ENTRY_END_MARKER;
    *next = pos + kCentralLen + n + m + k;
    return XLZ_OK;
}

// An entry against its local header (x.header_off: as declared, not shifted yet) and its payload.  Sizes and CRC stay
// the central directory's: a local header written in front of a data descriptor holds zeros.  Sets header_off, data_off,
// props, dict_size and the class bits.
inline void resolve(const uint8_t *f, size_t len, const End &e, bool bad64, xlz_zip_entry &x)
{
    bool bad = bad64;
    const uint64_t declared = x.header_off;
    if (declared > ~(uint64_t)0 - e.shift) bad = true;
    x.header_off = bad ? declared : declared + e.shift;
    if (!bad && (x.header_off > len || len - x.header_off < kLocalLen || le32(f + x.header_off) != kSigLocal)) bad = true;
    if (bad) {
        x.data_off = 0;
    } else {
        // (from the LOCAL header's own lengths: its extra field is not the central record's)
        x.data_off = x.header_off + kLocalLen + le16(f + x.header_off + 26) + le16(f + x.header_off + 28);
        if (x.data_off > e.cd_pos || x.comp_size > e.cd_pos - x.data_off) bad = true;
    }
    if (!bad && x.method == kLzma) {
        const uint8_t *p = f + x.data_off;
        if (x.comp_size < kLzmaHead || le16(p + 2) != 5 || p[4] >= 225)
            bad = true;
        else
            x.props = p[4], x.dict_size = le32(p + 5);
    }
    if (bad) x.flags |= XLZ_ZIP_ENTRY_BAD;
    if (!bad && !unsupported(x)) x.flags |= XLZ_ZIP_ENTRY_SUPPORTED;
    // a bit beside the classes, which stay as they were: what deflate mode 1 / 2 inflates (open has no context to ask)
    if (!bad && x.method == kDeflate && !(x.gp_flags & (1u | 1u << 5 | 1u << 6)) && x.size < kMaxDeviceEntry && x.comp_size < kMaxDeviceEntry)
        x.flags |= XLZ_ZIP_ENTRY_DEFLATE;
}

struct Table {
    End end;
    std::vector<xlz_zip_entry> entries;
    std::vector<char> names;
    uint64_t total_size = 0; // the sum of the sizes of the entries that have bytes (saturating)
};

// The whole of xlz_zip_open but the handle.  Beyond read_end: XLZ_ERR_UNEXPECTED_EOF -- a record does not fit into the
// directory's size; XLZ_ERR_RESULT -- a record without signature, or the records do not fill the directory's size
// exactly (a count that disagrees).  No entry's defect fails it.
inline int parse(const uint8_t *f, size_t len, Table &t)
{
    t = Table{};
    if (!f) return len ? XLZ_ERR_BAD_ARG : XLZ_ERR_UNEXPECTED_EOF;
    int st = read_end(f, len, t.end);
    if (st != XLZ_OK) return st;
    const uint64_t end = t.end.cd_pos + t.end.cd_size;
    if (t.end.n_entries > t.end.cd_size / kCentralLen) return XLZ_ERR_RESULT; // (no allocation the span cannot back)
    t.entries.resize((size_t)t.end.n_entries);
    uint64_t pos = t.end.cd_pos;
    for (xlz_zip_entry &x : t.entries) {
        bool bad64 = false;
        st = read_central(f, pos, end, x, t.names, &pos, &bad64);
        if (st != XLZ_OK) return st;
        resolve(f, len, t.end, bad64, x);
        if (has_bytes(x)) t.total_size = x.size > ~(uint64_t)0 - t.total_size ? ~(uint64_t)0 : t.total_size + x.size;
    }
    return pos == end ? XLZ_OK : XLZ_ERR_RESULT;
}

// ---------------------------------------------------------------- windows ----
// false: an entry index outside the table; the window [dst_off, dst_off + dst_cap) of an entry with bytes does not fit
// in out_cap (no sum is formed unless it fits); two such windows share a byte.  The window of an entry without bytes, and
// one with dst_cap == 0, declares no byte, wherever its dst_off points.
inline bool wants_ok(const xlz_zip_entry *e, size_t ne, const xlz_zip_want *w, size_t n, uint64_t out_cap)
{
    std::vector<xlzwin::Window> win;
    for (size_t i = 0; i < n; i++) {
        if (w[i].entry >= ne) return false;
        if (has_bytes(e[w[i].entry]) && w[i].dst_cap) win.emplace_back(w[i].dst_off, w[i].dst_cap);
    }
    return xlzwin::disjoint_within(std::move(win), out_cap);
}

// Windows of the wanted entries' sizes back to back, in want order: dst_off = the first multiple of align (>= 1) at or
// behind the end of the window before, *total = the end of the last one.  false: an offset or an end does not fit 64 bits.
inline bool layout(const xlz_zip_entry *e, xlz_zip_want *w, size_t n, uint64_t align, uint64_t *total)
{
    std::vector<uint64_t> size(n), off(n);
    for (size_t i = 0; i < n; i++) size[i] = has_bytes(e[w[i].entry]) ? e[w[i].entry].size : 0;
    if (!xlzwin::back_to_back(size.data(), n, align, off.data(), total)) return false;
    for (size_t i = 0; i < n; i++) w[i].dst_off = off[i], w[i].dst_cap = size[i];
    return true;
}

// ---------------------------------------------------------------- the plan of an extraction ----
constexpr size_t kNone = ~(size_t)0;
struct Span { // a stored entry's bytes: file + src_off -> dst
    uint64_t dst, src_off, len;
};
struct Plan {
    std::vector<int32_t> pre;            // per want: XLZ_OK, or what settles it before the batch
    std::vector<xlz_stream_desc> streams; // the wanted method-14 entries that are left, in want order: descriptors INTO the file
    std::vector<size_t> stream_want;      // as streams: the want
    std::vector<xlz_pack_item> items;     // as streams: the whole stream -> dst[want]
    std::vector<Span> spans;              // the wanted stored entries that are left
    std::vector<size_t> span_want;        // as spans: the want
    std::vector<xlz_inflate_item> inflate; // deflate mode 1 / 2: the wanted deflate entries that are left, INTO the file -> dst[want]
    std::vector<size_t> inflate_want;      // as inflate: the want
};

// dst[i]: where want i's bytes go (the window's dst_off, or its place in the staging block).  deflate_mode 0: a deflate
// entry is unsupported, as every entry of another method is
inline void plan(const uint8_t *file, const xlz_zip_entry *e, const xlz_zip_want *w, const uint64_t *dst, size_t n, Plan &p, int deflate_mode = 0)
{
    p = Plan{};
    p.pre.assign(n, XLZ_OK);
    for (size_t i = 0; i < n; i++) {
        const xlz_zip_entry &x = e[w[i].entry];
        if (!has_bytes(x)) continue;
        if (w[i].dst_cap < x.size) {
            p.pre[i] = XLZ_ERR_OUT_CAP;
        } else if (deflate_mode && (x.flags & XLZ_ZIP_ENTRY_DEFLATE)) {
            p.inflate.push_back(xlz_inflate_item{file + x.data_off, x.comp_size, dst[i], x.size}), p.inflate_want.push_back(i);
        } else if (unsupported(x)) {
            p.pre[i] = XLZ_ERR_UNSUPPORTED;
        } else if (x.flags & XLZ_ZIP_ENTRY_BAD) {
            p.pre[i] = XLZ_ERR_RESULT;
        } else if (x.method == kStored) {
            p.spans.push_back(Span{dst[i], x.data_off, x.size}), p.span_want.push_back(i);
        } else {
            xlz_stream_desc d;
            memset(&d, 0, sizeof d);
            d.in = file + x.data_off + kLzmaHead, d.in_len = (size_t)(x.comp_size - kLzmaHead), d.out_cap = (size_t)x.size;
            d.format = XLZ_FMT_LZMA_RAW, d.props = x.props, d.dict_size = x.dict_size;
            // an end marker closes the stream: the size is not told, the room is the size; else the stream ends AT the size
            d.unpack_size = (x.flags & XLZ_ZIP_ENTRY_END_MARKER) ? ~(uint64_t)0 : x.size;
            p.items.push_back(xlz_pack_item{p.streams.size(), 0, x.size, dst[i]});
            p.streams.push_back(d), p.stream_want.push_back(i);
        }
    }
}

// The CRC32 ranges of a verifying call and per want its range (kNone: none): a method-14 entry over its stream, a stored
// or a deflate entry over its bytes where they lie in the destination.
inline void check_ranges(const Plan &p, size_t n, std::vector<xlz_check_range> &cr, std::vector<size_t> &range_of)
{
    cr.clear(), range_of.assign(n, kNone);
    xlz_check_range c;
    memset(&c, 0, sizeof c);
    c.kind = XLZ_CHECK_CRC32;
    for (size_t k = 0; k < p.streams.size(); k++) {
        c.stream = k, c.off = 0, c.len = p.items[k].len;
        range_of[p.stream_want[k]] = cr.size(), cr.push_back(c);
    }
    for (size_t k = 0; k < p.spans.size(); k++) {
        c.stream = kDestStream, c.off = p.spans[k].dst, c.len = p.spans[k].len;
        range_of[p.span_want[k]] = cr.size(), cr.push_back(c);
    }
    for (size_t k = 0; k < p.inflate.size(); k++) {
        c.stream = kDestStream, c.off = p.inflate[k].dst_off, c.len = p.inflate[k].dst_cap;
        range_of[p.inflate_want[k]] = cr.size(), cr.push_back(c);
    }
}

// ---------------------------------------------------------------- the verdict ----
// What a method-14 entry's stream says of it: XLZ_OK where it ended with a status >= 0 and exactly the entry's size; its
// own status where that is negative -- but XLZ_ERR_OUT_CAP from an end-marker stream, which only wanted to go on behind
// the declared size: XLZ_ERR_RESULT; XLZ_ERR_RESULT otherwise.
inline int32_t stream_status(const xlz_zip_entry &x, int32_t status, uint64_t out_len)
{
    if (status < 0) return status == XLZ_ERR_OUT_CAP && (x.flags & XLZ_ZIP_ENTRY_END_MARKER) ? (int32_t)XLZ_ERR_RESULT : status;
    return out_len == x.size ? (int32_t)XLZ_OK : (int32_t)XLZ_ERR_RESULT;
}

// What a deflate entry's item says of it: its own status where that is negative -- but XLZ_ERR_OUT_CAP, from a stream that only
// wanted to go on behind the declared size: XLZ_ERR_RESULT, as for end-marker streams; XLZ_OK where it produced exactly the
// entry's size; XLZ_ERR_RESULT otherwise.
inline int32_t inflate_status(const xlz_zip_entry &x, int32_t status, uint64_t produced)
{
    if (status < 0) return status == XLZ_ERR_OUT_CAP ? (int32_t)XLZ_ERR_RESULT : status;
    return produced == x.size ? (int32_t)XLZ_OK : (int32_t)XLZ_ERR_RESULT;
}

enum : uint8_t { kDigestGood = 0, kDigestBad = 1, kDigestNone = 2 }; // (none: verify is off)

// pre: Plan::pre; stream_st: stream_status of its stream (XLZ_OK for a stored entry); digest: of the entry's bytes.
// In this order: what settled it before the batch; an entry without bytes is good; its stream; its CRC32.
inline xlz_zip_file_result verdict(int32_t pre, const xlz_zip_entry &x, int32_t stream_st, uint8_t digest, bool verify)
{
    if (!has_bytes(x)) return {XLZ_OK, 0, 0};
    if (pre < 0) return {pre, 0, 0};
    if (stream_st < 0) return {stream_st, 0, 0};
    if (verify && digest == kDigestBad) return {XLZ_ERR_RESULT, 0, 0};
    return {XLZ_OK, 0, x.size};
}

} // namespace xlzzip

// What xlz_zip_open makes and the extraction reads (xlz_zip.hip); never changed after open.
struct xlz_zip_archive {
    const uint8_t *file = nullptr; // borrowed: the caller keeps it alive
    size_t len = 0;
    xlzzip::Table t;
};
