// xlz_7z_files.h -- what the file table of a .7z archive and the extraction of chosen files (xlz_7z_open / xlz_7z_cover /
// xlz_7z_extract, xlz_7z.hip and xlz_7z_extract.hip) decide without a device: the FilesInfo section parsed over a bounded
// span, the entries mapped onto the folders' substreams, which folders a set of wanted entries needs and how much of each
// (the cover and its cuts), whether the windows in the destination are well formed and how they are laid out, the pack
// items, what a cut stream must end in, and how stream outcomes and digests fold into a verdict per wanted entry.
// Written from 7-Zip's published 7zFormat.txt.  Plain C++, no HIP and no library calls (tests/c/sevenzip_files_selftest.cpp
// runs it without a GPU); not part of the C ABI.
//
// Names are handed out AS STORED in the archive, converted to UTF-8: no separator is normalised, no ".." removed.  The
// library writes no files; a caller that does must not trust a name as a path.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/xlz.h"
#include "xlz_windows.h"

namespace xlz7zf {

constexpr uint64_t kMaxItems = 1u << 24; // folders / streams / files we are willing to index

// bounded reader over a header: never reads past the span, `bad` once it would have
struct Rd {
    const uint8_t *p;
    size_t n, pos = 0;
    bool bad = false;
    size_t left() const { return n - pos; }
    uint8_t byte()
    {
        if (pos >= n) {
            bad = true;
            return 0;
        }
        return p[pos++];
    }
    // 7z "NUMBER": the count of leading one bits of the first byte = extra bytes (little endian)
    uint64_t number()
    {
        const uint8_t first = byte();
        uint8_t mask = 0x80;
        uint64_t v = 0;
        for (int i = 0; i < 8; i++) {
            if (!(first & mask)) {
                v |= (uint64_t)(first & (mask - 1)) << (8 * i);
                return v;
            }
            v |= (uint64_t)byte() << (8 * i);
            mask >>= 1;
        }
        return v;
    }
    bool skip(uint64_t k)
    {
        if (k > n - pos) {
            bad = true;
            return false;
        }
        pos += (size_t)k;
        return true;
    }
};

// ---------------------------------------------------------------- FilesInfo ----
enum : uint8_t { kEmptyStream = 0x0E, kEmptyFile = 0x0F, kAnti = 0x10, kNames = 0x11, kMTime = 0x14, kWinAttributes = 0x15 };

struct Files {
    bool present = false; // the archive has a FilesInfo section
    uint64_t n = 0;       // NumFiles
    uint64_t n_empty = 0; // of them without a stream
    std::vector<uint8_t> empty_stream;      // n entries, or none: every entry has a stream
    std::vector<uint8_t> empty_file, anti;  // over the empty-stream entries, in order; may be shorter: the rest is 0
    std::vector<uint8_t> has_mtime, has_attr; // n entries, or none
    std::vector<uint64_t> mtime;              // as has_mtime
    std::vector<uint32_t> attr;               // as has_attr
    std::vector<char> names;                  // UTF-8, every name NUL-terminated
    std::vector<uint64_t> name_off;           // n entries, or none: every name is empty
    std::vector<uint32_t> name_len;
};

// `count` bits, MSB first; false: the span does not hold them
inline bool read_bits(Rd &r, uint64_t count, std::vector<uint8_t> &out)
{
    if ((count + 7) / 8 > r.left()) return false;
    out.assign((size_t)count, 0);
    uint8_t b = 0, mask = 0;
    for (uint64_t i = 0; i < count; i++) {
        if (!mask) b = r.byte(), mask = 0x80;
        out[(size_t)i] = (b & mask) != 0;
        mask >>= 1;
    }
    return true;
}

// kMTime / kWinAttributes: AllDefined byte, else a bit vector; an External byte; `width` bytes per defined entry, little endian
template <class T> int read_values(Rd &r, uint64_t count, unsigned width, std::vector<uint8_t> &defined, std::vector<T> &v)
{
    const uint8_t all = r.byte();
    if (r.bad) return XLZ_ERR_RESULT;
    if (!all) {
        if (!read_bits(r, count, defined)) return XLZ_ERR_RESULT;
    } else {
        if (count > r.left() / width) return XLZ_ERR_RESULT; // (no allocation the span cannot back)
        defined.assign((size_t)count, 1);
    }
    const uint8_t external = r.byte();
    if (r.bad) return XLZ_ERR_RESULT;
    if (external) return XLZ_ERR_UNSUPPORTED;
    v.assign((size_t)count, 0);
    for (uint64_t i = 0; i < count; i++) {
        if (!defined[(size_t)i]) continue;
        if (r.left() < width) return XLZ_ERR_RESULT;
        T x = 0;
        for (unsigned k = 0; k < width; k++) x |= (T)r.p[r.pos + k] << (8 * k);
        r.pos += width;
        v[(size_t)i] = x;
    }
    return XLZ_OK;
}

inline void put_utf8(std::vector<char> &pool, uint32_t c)
{
    if (c < 0x80) {
        pool.push_back((char)c);
    } else if (c < 0x800) {
        pool.push_back((char)(0xC0 | c >> 6)), pool.push_back((char)(0x80 | (c & 63)));
    } else if (c < 0x10000) {
        pool.push_back((char)(0xE0 | c >> 12)), pool.push_back((char)(0x80 | (c >> 6 & 63))), pool.push_back((char)(0x80 | (c & 63)));
    } else {
        pool.push_back((char)(0xF0 | c >> 18)), pool.push_back((char)(0x80 | (c >> 12 & 63)));
        pool.push_back((char)(0x80 | (c >> 6 & 63))), pool.push_back((char)(0x80 | (c & 63)));
    }
}

// kNames behind its External byte: UTF-16LE, every name NUL-terminated, exactly `count` of them filling the span
inline int read_names(Rd &r, uint64_t count, Files &f)
{
    if (r.left() % 2 || count > r.left() / 2) return XLZ_ERR_RESULT; // (a name takes its terminator at least)
    f.names.clear(), f.name_off.clear(), f.name_len.clear();
    f.names.reserve(r.left() / 2 * 3);
    const size_t units = r.left() / 2;
    auto unit = [&](size_t k) { return (uint32_t)r.p[r.pos + 2 * k] | (uint32_t)r.p[r.pos + 2 * k + 1] << 8; };
    size_t start = f.names.size();
    for (size_t k = 0; k < units; k++) {
        uint32_t c = unit(k);
        if (c == 0) {
            if (f.name_off.size() == count) return XLZ_ERR_RESULT; // more names than entries
            f.name_off.push_back(start), f.name_len.push_back((uint32_t)(f.names.size() - start));
            f.names.push_back('\0');
            start = f.names.size();
            continue;
        }
        if (c >= 0xD800 && c < 0xDC00 && k + 1 < units && unit(k + 1) >= 0xDC00 && unit(k + 1) < 0xE000) {
            c = 0x10000 + ((c - 0xD800) << 10) + (unit(k + 1) - 0xDC00);
            k++;
        } else if (c >= 0xD800 && c < 0xE000) {
            c = 0xFFFD; // an unpaired surrogate
        }
        put_utf8(f.names, c);
    }
    r.pos += 2 * units;
    if (start != f.names.size() || f.name_off.size() != count) return XLZ_ERR_RESULT; // an unterminated name, or too few
    return XLZ_OK;
}

// The section behind its id byte (0x05): NumFiles, then properties (type, size, data) until 0x00.  *used = the bytes read.
inline int parse_files(const uint8_t *p, size_t len, Files &f, size_t *used)
{
    Rd r{p, len};
    f = Files{};
    f.present = true;
    f.n = r.number();
    if (r.bad) return XLZ_ERR_RESULT;
    if (f.n > kMaxItems) return XLZ_ERR_UNSUPPORTED;
    for (;;) {
        const uint8_t type = r.byte();
        if (r.bad) return XLZ_ERR_RESULT;
        if (type == 0) break;
        const uint64_t size = r.number();
        if (r.bad || size > r.left()) return XLZ_ERR_RESULT;
        Rd q{p + r.pos, (size_t)size};
        r.pos += (size_t)size;
        int st = XLZ_OK;
        switch (type) {
        case kEmptyStream:
            if (!read_bits(q, f.n, f.empty_stream)) return XLZ_ERR_RESULT;
            f.n_empty = (uint64_t)std::count(f.empty_stream.begin(), f.empty_stream.end(), 1);
            break;
        case kEmptyFile:
            if (!read_bits(q, f.n_empty, f.empty_file)) return XLZ_ERR_RESULT;
            break;
        case kAnti:
            if (!read_bits(q, f.n_empty, f.anti)) return XLZ_ERR_RESULT;
            break;
        case kNames: {
            const uint8_t external = q.byte();
            if (q.bad) return XLZ_ERR_RESULT;
            if (external) return XLZ_ERR_UNSUPPORTED;
            st = read_names(q, f.n, f);
            break;
        }
        case kMTime: st = read_values(q, f.n, 8, f.has_mtime, f.mtime); break;
        case kWinAttributes: st = read_values(q, f.n, 4, f.has_attr, f.attr); break;
        default: continue; // kCTime, kATime, kStartPos, kDummy, unknown: skipped by their size
        }
        if (st != XLZ_OK) return st;
        if (q.bad || q.pos != q.n) return XLZ_ERR_RESULT; // the data overruns, or does not fill, its announced size
    }
    if (used) *used = r.pos;
    return XLZ_OK;
}

// ---------------------------------------------------------------- entries ----
// The entries that have a stream map, in order, onto the substreams, which lie folder by folder (first_substream,
// n_substreams).  XLZ_ERR_RESULT: their number is not the number of substreams.
inline int build_entries(const Files &f, const xlz_7z_folder *fo, size_t nf, const xlz_7z_substream *subs, size_t ns, std::vector<xlz_7z_entry> &e)
{
    e.clear();
    if (!f.present) return XLZ_OK;
    if (f.n < f.n_empty || f.n - f.n_empty != ns) return XLZ_ERR_RESULT;
    e.resize((size_t)f.n);
    size_t fi = 0, si = 0, ei = 0; // folder, substream, empty-stream entry
    uint64_t off = 0;
    for (size_t i = 0; i < e.size(); i++) {
        xlz_7z_entry &x = e[i];
        memset(&x, 0, sizeof x);
        if (!f.name_off.empty()) x.name_off = f.name_off[i], x.name_len = f.name_len[i];
        if (!f.has_mtime.empty() && f.has_mtime[i]) x.mtime = f.mtime[i], x.flags |= XLZ_7Z_ENTRY_HAS_MTIME;
        if (!f.has_attr.empty() && f.has_attr[i]) x.attributes = f.attr[i], x.flags |= XLZ_7Z_ENTRY_HAS_ATTRIBUTES;
        if (!f.empty_stream.empty() && f.empty_stream[i]) {
            x.folder = x.substream = XLZ_7Z_NO_FOLDER;
            if (!(ei < f.empty_file.size() && f.empty_file[ei])) x.flags |= XLZ_7Z_ENTRY_IS_DIR;
            if (ei < f.anti.size() && f.anti[ei]) x.flags |= XLZ_7Z_ENTRY_IS_ANTI;
            ei++;
            continue;
        }
        while (fi < nf && si >= (size_t)fo[fi].first_substream + fo[fi].n_substreams) fi++, off = 0;
        if (fi >= nf || si >= ns) return XLZ_ERR_RESULT; // (the folders do not account for the substreams)
        x.flags |= XLZ_7Z_ENTRY_HAS_STREAM;
        x.size = subs[si].size, x.folder = fi, x.folder_off = off, x.substream = si;
        if (subs[si].has_crc) x.crc = subs[si].crc, x.flags |= XLZ_7Z_ENTRY_HAS_CRC;
        if (x.size > fo[fi].unpack_len || off > fo[fi].unpack_len - x.size) return XLZ_ERR_RESULT;
        off += x.size, si++;
    }
    return XLZ_OK;
}

inline bool has_bytes(const xlz_7z_entry &x) { return (x.flags & XLZ_7Z_ENTRY_HAS_STREAM) && x.size; }

// ---------------------------------------------------------------- the cover ----
// How a covering folder goes into the batch, and with it what its stream must end in:
//   kWhole    all of it: a status >= 0 with exactly the folder's size
//   kCapCut   out_cap = decode_len, the input whole: XLZ_ERR_OUT_CAP with exactly decode_len bytes
//   kUnitCut  an LZMA2 folder cut behind a unit, input and output: XLZ_ERR_UNEXPECTED_EOF with exactly decode_len bytes
//             and all of in_len used (what a slice that ends before its stream does ends in: xlz.h, XLZ_STREAM_F_LZMA2_SLICE)
enum : uint8_t { kWhole = 0, kCapCut = 1, kUnitCut = 2 };
struct Cut {
    uint64_t decode_len, in_len;
    uint8_t kind;
};

// P = how far the last wanted entry reaches into the folder's bytes (> 0).  steps: the folder has filter steps.  u: the
// units of an LZMA2 folder's payload (xlz_lzma2_units; nu == 0: not known).  A unit table that does not lie back to back
// from 0 or does not add up to the folder's size is not trusted: whole.
inline Cut cut_folder(uint32_t method, bool steps, uint64_t unpack_len, uint64_t pack_len, const xlz_lzma2_unit *u, size_t nu, uint64_t P)
{
    const Cut whole = {unpack_len, pack_len, kWhole};
    if (steps || P >= unpack_len || P == 0) return whole;
    if (method == XLZ_7Z_LZMA) return {P, pack_len, kCapCut};
    if (method != XLZ_7Z_LZMA2 || nu == 0) return whole;
    if (nu == 1) return {P, pack_len, kCapCut};
    uint64_t in_at = 0, out_at = 0;
    for (size_t k = 0; k < nu; k++) {
        if (u[k].in_off != in_at || u[k].out_off != out_at || u[k].in_len > pack_len - in_at || u[k].out_len > unpack_len - out_at) return whole;
        in_at += u[k].in_len, out_at += u[k].out_len;
    }
    if (out_at != unpack_len) return whole;
    for (size_t k = 0; k + 1 < nu; k++)
        if (u[k + 1].out_off >= P) { // unit k holds byte P - 1 (behind it only empty units: nothing to save)
            if (u[k + 1].out_off >= unpack_len) return whole;
            return {u[k + 1].out_off, u[k + 1].in_off, kUnitCut};
        }
    return whole; // the last unit holds it
}

// Per folder: how far the wanted entries reach (0: no wanted entry has bytes in it).  want_ok (optional): entry i of the
// list counts only where want_ok[i] != 0.
inline void reach(const xlz_7z_entry *e, const uint64_t *wanted, const uint8_t *want_ok, size_t n, size_t nf, std::vector<uint64_t> &P)
{
    P.assign(nf, 0);
    for (size_t i = 0; i < n; i++) {
        const xlz_7z_entry &x = e[wanted[i]];
        if ((want_ok && !want_ok[i]) || !has_bytes(x)) continue;
        P[(size_t)x.folder] = std::max(P[(size_t)x.folder], x.folder_off + x.size);
    }
}

// What a cut stream's outcome says of its folder: XLZ_OK where it is the one outcome of its kind, a negative status of
// its own where that is another one than the expected, XLZ_ERR_RESULT otherwise.
inline int32_t stream_status(const Cut &c, int32_t status, uint64_t out_len, uint64_t in_consumed)
{
    switch (c.kind) {
    case kWhole:
        if (status < 0) return status;
        return out_len == c.decode_len ? (int32_t)XLZ_OK : (int32_t)XLZ_ERR_RESULT;
    case kCapCut:
        if (status == XLZ_ERR_OUT_CAP) return out_len == c.decode_len ? (int32_t)XLZ_OK : (int32_t)XLZ_ERR_RESULT;
        return status < 0 ? status : (int32_t)XLZ_ERR_RESULT;
    default:
        if (status == XLZ_ERR_UNEXPECTED_EOF)
            return out_len == c.decode_len && in_consumed == c.in_len ? (int32_t)XLZ_OK : (int32_t)XLZ_ERR_RESULT;
        return status < 0 ? status : (int32_t)XLZ_ERR_RESULT;
    }
}
// the status a stream of that kind must end in, as DeviceDest::want_status takes it (XLZ_OK: any status >= 0)
inline int32_t expected_status(uint8_t kind) { return kind == kWhole ? (int32_t)XLZ_OK : kind == kCapCut ? (int32_t)XLZ_ERR_OUT_CAP : (int32_t)XLZ_ERR_UNEXPECTED_EOF; }

// ---------------------------------------------------------------- windows ----
// false: an entry index outside the table; the window [dst_off, dst_off + dst_cap) of an entry with bytes does not fit
// in out_cap (no sum is formed unless it fits); two such windows share a byte.  The window of an entry without bytes, and
// one with dst_cap == 0, declares no byte, wherever its dst_off points.
inline bool wants_ok(const xlz_7z_entry *e, size_t ne, const xlz_7z_want *w, size_t n, uint64_t out_cap)
{
    std::vector<xlzwin::Window> win;
    for (size_t i = 0; i < n; i++) {
        if (w[i].entry >= ne) return false;
        if (has_bytes(e[w[i].entry]) && w[i].dst_cap) win.emplace_back(w[i].dst_off, w[i].dst_cap);
    }
    return xlzwin::disjoint_within(std::move(win), out_cap);
}

// Windows of the wanted entries' sizes back to back, in order: dst_off = the first multiple of align (>= 1) at or behind
// the end of the window before, *total = the end of the last one.  false: an offset or an end does not fit 64 bits.
inline bool layout(const xlz_7z_entry *e, xlz_7z_want *w, size_t n, uint64_t align, uint64_t *total)
{
    std::vector<uint64_t> size(n), off(n);
    for (size_t i = 0; i < n; i++) size[i] = e[w[i].entry].size;
    if (!xlzwin::back_to_back(size.data(), n, align, off.data(), total)) return false;
    for (size_t i = 0; i < n; i++) w[i].dst_off = off[i], w[i].dst_cap = size[i];
    return true;
}

// ---------------------------------------------------------------- the plan of an extraction ----
constexpr size_t kNoStream = ~(size_t)0;
struct FolderShape {
    uint32_t method;   // XLZ_7Z_*, as xlz_7z_index_bcj2 reports it
    bool steps;        // it is a filter chain
    bool usable;       // its steps can run (filter mode 1), or it has none
    uint64_t unpack_len, pack_len;
    const xlz_lzma2_unit *units;
    size_t n_units;
};
constexpr uint64_t kMaxDeviceFolder = 0xFFFF0000ull; // what a unit's 32-bit counters hold (xlz_xz_many.h: kMaxDeviceBlock)

struct Plan {
    std::vector<int32_t> pre;        // per want: XLZ_OK, or what settles it before the batch (XLZ_ERR_OUT_CAP, XLZ_ERR_UNSUPPORTED)
    std::vector<size_t> folders;     // the cover of the wants that are left, ascending
    std::vector<Cut> cuts;           // as folders
    std::vector<size_t> stream_of;   // per folder of the archive: its stream in the batch (the LZMA / LZMA2 folders of the cover, in order) or kNoStream
    std::vector<size_t> stream_folder; // per stream: its folder
    std::vector<xlz_pack_item> items;  // per want that is left, in a folder that is a stream: its bytes -> dst[i]
    std::vector<size_t> item_want;     // as items: the want
    std::vector<size_t> copy_wants;    // the wants that are left in Copy folders
};

// dst[i]: where want i's bytes go (the window's dst_off, or its place in the staging block)
inline void plan(const xlz_7z_entry *e, const FolderShape *fs, size_t nf, const xlz_7z_want *w, const uint64_t *dst, size_t n, Plan &p)
{
    p = Plan{};
    p.pre.assign(n, XLZ_OK);
    std::vector<uint8_t> left(n, 0);
    std::vector<uint64_t> wanted(n);
    for (size_t i = 0; i < n; i++) {
        const xlz_7z_entry &x = e[w[i].entry];
        wanted[i] = w[i].entry;
        if (!has_bytes(x)) continue;
        const FolderShape &f = fs[(size_t)x.folder];
        if (w[i].dst_cap < x.size)
            p.pre[i] = XLZ_ERR_OUT_CAP;
        else if ((f.method != XLZ_7Z_LZMA && f.method != XLZ_7Z_LZMA2 && f.method != XLZ_7Z_COPY) || !f.usable)
            p.pre[i] = XLZ_ERR_UNSUPPORTED;
        else if (f.method != XLZ_7Z_COPY && (f.unpack_len > kMaxDeviceFolder || f.pack_len > kMaxDeviceFolder))
            p.pre[i] = XLZ_ERR_UNSUPPORTED; // (a folder or packed stream of 4 GiB or more, whatever its cut: stricter than the cut needs)
        else
            left[i] = 1;
    }
    std::vector<uint64_t> P;
    reach(e, wanted.data(), left.data(), n, nf, P);
    p.stream_of.assign(nf, kNoStream);
    for (size_t k = 0; k < nf; k++) {
        if (!P[k]) continue;
        p.folders.push_back(k);
        p.cuts.push_back(cut_folder(fs[k].method, fs[k].steps, fs[k].unpack_len, fs[k].pack_len, fs[k].units, fs[k].n_units, P[k]));
        if (fs[k].method != XLZ_7Z_COPY) p.stream_of[k] = p.stream_folder.size(), p.stream_folder.push_back(k);
    }
    for (size_t i = 0; i < n; i++) {
        if (!left[i]) continue;
        const xlz_7z_entry &x = e[w[i].entry];
        if (fs[(size_t)x.folder].method == XLZ_7Z_COPY)
            p.copy_wants.push_back(i);
        else
            p.items.push_back(xlz_pack_item{p.stream_of[(size_t)x.folder], x.folder_off, x.size, dst[i]}), p.item_want.push_back(i);
    }
}

// ---------------------------------------------------------------- the verdict ----
enum : uint8_t { kDigestGood = 0, kDigestBad = 1, kDigestNone = 2 }; // (none: the entry carries no CRC, or verify is off)

// pre: Plan::pre; folder_st: stream_status of its folder's stream (XLZ_OK for a Copy folder); digest: of the entry's bytes.
// In this order: what settled it before the batch; an entry without bytes is good; the folder's stream; the entry's CRC.
inline xlz_7z_file_result verdict(int32_t pre, const xlz_7z_entry &x, int32_t folder_st, uint8_t digest, bool verify)
{
    if (pre < 0) return {pre, 0, 0};
    if (!has_bytes(x)) return {XLZ_OK, 0, 0};
    if (folder_st < 0) return {folder_st, 0, 0};
    if (verify && digest == kDigestBad) return {XLZ_ERR_RESULT, 0, 0};
    return {XLZ_OK, verify && !(x.flags & XLZ_7Z_ENTRY_HAS_CRC) ? 1u : 0u, x.size};
}

} // namespace xlz7zf

// What xlz_7z_open makes (xlz_7z.hip) and the extraction reads (xlz_7z_extract.hip); never changed after open.
struct xlz_7z_archive {
    const uint8_t *file = nullptr; // borrowed: the caller keeps it alive
    size_t len = 0;
    std::vector<xlz_7z_folder> folders;    // as xlz_7z_index_bcj2 lists them
    std::vector<xlz_7z_substream> subs;
    std::vector<xlz_filter_step> steps;    // of the chains, ascending by stream (= folder)
    std::vector<xlz_7z_entry> entries;
    std::vector<char> names;               // the pool xlz_7z_entry::name_off points into
    uint64_t total_size = 0;               // the sum of the entries' sizes
};
