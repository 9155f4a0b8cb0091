// xlz_7z_extract.hip -- chosen files of a .7z archive as ONE batch (xlz_7z_cover / xlz_7z_extract_layout / xlz_7z_extract /
// xlz_7z_extract_device).
//
// Host-only code (no kernels here).  xlz_7z_open (xlz_7z.hip) made the table; xlz_7z_files.h decides everything that
// needs no device -- the cover and its cuts, the windows, the pack items, the verdicts --; this file gives the covering
// folders to the batch engine through the tolerant device-destination stage (xlz_internal_decode_device): filters, the
// CRC32 of every wanted entry as a range over its folder's stream, one pack into the windows.  A solid folder is decoded
// only as far as the last wanted file reaches.
// (It is a file of its own because tests/c/bcj2_index_fuzz.cpp compiles xlz_7z.hip into a program that stubs what that
// file called of the library when the program was written.)
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/xlz.h"
#include "xlz_7z_files.h"
#include "xlz_check.h"
#include "xlz_check_host.h"

namespace {

using namespace xlz7zf;

// The folders as the plan sees them.  touched[k] != 0: the unit table of folder k is wanted (an LZMA2 folder without
// filter steps; a payload that xlz_lzma2_units refuses has none and is decoded whole).
struct Shapes {
    std::vector<FolderShape> fs;
    std::vector<std::vector<xlz_lzma2_unit>> units;
};
void shapes(const xlz_7z_archive *a, const std::vector<uint8_t> &touched, bool filters_on, Shapes &sh)
{
    const size_t nf = a->folders.size();
    sh.fs.resize(nf), sh.units.assign(nf, {});
    for (size_t k = 0; k < nf; k++) {
        const xlz_7z_folder &f = a->folders[k];
        const auto it = std::lower_bound(a->steps.begin(), a->steps.end(), k, [](const xlz_filter_step &s, size_t v) { return s.stream < v; });
        const bool steps = it != a->steps.end() && it->stream == k;
        if (touched[k] && f.method == XLZ_7Z_LZMA2 && !steps) {
            size_t nu = 0;
            if (xlz_lzma2_units(a->file + f.pack_off, (size_t)f.pack_len, nullptr, 0, &nu) == XLZ_OK && nu) {
                sh.units[k].resize(nu);
                if (xlz_lzma2_units(a->file + f.pack_off, (size_t)f.pack_len, sh.units[k].data(), nu, &nu) != XLZ_OK) sh.units[k].clear();
            }
        }
        sh.fs[k] = FolderShape{f.method, steps, !steps || filters_on, f.unpack_len, f.pack_len, sh.units[k].data(), sh.units[k].size()};
    }
}

} // namespace

extern "C" int xlz_7z_cover(const xlz_7z_archive *a, const uint64_t *entries, size_t n, xlz_7z_cover_item *items, size_t max_items, size_t *n_items)
{
    if (!a || (!entries && n) || !n_items || (!items && max_items)) return XLZ_ERR_BAD_ARG;
    *n_items = 0;
    for (size_t i = 0; i < n; i++)
        if (entries[i] >= a->entries.size()) return XLZ_ERR_BAD_ARG;
    const size_t nf = a->folders.size();
    std::vector<uint64_t> P;
    reach(a->entries.data(), entries, nullptr, n, nf, P);
    std::vector<uint8_t> touched(nf);
    for (size_t k = 0; k < nf; k++) touched[k] = P[k] != 0;
    Shapes sh;
    shapes(a, touched, true, sh);
    size_t m = 0;
    for (size_t k = 0; k < nf; k++) {
        if (!P[k]) continue;
        const FolderShape &f = sh.fs[k];
        const Cut c = cut_folder(f.method, f.steps, f.unpack_len, f.pack_len, f.units, f.n_units, P[k]);
        if (m < max_items) items[m] = xlz_7z_cover_item{k, c.decode_len, c.in_len};
        m++;
    }
    *n_items = m;
    return max_items && m > max_items ? XLZ_ERR_OUT_CAP : XLZ_OK;
}

extern "C" int xlz_7z_extract_layout(const xlz_7z_archive *a, xlz_7z_want *wants, size_t n, uint64_t align, uint64_t *total)
{
    if (!a || !total || !align || (!wants && n)) return XLZ_ERR_BAD_ARG;
    *total = 0;
    for (size_t i = 0; i < n; i++)
        if (wants[i].entry >= a->entries.size()) return XLZ_ERR_BAD_ARG;
    if (!layout(a->entries.data(), wants, n, align, total)) {
        *total = 0;
        return XLZ_ERR_OUT_CAP;
    }
    return XLZ_OK;
}

// out: the host form (d_out == NULL) -- the pack goes to a staging block of the context's pool, where the wanted sizes lie
// back to back in the order of the wants, and comes down from there in one copy
static int sz_extract(xlz_ctx *ctx, const xlz_7z_archive *a, const xlz_7z_want *wants, size_t n, uint8_t *out, void *d_out, bool device,
                      size_t out_cap, int verify, xlz_7z_file_result *results)
{
    // ---- the arguments: all of them before the context is used, but the last
    if (!n) return XLZ_OK;
    if (!a || !wants || !results || (out_cap && !(device ? d_out != nullptr : out != nullptr))) return XLZ_ERR_BAD_ARG;
    const xlz_7z_entry *e = a->entries.data();
    if (!wants_ok(e, a->entries.size(), wants, n, out_cap)) return XLZ_ERR_BAD_ARG;
    if (!ctx) return XLZ_ERR_BAD_ARG;
    if (device && out_cap) {
        const int ok = xlz_internal_device_dst_ok(ctx, d_out, out_cap);
        if (ok != XLZ_OK) return ok;
    }
    // ---- the plan: what settles an entry before the batch, the cover and its cuts, the pack items
    const size_t nf = a->folders.size();
    std::vector<uint8_t> touched(nf, 0);
    std::vector<uint64_t> dst(n, 0);
    HostStaging staging(ctx); // host form: the wanted sizes back to back
    for (size_t i = 0; i < n; i++) {
        const xlz_7z_entry &x = e[wants[i].entry];
        if (!has_bytes(x)) continue;
        touched[(size_t)x.folder] = 1;
        dst[i] = wants[i].dst_off;
        if (!device && wants[i].dst_cap >= x.size) dst[i] = staging.add(x.size);
    }
    Shapes sh;
    shapes(a, touched, xlz_ctx_filter_mode(ctx) == 1, sh);
    Plan p;
    plan(e, sh.fs.data(), nf, wants, dst.data(), n, p);
    const size_t ns = p.stream_folder.size();
    xlz_7z_extract_stats xs = {};
    xs.entries = n;
    for (size_t i = 0; i < n; i++) xs.empty_entries += !has_bytes(e[wants[i].entry]);
    for (size_t q = 0; q < p.folders.size(); q++) {
        const xlz_7z_folder &f = a->folders[p.folders[q]];
        xs.folders++, xs.comp_bytes += p.cuts[q].in_len, xs.decoded_bytes += p.cuts[q].decode_len, xs.folder_bytes += f.unpack_len;
    }
    // (from here on the call has run: its statistics are published at its end, whatever the device then says)
    xlz_internal_check_stats_reset(ctx), xlz_internal_filter_stats_reset(ctx), xlz_internal_pack_stats_reset(ctx);
    // ---- the batch: stream k = folder p.stream_folder[k], as far as its cut says; steps; the wanted entries' CRC ranges
    std::vector<xlz_stream_desc> d(ns);
    std::vector<xlz_result> r(ns);
    std::vector<Cut> cut(ns);
    std::vector<uint64_t> want_out(ns), want_in(ns);
    std::vector<int32_t> want_status(ns);
    std::vector<xlz_filter_step> fs;
    for (size_t q = 0, k = 0; q < p.folders.size(); q++) {
        const size_t fi = p.folders[q];
        const xlz_7z_folder &f = a->folders[fi];
        if (f.method == XLZ_7Z_COPY) continue;
        cut[k] = p.cuts[q];
        memset(&d[k], 0, sizeof d[k]);
        d[k].in = a->file + f.pack_off, d[k].in_len = (size_t)cut[k].in_len, d[k].out_cap = (size_t)cut[k].decode_len;
        d[k].dict_size = f.dict_size; // (the batch engine applies DecodeDictSize's 4096 floor)
        if (f.method == XLZ_7Z_LZMA)
            d[k].format = XLZ_FMT_LZMA_RAW, d[k].props = f.props, d[k].unpack_size = f.unpack_len;
        else
            d[k].format = XLZ_FMT_LZMA2_RAW;
        want_out[k] = cut[k].decode_len, want_in[k] = cut[k].kind == kUnitCut ? cut[k].in_len : DeviceDest::kAnyInput;
        want_status[k] = expected_status(cut[k].kind);
        auto it = std::lower_bound(a->steps.begin(), a->steps.end(), fi, [](const xlz_filter_step &s, size_t v) { return s.stream < v; });
        for (; it != a->steps.end() && it->stream == fi; ++it) fs.push_back(*it), fs.back().stream = k;
        k++;
    }
    std::vector<xlz_check_range> cr;
    std::vector<size_t> range_of(p.items.size(), kNoStream); // per pack item: its range
    for (size_t j = 0; j < p.items.size() && verify; j++) {
        if (!(e[wants[p.item_want[j]].entry].flags & XLZ_7Z_ENTRY_HAS_CRC)) continue;
        xlz_check_range c;
        memset(&c, 0, sizeof c);
        c.stream = p.items[j].stream, c.off = p.items[j].off, c.len = p.items[j].len, c.kind = XLZ_CHECK_CRC32;
        range_of[j] = cr.size(), cr.push_back(c);
    }
    std::vector<uint64_t> got(cr.size(), 0);
    std::vector<DeviceCopy> copies;
    std::vector<int32_t> copy_st(p.copy_wants.size(), XLZ_OK);
    for (size_t j = 0; j < p.copy_wants.size(); j++) {
        const xlz_7z_entry &x = e[wants[p.copy_wants[j]].entry];
        const xlz_7z_folder &f = a->folders[(size_t)x.folder];
        if (f.pack_len != f.unpack_len)
            copy_st[j] = XLZ_ERR_RESULT; // (a Copy folder is as long as its packed stream)
        else
            copies.push_back(DeviceCopy{dst[p.copy_wants[j]], a->file + f.pack_off + x.folder_off, x.size});
    }
    int st = staging.acquire();
    if (st == XLZ_OK && (ns || !copies.empty())) {
        const PostWork w = {fs.data(), fs.size(), cr.data(), cr.size(), got.data(), nullptr, true};
        DeviceDest dest;
        dest.d_dst = device ? d_out : staging.d_dst(), dest.cap = device ? out_cap : staging.cap();
        dest.want_out = want_out.data(), dest.want_in = want_in.data(), dest.want_status = want_status.data();
        dest.items = p.items.data(), dest.n_items = p.items.size(), dest.have_items = true, dest.tolerant = true;
        dest.copies = copies.data(), dest.n_copies = copies.size();
        st = xlz_internal_decode_device(ctx, d.data(), ns, r.data(), w, dest);
    }
    // ---- the verdicts
    std::vector<int32_t> folder_st(ns, XLZ_OK);
    for (size_t k = 0; k < ns && st == XLZ_OK; k++) folder_st[k] = stream_status(cut[k], r[k].status, r[k].out_len, r[k].in_consumed);
    std::vector<int32_t> fst(n, XLZ_OK);
    std::vector<uint8_t> dig(n, kDigestNone);
    for (size_t j = 0; j < p.items.size() && st == XLZ_OK; j++) {
        const size_t i = p.item_want[j];
        fst[i] = folder_st[(size_t)p.items[j].stream];
        if (range_of[j] != kNoStream && fst[i] == XLZ_OK) dig[i] = (uint32_t)got[range_of[j]] == e[wants[i].entry].crc ? kDigestGood : kDigestBad;
    }
    uint64_t host_ranges = 0, host_bytes = 0;
    for (size_t j = 0; j < p.copy_wants.size() && st == XLZ_OK; j++) { // (Copy folders never were on the device: the host's CRC, over the file)
        const size_t i = p.copy_wants[j];
        const xlz_7z_entry &x = e[wants[i].entry];
        fst[i] = copy_st[j];
        if (!verify || fst[i] != XLZ_OK || !(x.flags & XLZ_7Z_ENTRY_HAS_CRC)) continue;
        const xlz_7z_folder &f = a->folders[(size_t)x.folder];
        dig[i] = xlzcheck::crc32(a->file + f.pack_off + x.folder_off, (size_t)x.size) == x.crc ? kDigestGood : kDigestBad;
        host_ranges++, host_bytes += x.size;
    }
    if (host_ranges) xlz_internal_check_stats_host(ctx, host_ranges, host_bytes);
    std::vector<xlz_7z_file_result> v(n);
    for (size_t i = 0; i < n && st == XLZ_OK; i++) v[i] = verdict(p.pre[i], e[wants[i].entry], fst[i], dig[i], verify != 0);
    st = xlz_internal_extract_finish(staging, st, wants, dst.data(), v, out, results, xs); // (ONE copy of the staging block, the good entries scattered)
    xlz_internal_7z_extract_stats_set(ctx, xs);
    return st;
}

extern "C" int xlz_7z_extract(xlz_ctx *ctx, const xlz_7z_archive *a, const xlz_7z_want *wants, size_t n, uint8_t *out, size_t out_cap, int verify,
                              xlz_7z_file_result *results)
{
    return sz_extract(ctx, a, wants, n, out, nullptr, false, out_cap, verify, results);
}

extern "C" int xlz_7z_extract_device(xlz_ctx *ctx, const xlz_7z_archive *a, const xlz_7z_want *wants, size_t n, void *d_out, size_t out_cap,
                                     int verify, xlz_7z_file_result *results)
{
    return sz_extract(ctx, a, wants, n, nullptr, d_out, true, out_cap, verify, results);
}
