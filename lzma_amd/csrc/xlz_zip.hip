// xlz_zip.hip -- the entries of a .zip archive: the table, and chosen entries as ONE batch (xlz_zip_open /
// xlz_zip_extract_layout / xlz_zip_extract / xlz_zip_extract_device).
//
// Host-only code (no kernels here).  xlz_zip.h decides everything that needs no device -- the end record, the table, the
// classes, the windows, the streams, the stored spans, the pack items, the check ranges, the verdicts --; this file
// gives the wanted method-14 entries to the batch engine through the tolerant device-destination stage
// (xlz_internal_decode_device): one decode launch sequence, the CRC32 of every wanted entry on the device, one pack
// into the windows, and the stored entries gathered into one pinned block, uploaded once and scattered by the pack kernel
// (DeviceDest::gather_copies).  In deflate mode 1 / 2 the wanted deflate entries are inflated in the same call
// (DeviceDest::inflate: xlz_inflate_dev.hip, or host threads), in place, and checked where they lie.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/xlz.h"
#include "xlz_check_host.h"
#include "xlz_zip.h"

using namespace xlzzip;

// The context's deflate mode, as a WEAK reference: a program that is this file alone, without the library's contexts
// (tests/c/zip_fuzz.cpp), links without it and is in mode 0.
extern "C" int xlz_ctx_deflate_mode(const xlz_ctx *ctx) __attribute__((weak));

static_assert(sizeof(xlz_zip_entry) == 72, "include/xlz.h documents the entry's size");
static_assert(xlzzip::kDestStream == xlzpost::kDestStream, "xlz_zip.h names the destination as xlz_post.h does");

extern "C" int xlz_zip_open(const uint8_t *file, size_t len, xlz_zip_archive **a)
{
    if (!a) return XLZ_ERR_BAD_ARG;
    *a = nullptr;
    if (!file && len) return XLZ_ERR_BAD_ARG;
    xlz_zip_archive *z = new (std::nothrow) xlz_zip_archive;
    if (!z) return XLZ_ERR_DEVICE;
    z->file = file, z->len = len;
    const int st = parse(file, len, z->t);
    if (st != XLZ_OK) {
        delete z;
        return st;
    }
    *a = z;
    return XLZ_OK;
}

extern "C" void xlz_zip_close(xlz_zip_archive *a) { delete a; }

extern "C" int xlz_zip_archive_info(const xlz_zip_archive *a, size_t *n_entries, size_t *name_bytes, uint64_t *total_size, uint64_t *shift)
{
    if (!a) return XLZ_ERR_BAD_ARG;
    if (n_entries) *n_entries = a->t.entries.size();
    if (name_bytes) *name_bytes = a->t.names.size();
    if (total_size) *total_size = a->t.total_size;
    if (shift) *shift = a->t.end.shift;
    return XLZ_OK;
}

extern "C" int xlz_zip_archive_entries(const xlz_zip_archive *a, xlz_zip_entry *entries, size_t max_entries, char *names, size_t names_cap)
{
    if (!a || (!entries && max_entries) || (!names && names_cap)) return XLZ_ERR_BAD_ARG;
    const size_t ne = std::min(max_entries, a->t.entries.size()), nb = std::min(names_cap, a->t.names.size());
    if (ne) memcpy(entries, a->t.entries.data(), ne * sizeof *entries);
    if (nb) memcpy(names, a->t.names.data(), nb);
    return ne < a->t.entries.size() || nb < a->t.names.size() ? XLZ_ERR_OUT_CAP : XLZ_OK;
}

extern "C" int xlz_zip_extract_layout(const xlz_zip_archive *a, xlz_zip_want *wants, size_t n, uint64_t align, uint64_t *total)
{
    if (!a || !total || !align || (!wants && n)) return XLZ_ERR_BAD_ARG;
    *total = 0;
    for (size_t i = 0; i < n; i++)
        if (wants[i].entry >= a->t.entries.size()) return XLZ_ERR_BAD_ARG;
    if (!layout(a->t.entries.data(), wants, n, align, total)) {
        *total = 0;
        return XLZ_ERR_OUT_CAP;
    }
    return XLZ_OK;
}

// out: the host form (d_out == NULL) -- everything goes to a staging block of the context's pool, where the wanted sizes
// lie back to back in the order of the wants, and comes down from there in one copy
static int zip_extract(xlz_ctx *ctx, const xlz_zip_archive *a, const xlz_zip_want *wants, size_t n, uint8_t *out, void *d_out, bool device,
                       size_t out_cap, int verify, xlz_zip_file_result *results)
{
    // ---- the arguments: all of them before the context is used, but the last
    if (!n) return XLZ_OK;
    if (!a || !wants || !results || (out_cap && !(device ? d_out != nullptr : out != nullptr))) return XLZ_ERR_BAD_ARG;
    const xlz_zip_entry *e = a->t.entries.data();
    if (!wants_ok(e, a->t.entries.size(), wants, n, out_cap)) return XLZ_ERR_BAD_ARG;
    if (!ctx) return XLZ_ERR_BAD_ARG;
    if (device && out_cap) {
        const int ok = xlz_internal_device_dst_ok(ctx, d_out, out_cap);
        if (ok != XLZ_OK) return ok;
    }
    // ---- the plan: what settles an entry before the batch, the streams, the stored spans, the pack items
    std::vector<uint64_t> dst(n, 0);
    HostStaging staging(ctx); // host form: the wanted sizes back to back
    for (size_t i = 0; i < n; i++) {
        const xlz_zip_entry &x = e[wants[i].entry];
        if (!has_bytes(x)) continue;
        dst[i] = wants[i].dst_off;
        if (!device && wants[i].dst_cap >= x.size) dst[i] = staging.add(x.size);
    }
    Plan p;
    const int deflate_mode = xlz_ctx_deflate_mode ? xlz_ctx_deflate_mode(ctx) : 0;
    plan(a->file, e, wants, dst.data(), n, p, deflate_mode);
    const size_t ns = p.streams.size();
    xlz_zip_extract_stats xs = {};
    xs.entries = n, xs.lzma_entries = ns, xs.stored_entries = p.spans.size();
    for (size_t i = 0; i < n; i++) xs.empty_entries += !has_bytes(e[wants[i].entry]);
    for (size_t k = 0; k < ns; k++) xs.comp_bytes += e[wants[p.stream_want[k]].entry].comp_size;
    for (const Span &s : p.spans) xs.comp_bytes += s.len;
    for (const xlz_inflate_item &it : p.inflate) xs.comp_bytes += it.in_len;
    std::vector<xlz_inflate_result> ir(p.inflate.size());
    // (from here on the call has run: its statistics are published at its end, whatever the device then says)
    xlz_internal_check_stats_reset(ctx), xlz_internal_pack_stats_reset(ctx);
    std::vector<xlz_result> r(ns);
    std::vector<uint64_t> want_out(ns);
    for (size_t k = 0; k < ns; k++) want_out[k] = p.items[k].len;
    std::vector<xlz_check_range> cr;
    std::vector<size_t> range_of(n, kNone);
    if (verify) check_ranges(p, n, cr, range_of);
    std::vector<uint64_t> got(cr.size(), 0);
    std::vector<DeviceCopy> copies;
    for (const Span &s : p.spans) copies.push_back(DeviceCopy{s.dst, a->file + s.src_off, s.len});
    int st = staging.acquire();
    if (st == XLZ_OK && (ns || !copies.empty() || !p.inflate.empty())) {
        const PostWork w = {nullptr, 0, cr.data(), cr.size(), got.data(), nullptr, true};
        DeviceDest dest;
        dest.d_dst = device ? d_out : staging.d_dst(), dest.cap = device ? out_cap : staging.cap();
        dest.want_out = want_out.data();
        dest.items = p.items.data(), dest.n_items = p.items.size(), dest.have_items = true, dest.tolerant = true;
        dest.copies = copies.data(), dest.n_copies = copies.size(), dest.gather_copies = true, dest.copy_uploads = &xs.stored_uploads;
        dest.inflate = p.inflate.data(), dest.n_inflate = p.inflate.size(), dest.inflate_res = ir.data(), dest.inflate_mode = deflate_mode;
        st = xlz_internal_decode_device(ctx, p.streams.data(), ns, r.data(), w, dest);
    }
    // ---- the verdicts
    std::vector<int32_t> sst(n, XLZ_OK);
    std::vector<uint8_t> dig(n, kDigestNone);
    for (size_t k = 0; k < ns && st == XLZ_OK; k++) sst[p.stream_want[k]] = stream_status(e[wants[p.stream_want[k]].entry], r[k].status, r[k].out_len);
    for (size_t k = 0; k < p.inflate.size() && st == XLZ_OK; k++)
        sst[p.inflate_want[k]] = inflate_status(e[wants[p.inflate_want[k]].entry], ir[k].status, ir[k].produced);
    std::vector<xlz_zip_file_result> v(n);
    for (size_t i = 0; i < n && st == XLZ_OK; i++) {
        const xlz_zip_entry &x = e[wants[i].entry];
        if (range_of[i] != kNone && sst[i] == XLZ_OK) dig[i] = (uint32_t)got[range_of[i]] == x.crc ? kDigestGood : kDigestBad;
        v[i] = verdict(p.pre[i], x, sst[i], dig[i], verify != 0);
    }
    st = xlz_internal_extract_finish(staging, st, wants, dst.data(), v, out, results, xs); // (ONE copy of the staging block, the good entries scattered)
    xlz_internal_zip_extract_stats_set(ctx, xs);
    return st;
}

extern "C" int xlz_zip_extract(xlz_ctx *ctx, const xlz_zip_archive *a, const xlz_zip_want *wants, size_t n, uint8_t *out, size_t out_cap, int verify,
                               xlz_zip_file_result *results)
{
    return zip_extract(ctx, a, wants, n, out, nullptr, false, out_cap, verify, results);
}

extern "C" int xlz_zip_extract_device(xlz_ctx *ctx, const xlz_zip_archive *a, const xlz_zip_want *wants, size_t n, void *d_out, size_t out_cap,
                                      int verify, xlz_zip_file_result *results)
{
    return zip_extract(ctx, a, wants, n, nullptr, d_out, true, out_cap, verify, results);
}
