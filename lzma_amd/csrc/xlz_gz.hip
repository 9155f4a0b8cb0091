// xlz_gz.hip -- gzip files, BGZF files and zlib streams as ONE batch (xlz_gz_probe / xlz_gz_decode_host /
// xlz_gz_decode_many / xlz_gz_decode_many_device).
//
// Host-only code (no kernels here).  xlz_gz.h decides everything that needs no device -- the headers, whether a file is
// BGZF, where the next member begins, the ranges to check, the verdicts --; this file turns the files into ROUNDS of
// xlz_inflate_batch (one gathered upload and one launch sequence each, host threads for long items and in deflate mode
// 2), then has the CRC32 of every gzip member formed by the check kernels over the destination (the tolerant
// device-destination stage, xlz_internal_decode_device, with ranges alone) and the Adler-32 of every zlib stream by
// xlz_adler_dev.hip, and folds the digests into one result per file.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/xlz.h"
#include "xlz_check_host.h"
#include "xlz_gz.h"
#include "xlz_windows.h"

using namespace xlzgz;

static_assert(sizeof(xlz_gz_info) == 40 && sizeof(xlz_gz_file) == 40 && sizeof(xlz_gz_result) == 24 && sizeof(xlz_gz_stats) == 80 &&
                  sizeof(xlz_adler_range) == 16,
              "include/xlz.h: the structs hold no implicit padding");

static bool format_ok(uint32_t f) { return f == XLZ_GZ_AUTO || f == XLZ_GZ_GZIP || f == XLZ_GZ_ZLIB; }

extern "C" int xlz_gz_probe(const uint8_t *in, size_t in_len, uint32_t format, xlz_gz_info *out)
{
    if (!out || (!in && in_len) || !format_ok(format)) return XLZ_ERR_BAD_ARG;
    return probe(in, in_len, format, out);
}

extern "C" int xlz_gz_decode_host(const uint8_t *in, size_t in_len, uint32_t format, uint8_t *out, size_t out_cap, int verify, xlz_gz_result *r)
{
    if (!r) return XLZ_ERR_BAD_ARG;
    *r = xlz_gz_result{};
    if ((!in && in_len) || (!out && out_cap) || !format_ok(format)) return XLZ_ERR_BAD_ARG;
    return decode_host(in, in_len, format, out, out_cap, verify != 0, r);
}

// dst: the host form (d_dst == NULL) -- every window lies in a staging block of the context's pool, back to back in the
// order of the files, and comes down from there in one copy
static int gz_decode_many(xlz_ctx *ctx, const xlz_gz_file *files, size_t n, uint8_t *dst, void *d_dst, bool device, size_t dst_cap, int verify,
                          xlz_gz_result *results)
{
    // ---- the arguments: all of them before the context is used, but the last
    if (!ctx) return XLZ_ERR_BAD_ARG;
    if (!n) return XLZ_OK;
    if (!files || !results || (dst_cap && !(device ? d_dst != nullptr : dst != nullptr))) return XLZ_ERR_BAD_ARG;
    std::vector<xlzwin::Window> win;
    for (size_t i = 0; i < n; i++) {
        if ((!files[i].in && files[i].in_len) || !format_ok(files[i].format)) return XLZ_ERR_BAD_ARG;
        win.emplace_back(files[i].dst_off, files[i].dst_cap);
    }
    if (!xlzwin::disjoint_within(std::move(win), dst_cap)) return XLZ_ERR_BAD_ARG;
    if (device && dst_cap) {
        const int ok = xlz_internal_device_dst_ok(ctx, d_dst, dst_cap);
        if (ok != XLZ_OK) return ok;
    }
    // ---- the windows: the caller's, or the staging block's
    HostStaging staging(ctx);
    std::vector<uint64_t> base(n);
    for (size_t i = 0; i < n; i++) base[i] = device ? files[i].dst_off : staging.add(files[i].dst_cap);
    int st = staging.acquire();
    void *d = device ? d_dst : staging.d_dst();
    const size_t cap = device ? dst_cap : staging.cap();
    // ---- the rounds
    xlz_gz_stats gs = {};
    gs.files = n;
    std::vector<File> f(n);
    struct Owner {
        size_t file, block; // block: of a BGZF file, else unused
    };
    std::vector<xlz_inflate_item> items;
    std::vector<Owner> owner;
    std::vector<Item> tmp;
    for (size_t i = 0; i < n && st == XLZ_OK; i++) {
        tmp.clear();
        open(f[i], files[i].in, files[i].in_len, files[i].format, files[i].dst_cap, verify != 0, tmp);
        gs.bgzf_files += f[i].bgzf;
        for (size_t k = 0; k < tmp.size(); k++) {
            items.push_back(xlz_inflate_item{files[i].in + tmp[k].in_off, tmp[k].in_len, base[i] + tmp[k].dst_off, tmp[k].dst_cap});
            owner.push_back(Owner{i, k});
        }
    }
    std::vector<xlz_inflate_result> ir;
    while (st == XLZ_OK) {
        for (size_t i = 0; i < n; i++) {
            Item it;
            if (f[i].bgzf || !next_item(f[i], it)) continue;
            items.push_back(xlz_inflate_item{files[i].in + it.in_off, it.in_len, base[i] + it.dst_off, it.dst_cap});
            owner.push_back(Owner{i, 0});
        }
        if (items.empty()) break;
        ir.assign(items.size(), xlz_inflate_result{});
        if (!cap) { // every room is empty and there is no destination: nothing can be written, the serial decoder says what happens
            for (size_t q = 0; q < items.size(); q++) {
                size_t produced = 0, consumed = 0;
                ir[q].status = xlzinf::host_inflate(items[q].in, (size_t)items[q].in_len, nullptr, 0, &produced, &consumed);
                ir[q].produced = produced, ir[q].in_consumed = consumed;
            }
            gs.host_items += items.size();
        } else {
            st = xlz_inflate_batch(ctx, items.data(), items.size(), d, cap, ir.data());
            if (st != XLZ_OK) break;
            xlz_inflate_stats is = {};
            if (xlz_ctx_last_inflate_stats(ctx, &is) == XLZ_OK)
                gs.device_items += is.device_items, gs.host_items += is.host_items, gs.uploads += is.uploads;
        }
        for (size_t q = 0; q < items.size(); q++) {
            File &x = f[owner[q].file];
            if (x.bgzf)
                block_done(x, owner[q].block, ir[q].status, ir[q].produced, ir[q].in_consumed);
            else
                item_done(x, ir[q].status, ir[q].produced, ir[q].in_consumed);
        }
        // (a round of BGZF blocks alone is a round too: `rounds` counts the inflate runs, which for a call with an
        //  ordinary file in it is the largest member count of one)
        gs.rounds++;
        items.clear(), owner.clear();
    }
    // ---- the checks: CRC32 of the gzip members by the check kernels, Adler-32 of the zlib streams by the Adler kernels
    std::vector<std::vector<uint32_t>> got(n);
    std::vector<xlz_check_range> cr;
    std::vector<xlz_adler_range> ar;
    struct Slot {
        size_t file, k;
    };
    std::vector<Slot> cr_slot, ar_slot;
    for (size_t i = 0; i < n && st == XLZ_OK; i++) {
        got[i].assign(f[i].checks.size(), 0);
        for (size_t k = 0; k < f[i].checks.size(); k++) {
            const Check &c = f[i].checks[k];
            const bool adler = f[i].format == XLZ_GZ_ZLIB;
            (adler ? gs.adler_ranges : gs.crc_ranges)++;
            if (!c.len) { // (of no byte: 1 and 0)
                got[i][k] = adler ? 1 : 0;
            } else if (adler) {
                ar.push_back(xlz_adler_range{base[i] + c.off, c.len}), ar_slot.push_back(Slot{i, k});
            } else {
                cr.push_back(xlz_check_range{xlzpost::kDestStream, base[i] + c.off, c.len, XLZ_CHECK_CRC32, 0}), cr_slot.push_back(Slot{i, k});
            }
        }
    }
    if (st == XLZ_OK && !cr.empty()) {
        std::vector<uint64_t> dig(cr.size(), 0);
        xlz_internal_check_stats_reset(ctx);
        const PostWork w = {nullptr, 0, cr.data(), cr.size(), dig.data(), nullptr, true};
        DeviceDest dest;
        dest.d_dst = d, dest.cap = cap, dest.have_items = true, dest.tolerant = true, dest.gather_copies = true;
        st = xlz_internal_decode_device(ctx, nullptr, 0, nullptr, w, dest);
        for (size_t q = 0; q < cr.size() && st == XLZ_OK; q++) got[cr_slot[q].file][cr_slot[q].k] = (uint32_t)dig[q];
    }
    if (st == XLZ_OK && !ar.empty()) {
        std::vector<uint32_t> dig(ar.size(), 0);
        st = xlz_internal_adler_run(ctx, d, cap, ar.data(), ar.size(), dig.data(), &gs.adler_kernel_ms);
        for (size_t q = 0; q < ar.size() && st == XLZ_OK; q++) got[ar_slot[q].file][ar_slot[q].k] = dig[q];
    }
    // ---- the verdicts, and in the host form ONE copy of the staging block, the good files scattered
    std::vector<xlz_gz_result> v(n);
    for (size_t i = 0; i < n && st == XLZ_OK; i++) v[i] = verdict(f[i], got[i].data());
    if (st == XLZ_OK && staging.d_dst()) {
        std::vector<HostStaging::Piece> good;
        for (size_t i = 0; i < n; i++)
            if (v[i].status == XLZ_OK && v[i].out_len) good.push_back({base[i], files[i].dst_off, v[i].out_len});
        st = staging.download(dst, good);
    }
    for (size_t i = 0; i < n; i++) {
        results[i] = st == XLZ_OK ? v[i] : xlz_gz_result{st, 0, 0, 0};
        gs.failed_files += results[i].status != XLZ_OK, gs.members += results[i].members;
    }
    xlz_internal_gz_stats_set(ctx, gs);
    return st;
}

extern "C" int xlz_gz_decode_many_device(xlz_ctx *ctx, const xlz_gz_file *files, size_t n, void *d_dst, size_t dst_cap, int verify,
                                         xlz_gz_result *results)
{
    return gz_decode_many(ctx, files, n, nullptr, d_dst, true, dst_cap, verify, results);
}

extern "C" int xlz_gz_decode_many(xlz_ctx *ctx, const xlz_gz_file *files, size_t n, uint8_t *dst, size_t dst_cap, int verify, xlz_gz_result *results)
{
    return gz_decode_many(ctx, files, n, dst, nullptr, false, dst_cap, verify, results);
}
