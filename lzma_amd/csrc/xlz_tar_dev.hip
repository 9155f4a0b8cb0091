// xlz_tar_dev.hip -- the members of a .tar image that lies in device memory: the classify and gather kernels with their
// launches, and the entry points xlz_tar_parse_host / xlz_tar_scan_device / xlz_xz_tar_list (include/xlz.h; DESIGN.md
// section 3.18).  The lane scheme is xlz_tar_dev.h (it also runs on the CPU: tests/c/tar_dev_selftest.cpp), the walk along
// the header chain xlz_tar_walk.h (plain C++).  The reference has nothing of the kind.
//
// xlz_tar_classify_kernel: workgroups of 256 lanes, a wave per PAIR of 512-byte blocks, pairs walked grid-stride two at a
// time (both loads before either reduction); one aligned 16-byte load per lane and pair, five xor-shuffles, one ballot,
// one byte store by lane 9 of each half.  xlz_tar_gather_kernel: a thread per 16-byte chunk, grid-stride.  Neither uses
// LDS, scratch or atomics.  Resource usage of the gfx950 build (-Rpass-analysis=kernel-resource-usage): classify 36 VGPRs,
// gather 12 VGPRs, both at 8 waves per SIMD; no scratch, no LDS.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <new>
#include <vector>

#include "../../include/xlz.h"
#include "xlz_check_host.h"
#include "xlz_tar_dev.h"
#include "xlz_tar_walk.h"

using namespace xlztar;

namespace xlz {

// one pair of blocks, all 64 lanes of the wave: q as loaded (zeros where the image has no such block)
__device__ __forceinline__ void classify_pair(Quad q, uint64_t blk, uint64_t n_blocks, uint32_t lane, uint8_t *__restrict__ flags)
{
    const uint32_t sub = lane & (kBlockLanes - 1);
    const Part p = lane_part(q, sub);
    uint32_t packed = p.packed;
#pragma unroll
    for (int x = 1; x < (int)kBlockLanes; x <<= 1) packed += (uint32_t)__shfl_xor((int)packed, x);
    const unsigned long long seen = __ballot(p.any != 0);
    if (sub == kFieldLane && blk < n_blocks) flags[blk] = block_flag(packed, (uint32_t)(seen >> (lane & kBlockLanes)) != 0, q.w[1], q.w[2]);
}

__global__ __launch_bounds__(256) void xlz_tar_classify_kernel(const uint8_t *__restrict__ image, uint64_t len, uint8_t *__restrict__ flags)
{
    const uint64_t n_blocks = len >> 9, n_pairs = pair_count(len);
    const uint32_t lane = threadIdx.x & 63, half = lane >> 5, at = 16 * (lane & (kBlockLanes - 1));
    const uint64_t waves = (uint64_t)gridDim.x * (kThreads / 64), wave = (uint64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const Quad zero = {{0, 0, 0, 0}};
    for (uint64_t p = wave; p < n_pairs; p += 2 * waves) { // (the bound is the same for every lane of a wave)
        const uint64_t b0 = 2 * p + half, b1 = 2 * (p + waves) + half;
        Quad q0 = zero, q1 = zero;
        if (b0 < n_blocks) q0 = load16(image, len, b0 * kBlockBytes + at);
        if (b1 < n_blocks) q1 = load16(image, len, b1 * kBlockBytes + at);
        classify_pair(q0, b0, n_blocks, lane, flags);
        classify_pair(q1, b1, n_blocks, lane, flags);
    }
}

__global__ __launch_bounds__(256) void xlz_tar_gather_kernel(const uint8_t *__restrict__ image, uint64_t len, const uint64_t *__restrict__ idx,
                                                             uint64_t n, uint8_t *__restrict__ staging)
{
    const uint64_t chunks = n * kBlockLanes, step = (uint64_t)gridDim.x * kThreads;
    for (uint64_t c = (uint64_t)blockIdx.x * kThreads + threadIdx.x; c < chunks; c += step) gather_chunk(image, len, idx, staging, c);
}

// Memory-bound kernels: at most kTarWgPerCu workgroups per CU, the rest grid-stride.  -> 0, or -1.
constexpr uint32_t kTarWgPerCu = 8;
static uint32_t grid_for(uint64_t workgroups, int num_cus)
{
    const uint64_t cap = (uint64_t)(num_cus > 0 ? num_cus : 1) * kTarWgPerCu;
    return (uint32_t)(workgroups < cap ? workgroups : cap);
}
// Queues the classify of the len / 512 complete blocks of `image` (a multiple of 16) on `stream`: flags[len / 512].
int tar_classify_launch(const uint8_t *image, uint64_t len, uint8_t *flags, int num_cus, hipStream_t stream)
{
    const uint64_t n_pairs = pair_count(len);
    if (!n_pairs) return 0;
    if ((uintptr_t)image & 15) return -1;
    const uint64_t per_wg = 2 * (kThreads / 64); // pairs a workgroup takes per round
    hipLaunchKernelGGL(xlz_tar_classify_kernel, dim3(grid_for((n_pairs + per_wg - 1) / per_wg, num_cus)), dim3(kThreads), 0, stream, image, len, flags);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// Queues the gather of blocks idx[0 .. n) (device memory; every index < len / 512: the caller has checked) into staging.
int tar_gather_launch(const uint8_t *image, uint64_t len, const uint64_t *idx, uint64_t n, uint8_t *staging, int num_cus, hipStream_t stream)
{
    if (!n) return 0;
    if (((uintptr_t)image | (uintptr_t)staging) & 15) return -1;
    const uint64_t wgs = (n * kBlockLanes + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(xlz_tar_gather_kernel, dim3(grid_for(wgs, num_cus)), dim3(kThreads), 0, stream, image, len, idx, n, staging);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace xlz

struct xlz_tar {
    xlztar::Table t;
};

namespace {

// the Source of xlz_tar_scan_device: the flags of every block, the candidate blocks dense in rank order, and the data of
// the meta entries fetched so far
struct DeviceSource : Source {
    const std::vector<uint8_t> &flags;
    const std::vector<uint64_t> &cand; // ascending block indices with flag 1
    const std::vector<uint8_t> &blocks; // 512 bytes per candidate
    struct Meta {
        uint64_t n;
        std::vector<uint8_t> data;
    };
    std::map<uint64_t, Meta> metas;
    DeviceSource(const std::vector<uint8_t> &f, const std::vector<uint64_t> &c, const std::vector<uint8_t> &b) : flags(f), cand(c), blocks(b) {}
    int flag(uint64_t blk) override { return blk < flags.size() ? flags[(size_t)blk] : 0; }
    const uint8_t *header(uint64_t blk) override
    {
        const auto it = std::lower_bound(cand.begin(), cand.end(), blk);
        return it != cand.end() && *it == blk ? blocks.data() + (size_t)(it - cand.begin()) * 512 : nullptr;
    }
    const uint8_t *meta(uint64_t blk, uint64_t n) override
    {
        const auto it = metas.find(blk);
        return it != metas.end() && it->second.n == n ? it->second.data.data() : nullptr;
    }
};

int tar_scan(xlz_ctx *ctx, const void *d_image, uint64_t len, xlz_tar *t)
{
    xlz_tar_stats ts = {};
    ts.blocks = len >> 9;
    double ms = 0;
    std::vector<uint8_t> flags((size_t)ts.blocks);
    int st = xlz_internal_tar_classify_device(ctx, d_image, len, flags.data(), &ms);
    if (st != XLZ_OK) return st;
    if (ts.blocks) ts.kernel_ms += ms, ts.launches++, ts.downloaded_bytes += ts.blocks;
    std::vector<uint64_t> cand;
    for (size_t b = 0; b < flags.size(); b++) {
        if (flags[b] == 1) cand.push_back(b);
        else if (flags[b] == 2) ts.zero_blocks++;
    }
    ts.candidate_blocks = cand.size();
    std::vector<uint8_t> blocks(cand.size() * 512);
    st = xlz_internal_tar_gather_device(ctx, d_image, len, cand.data(), cand.size(), blocks.data(), &ms);
    if (st != XLZ_OK) return st;
    if (!cand.empty()) ts.kernel_ms += ms, ts.launches++, ts.downloaded_bytes += blocks.size();
    DeviceSource src(flags, cand, blocks);
    for (;;) {
        walk(src, len, t->t);
        if (t->t.wants.empty()) break;
        // the data of the meta entries this run met: one gather (the walk took care that they lie inside the image)
        std::vector<uint64_t> idx;
        for (const MetaWant &w : t->t.wants)
            for (uint64_t k = 0; k < w.n; k++) idx.push_back(w.blk + k);
        std::vector<uint8_t> data(idx.size() * 512);
        st = xlz_internal_tar_gather_device(ctx, d_image, len, idx.data(), idx.size(), data.data(), &ms);
        if (st != XLZ_OK) return st;
        ts.kernel_ms += ms, ts.launches++, ts.meta_bytes += data.size(), ts.downloaded_bytes += data.size();
        size_t at = 0;
        for (const MetaWant &w : t->t.wants) {
            DeviceSource::Meta &m = src.metas[w.blk];
            m.n = w.n, m.data.assign(data.begin() + at, data.begin() + at + (size_t)w.n * 512);
            at += (size_t)w.n * 512;
        }
    }
    ts.header_blocks = t->t.header_blocks;
    xlz_internal_tar_stats_set(ctx, ts);
    return XLZ_OK;
}

} // namespace

extern "C" int xlz_tar_parse_host(const void *image, uint64_t len, xlz_tar **out)
{
    if (!out) return XLZ_ERR_BAD_ARG;
    *out = nullptr;
    if (!image && len) return XLZ_ERR_BAD_ARG;
    xlz_tar *t = new (std::nothrow) xlz_tar;
    if (!t) return XLZ_ERR_DEVICE;
    HostSource src(static_cast<const uint8_t *>(image));
    walk(src, len, t->t);
    *out = t;
    return XLZ_OK;
}

extern "C" int xlz_tar_scan_device(xlz_ctx *ctx, const void *d_image, uint64_t len, xlz_tar **out)
{
    if (!out) return XLZ_ERR_BAD_ARG;
    *out = nullptr;
    if (!ctx || (!d_image && len) || ((uintptr_t)d_image & 15)) return XLZ_ERR_BAD_ARG;
    xlz_tar *t = new (std::nothrow) xlz_tar;
    if (!t) return XLZ_ERR_DEVICE;
    const int st = tar_scan(ctx, d_image, len, t);
    if (st != XLZ_OK) {
        delete t;
        return st;
    }
    *out = t;
    return XLZ_OK;
}

extern "C" int xlz_xz_tar_list(xlz_ctx *ctx, const xlz_xz_file *f, int verify, xlz_tar **out, size_t *unverified)
{
    if (!out) return XLZ_ERR_BAD_ARG;
    *out = nullptr;
    if (unverified) *unverified = 0;
    if (!ctx || !f) return XLZ_ERR_BAD_ARG;
    uint64_t size = 0;
    int st = xlz_xz_file_info(f, &size, nullptr, nullptr);
    if (st != XLZ_OK) return st;
    if ((uint64_t)(size_t)size != size) return XLZ_ERR_UNSUPPORTED;
    void *image = nullptr;
    if (size) {
        st = xlz_internal_device_block(ctx, (size_t)size, &image);
        if (st != XLZ_OK) return st;
        const xlz_xz_range all = {0, size, 0};
        uint64_t copied = 0;
        st = xlz_xz_read_device(ctx, f, &all, 1, image, (size_t)size, &copied, verify, unverified);
        if (st == XLZ_OK && copied != size) st = XLZ_ERR_RESULT;
    }
    if (st == XLZ_OK) st = xlz_tar_scan_device(ctx, image, size, out);
    xlz_internal_device_block_release(ctx, image);
    return st;
}

extern "C" void xlz_tar_info(const xlz_tar *t, size_t *n_entries, size_t *name_bytes, int *end_status, uint64_t *end_off)
{
    if (n_entries) *n_entries = t ? t->t.entries.size() : 0;
    if (name_bytes) *name_bytes = t ? t->t.names.size() : 0;
    if (end_status) *end_status = t ? t->t.end_status : XLZ_ERR_BAD_ARG;
    if (end_off) *end_off = t ? t->t.end_off : 0;
}

extern "C" int xlz_tar_entries(const xlz_tar *t, xlz_tar_entry *e, size_t cap, void *names, size_t names_cap)
{
    if (!t || (cap && !e) || (names_cap && !names)) return XLZ_ERR_BAD_ARG;
    const size_t n = std::min(cap, t->t.entries.size()), nb = std::min(names_cap, t->t.names.size());
    if (n) memcpy(e, t->t.entries.data(), n * sizeof(xlz_tar_entry));
    if (nb) memcpy(names, t->t.names.data(), nb);
    return n < t->t.entries.size() || nb < t->t.names.size() ? XLZ_ERR_OUT_CAP : XLZ_OK;
}

extern "C" void xlz_tar_close(xlz_tar *t) { delete t; }
