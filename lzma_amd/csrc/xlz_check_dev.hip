// xlz_check_dev.hip -- CRC32 / CRC64 of ranges of a batch's output arena, computed where the decode left the bytes.
// The arithmetic is xlz_check_dev.h (it also runs on the CPU: tests/c/check_dev_selftest.cpp); this file holds the two
// kernels per CRC and their launch.  The reference has no container code and no checks.
//
//  * xlz_check_crc32_kernel / xlz_check_crc64_kernel: one wave per segment (kSegBytes of a range), workgroups of four
//    waves that walk the segments of ALL ranges of the launch grid-stride.  The sixteen 256-entry tables of the row step
//    sit in LDS (16 KiB for CRC32, 32 KiB for CRC64), loaded once per workgroup.  Every lane reads aligned 16-byte chunks
//    of consecutive addresses across the wave; nothing outside a range is read.  One 64-bit value per segment.
//  * xlz_check_fold32_kernel / xlz_check_fold64_kernel: one workgroup of 256 threads per range folds its segment values
//    and writes the range's digest (the published CRC, zero-extended to 64 bits).
#include <hip/hip_runtime.h>

#include "xlz_check_dev.h"

using namespace xlzchk;

namespace xlz {

template <int W>
__device__ __forceinline__ void check_segments(const uint8_t *__restrict__ arena, const DevRange *__restrict__ ranges, uint32_t n_ranges,
                                               uint32_t total_segs, const typename Crc<W>::tab_t *__restrict__ g_tab,
                                               const Consts<W> *__restrict__ consts, uint64_t *__restrict__ seg_vals)
{
    __shared__ typename Crc<W>::tab_t T[kTabEntries];
    for (uint32_t i = threadIdx.x; i < kTabEntries; i += blockDim.x) T[i] = g_tab[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, waves = blockDim.x >> 6;
    for (uint64_t g = (uint64_t)blockIdx.x * waves + (threadIdx.x >> 6); g < total_segs; g += (uint64_t)gridDim.x * waves) {
        uint32_t lo = 0, hi = n_ranges - 1; // the range whose segments include g (seg_first ascends, every range has segments)
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (ranges[mid].seg_first <= g) lo = mid;
            else hi = mid - 1;
        }
        const DevRange R = ranges[lo];
        const SegGeom geo = seg_geom(R.off, R.len, g - R.seg_first);
        const uint64_t U = seg_lane<W>(arena, geo, R.off, R.off + R.len, lane, T);
        uint64_t x = lane_finish<W>(*consts, U, lane);
        for (int d = 32; d >= 1; d >>= 1) {
            const uint32_t xl = __shfl_xor((int)(uint32_t)x, d, 64), xh = __shfl_xor((int)(uint32_t)(x >> 32), d, 64);
            x ^= (uint64_t)xl | (uint64_t)xh << 32;
        }
        if (lane == 0) seg_vals[g] = seg_finish<W>(*consts, x, geo.pad);
    }
}

template <int W>
__device__ __forceinline__ void check_fold(const DevRange *__restrict__ ranges, const Consts<W> *__restrict__ consts,
                                           const uint64_t *__restrict__ seg_vals, uint64_t *__restrict__ digests)
{
    __shared__ uint64_t part[kFoldThreads];
    const DevRange R = ranges[blockIdx.x];
    const uint64_t *v = seg_vals + R.seg_first;
    const uint32_t t = threadIdx.x;
    part[t] = fold_thread<W>(*consts, v, R.n_segs, t);
    __syncthreads();
    for (uint32_t d = kFoldThreads / 2; d >= 1; d >>= 1) {
        if (t < d) part[t] ^= part[t + d];
        __syncthreads();
    }
    if (t == 0) digests[R.out_index] = range_finish<W>(*consts, part[0], v, R.n_segs, R.off, R.len);
}

__global__ __launch_bounds__(256) void xlz_check_crc32_kernel(const uint8_t *arena, const DevRange *ranges, uint32_t n_ranges, uint32_t total_segs,
                                                              const uint32_t *tab, const Consts<32> *consts, uint64_t *seg_vals)
{
    check_segments<32>(arena, ranges, n_ranges, total_segs, tab, consts, seg_vals);
}
__global__ __launch_bounds__(256) void xlz_check_crc64_kernel(const uint8_t *arena, const DevRange *ranges, uint32_t n_ranges, uint32_t total_segs,
                                                              const uint64_t *tab, const Consts<64> *consts, uint64_t *seg_vals)
{
    check_segments<64>(arena, ranges, n_ranges, total_segs, tab, consts, seg_vals);
}
__global__ __launch_bounds__(256) void xlz_check_fold32_kernel(const DevRange *ranges, const Consts<32> *consts, const uint64_t *seg_vals,
                                                               uint64_t *digests)
{
    check_fold<32>(ranges, consts, seg_vals, digests);
}
__global__ __launch_bounds__(256) void xlz_check_fold64_kernel(const DevRange *ranges, const Consts<64> *consts, const uint64_t *seg_vals,
                                                               uint64_t *digests)
{
    check_fold<64>(ranges, consts, seg_vals, digests);
}

// Queues the segment and the fold kernel for `n_ranges` ranges of one kind (width 32 or 64; seg_first counts from 0 in
// seg_vals) on `stream`.  tab / consts: device copies of build_tables / build_consts for that width.  -> 0, or -1.
int check_launch(int width, const uint8_t *arena, const DevRange *ranges, uint32_t n_ranges, uint32_t total_segs, const void *tab,
                 const void *consts, uint64_t *seg_vals, uint64_t *digests, int num_cus, hipStream_t stream)
{
    if (!n_ranges || !total_segs) return 0;
    const uint32_t wg_for_all = (total_segs + 3) / 4;
    // enough resident waves to keep HBM busy, few enough that a workgroup's table load is shared by many segments
    const uint32_t per_cu = width == 32 ? 8 : 4;
    const uint32_t grid = wg_for_all < (uint32_t)num_cus * per_cu ? wg_for_all : (uint32_t)num_cus * per_cu;
    if (width == 32) {
        hipLaunchKernelGGL(xlz_check_crc32_kernel, dim3(grid), dim3(256), 0, stream, arena, ranges, n_ranges, total_segs,
                           (const uint32_t *)tab, (const Consts<32> *)consts, seg_vals);
        hipLaunchKernelGGL(xlz_check_fold32_kernel, dim3(n_ranges), dim3(kFoldThreads), 0, stream, ranges, (const Consts<32> *)consts, seg_vals,
                           digests);
    } else {
        hipLaunchKernelGGL(xlz_check_crc64_kernel, dim3(grid), dim3(256), 0, stream, arena, ranges, n_ranges, total_segs,
                           (const uint64_t *)tab, (const Consts<64> *)consts, seg_vals);
        hipLaunchKernelGGL(xlz_check_fold64_kernel, dim3(n_ranges), dim3(kFoldThreads), 0, stream, ranges, (const Consts<64> *)consts, seg_vals,
                           digests);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// LDS of one workgroup of the segment kernel (what it means next to a running decode grid)
uint32_t check_lds_bytes(int width) { return kTabEntries * (width == 32 ? 4u : 8u); }

} // namespace xlz
