// xlz_adler_dev.hip -- Adler-32 of ranges of a device buffer, computed where the bytes lie.  The arithmetic, the deferral
// bound and the geometry are xlz_adler_dev.h (it also runs on the CPU: tests/c/adler_dev_selftest.cpp); this file holds the
// two kernels and their launch.  The reference has no container code and no checks.
//
//  * xlz_adler_seg_kernel: one wave per segment (kSegBytes of a range), workgroups of four waves that walk the segments
//    of ALL ranges of the launch grid-stride.  Every lane reads aligned 16-byte lines of consecutive addresses across the
//    wave; nothing outside a range is read.  The lanes' sums are added by shuffles.  One 32-bit digest per segment.
//    No LDS, no atomics.
//  * xlz_adler_fold_kernel: one wave per range folds its segment digests by the combine rule and writes the range's digest.
#include <hip/hip_runtime.h>

#include "xlz_adler_dev.h"

using namespace xlzadl;

namespace xlz {

__device__ __forceinline__ uint32_t wave_sum(uint32_t x)
{
    for (int d = 32; d >= 1; d >>= 1) x += (uint32_t)__shfl_xor((int)x, d, 64);
    return x;
}

__global__ __launch_bounds__(256) void xlz_adler_seg_kernel(const uint8_t *__restrict__ buf, const DevRange *__restrict__ ranges, uint32_t n_ranges,
                                                            uint32_t total_segs, uint32_t *__restrict__ seg_vals)
{
    const uint32_t lane = threadIdx.x & 63, waves = blockDim.x >> 6;
    for (uint64_t g = (uint64_t)blockIdx.x * waves + (threadIdx.x >> 6); g < total_segs; g += (uint64_t)gridDim.x * waves) {
        uint32_t lo = 0, hi = n_ranges - 1; // the range whose segments include g (seg_first ascends, every range has segments)
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (ranges[mid].seg_first <= g) lo = mid;
            else hi = mid - 1;
        }
        const DevRange R = ranges[lo];
        const uint64_t s = g - R.seg_first;
        const SegGeom geo = seg_geom(R.off, R.len, s);
        const LanePart p = lane_finish(seg_lane(buf, geo, R.off, R.off + R.len, lane), lane);
        const uint32_t s_sum = wave_sum(p.s), b_sum = wave_sum(p.b); // (64 x 522 240 and 64 x 65 520: no reduction in between)
        if (lane == 0) seg_vals[g] = seg_finish(s_sum, b_sum, (uint32_t)(seg_end(R.off, R.len, s, R.n_segs) - seg_begin(R.off, s)), geo.pad);
    }
}

__global__ __launch_bounds__(64) void xlz_adler_fold_kernel(const DevRange *__restrict__ ranges, const uint32_t *__restrict__ seg_vals,
                                                            uint32_t *__restrict__ digests)
{
    const DevRange R = ranges[blockIdx.x];
    const FoldPart p = fold_thread(seg_vals + R.seg_first, R.n_segs, R.off, R.len, threadIdx.x);
    const uint32_t a = wave_sum(p.a), b = wave_sum(p.b); // (64 x 65 520 each)
    if (threadIdx.x == 0) digests[R.out_index] = range_finish(a, b);
}

// Queues the segment and the fold kernel for `n_ranges` ranges (none empty; seg_first counts from 0 in seg_vals, ascending)
// of `buf` (a multiple of 16) on `stream`.  -> 0, or -1.
uint32_t adler_grid(uint32_t total_segs, int num_cus);
int adler_launch(const uint8_t *buf, const DevRange *ranges, uint32_t n_ranges, uint32_t total_segs, uint32_t *seg_vals, uint32_t *digests,
                 int num_cus, hipStream_t stream)
{
    if (!n_ranges || !total_segs) return 0;
    hipLaunchKernelGGL(xlz_adler_seg_kernel, dim3(adler_grid(total_segs, num_cus)), dim3(256), 0, stream, buf, ranges, n_ranges, total_segs, seg_vals);
    hipLaunchKernelGGL(xlz_adler_fold_kernel, dim3(n_ranges), dim3(kFoldThreads), 0, stream, ranges, seg_vals, digests);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// workgroups of the segment kernel for a launch of total_segs segments: one wave per segment, at most 8 workgroups = 32
// waves per CU (the kernel holds no LDS and few registers, and HBM wants them all); the rest is walked grid-stride
uint32_t adler_grid(uint32_t total_segs, int num_cus)
{
    const uint32_t wg_for_all = (total_segs + 3) / 4;
    return wg_for_all < (uint32_t)num_cus * 8 ? wg_for_all : (uint32_t)num_cus * 8;
}

} // namespace xlz
