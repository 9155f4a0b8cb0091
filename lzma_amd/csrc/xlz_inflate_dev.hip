// xlz_inflate_dev.hip -- inflates raw-deflate streams (RFC 1951: the method-8 entries of a .zip archive) into one
// caller-owned device buffer, each where its item says, without a trip through the host.  The scheme is
// xlz_inflate_dev.h (it also runs on the CPU: tests/c/inflate_dev_selftest.cpp); this file holds the kernel and its launch.
// The reference has nothing of the kind.
//
// xlz_inflate_kernel: one workgroup of ONE wave per stream, the items -- sorted longest first by the host -- taken in turn
// by a grid that stays: workgroup g takes items g, g + grid, ...  Symbol decode is wave-uniform (scalar registers, the
// tables and the input window in LDS); the lanes carry the bytes.  About 5 KiB of LDS, no scratch, no atomics, no inline
// assembly.
#include <hip/hip_runtime.h>

#include "xlz_inflate_dev.h"

using namespace xlzinf;

namespace xlz {

__global__ __launch_bounds__(64) void xlz_inflate_kernel(const DevItem *__restrict__ items, uint32_t n_items, uint8_t *dst,
                                                         DevResult *__restrict__ results)
{
    __shared__ Wave w;
    for (uint32_t i = blockIdx.x; i < n_items; i += gridDim.x) {
        const DevItem it = items[i];
        const DevResult r = wave_inflate(w, it, dst);
        if (threadIdx.x == 0) results[i] = r;
        __syncthreads();
    }
}

// Queues the inflation of `n_items` items (`items` and `results` on the device; the items' destination ranges disjoint
// and inside the allocation behind dst) on `stream`.  A latency-bound kernel of one-wave workgroups: as many of them as
// there are items, up to kInflateWgPerCu per CU (5 KiB of LDS each: sixteen fit a CU's 160 KiB many times over, and
// sixteen waves are four per SIMD), the rest in turn.  -> 0, or -1.
constexpr uint32_t kInflateWgPerCu = 16;
int inflate_launch(const DevItem *items, uint32_t n_items, uint8_t *dst, DevResult *results, int num_cus, hipStream_t stream)
{
    if (!n_items) return 0;
    const uint32_t cap = (uint32_t)(num_cus > 0 ? num_cus : 1) * kInflateWgPerCu;
    hipLaunchKernelGGL(xlz_inflate_kernel, dim3(n_items < cap ? n_items : cap), dim3(kLanes), 0, stream, items, n_items, dst, results);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
uint32_t inflate_wg_per_cu() { return kInflateWgPerCu; }

} // namespace xlz
