// xlz_bcj2_dev.hip -- merges the four streams of a .7z BCJ2 folder (main, call, jump, range coder) into one caller-owned
// device buffer: the decoded x86 code, where the folder belongs in the file, without a trip through the host.  The scheme
// is xlz_bcj2_dev.h (it also runs on the CPU: tests/c/bcj2_dev_selftest.cpp); this file holds the kernel and its launch.
// The reference has nothing of the kind.
//
// xlz_bcj2_merge_kernel: one workgroup of ONE wave per item, items walked grid-stride.  Per window of 1024 main bytes:
// sixty-four aligned 16-byte loads, the candidates marked by all lanes, the decisions -- the only serial part -- by lane 0
// over LDS, then the window's output image stored with aligned 16-byte stores.  About 7 KiB of LDS, no scratch, no
// atomics, no inline assembly.
#include <hip/hip_runtime.h>

#include "xlz_bcj2_dev.h"

using namespace xlzbcj2;

namespace xlz {

__global__ __launch_bounds__(64) void xlz_bcj2_merge_kernel(const DevItem *__restrict__ items, uint32_t n_items, uint8_t *__restrict__ dst,
                                                            DevResult *__restrict__ results)
{
    __shared__ Wave w;
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = blockIdx.x; i < n_items; i += gridDim.x) {
        const DevItem it = items[i];
        wave_init(w, it, lane);
        __syncthreads();
        while (!w.done) {
            wave_load(w, it, lane);
            __syncthreads();
            wave_mark(w, it, lane);
            __syncthreads();
            if (lane == 0) wave_decide(w, it);
            __syncthreads();
            wave_place(w, lane);
            __syncthreads();
            wave_store(w, it, dst, lane);
            __syncthreads();
        }
        if (lane == 0) results[i] = wave_result(w, it);
        __syncthreads();
    }
}

// Queues the merge of `n_items` items (`items` and `results` on the device; the items' destination ranges disjoint and
// inside the allocation behind dst) on `stream`.  A latency-bound kernel of one-wave workgroups: as many of them as there
// are items, up to kBcj2WgPerCu per CU, the rest grid-stride.  -> 0, or -1.
constexpr uint32_t kBcj2WgPerCu = 16;
int bcj2_launch(const DevItem *items, uint32_t n_items, uint8_t *dst, DevResult *results, int num_cus, hipStream_t stream)
{
    if (!n_items) return 0;
    const uint32_t cap = (uint32_t)(num_cus > 0 ? num_cus : 1) * kBcj2WgPerCu;
    hipLaunchKernelGGL(xlz_bcj2_merge_kernel, dim3(n_items < cap ? n_items : cap), dim3(kLanes), 0, stream, items, n_items, dst, results);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace xlz
