// xlz_sha256_dev.hip -- SHA-256 of ranges of a batch's output arena, computed where the decode left the bytes.  The
// lane's code is xlz_sha256_dev.h (it also runs on the CPU: tests/c/sha256_dev_selftest.cpp); this file holds the kernel
// and its launch.  The reference has no container code and no checks.
//
//  * xlz_check_sha256_kernel: one lane per range, 64 ranges per wave, one wave per workgroup (the waves of a launch spread
//    over all SIMDs).  The host sorts the ranges of a launch by length, longest first: the lanes of a wave finish together
//    and the longest waves start first.  No LDS, no scratch: the message window and the state live in registers.
#include <hip/hip_runtime.h>

#include "xlz_sha256_dev.h"

using namespace xlzsha;

namespace xlz {

__global__ __launch_bounds__(64) void xlz_check_sha256_kernel(const uint8_t *__restrict__ arena, uint64_t arena_bytes,
                                                              const DevRange *__restrict__ ranges, uint32_t n_ranges,
                                                              uint32_t *__restrict__ digests)
{
    const uint32_t i = blockIdx.x * kLanes + threadIdx.x;
    if (i >= n_ranges) return;
    const DevRange R = ranges[i];
    uint32_t h[8];
    lane_digest(arena, arena_bytes, R.off, R.len, h);
    uint4 *out = reinterpret_cast<uint4 *>(digests + 8 * (size_t)R.out_index);
    out[0] = make_uint4(digest_word(h[0]), digest_word(h[1]), digest_word(h[2]), digest_word(h[3]));
    out[1] = make_uint4(digest_word(h[4]), digest_word(h[5]), digest_word(h[6]), digest_word(h[7]));
}

// Queues the kernel for `n_ranges` ranges (every one inside [0, arena_bytes), sorted longest first) on `stream`; digests:
// 32 bytes per range, 16-byte aligned.  -> 0, or -1.
int sha256_launch(const uint8_t *arena, uint64_t arena_bytes, const DevRange *ranges, uint32_t n_ranges, uint32_t *digests,
                  hipStream_t stream)
{
    if (!n_ranges) return 0;
    hipLaunchKernelGGL(xlz_check_sha256_kernel, dim3((n_ranges + kLanes - 1) / kLanes), dim3(kLanes), 0, stream, arena, arena_bytes, ranges,
                       n_ranges, digests);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace xlz
