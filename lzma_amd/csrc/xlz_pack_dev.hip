// xlz_pack_dev.hip -- packs ranges of a batch's output arena into one caller-owned device buffer: the decoded file,
// contiguous in HBM, without a trip through the host.  The scheme is xlz_pack_dev.h (it also runs on the CPU:
// tests/c/pack_dev_selftest.cpp); this file holds the kernel and its launch.  The reference has nothing of the kind.
//
// xlz_pack_kernel: a workgroup of 256 lanes per 16 KiB tile of the DESTINATION, tiles walked grid-stride; a tile's lanes
// store consecutive aligned 16 bytes, built from one aligned 16-byte load (source and destination congruent modulo 16)
// or from two and a byte shift.  No LDS, no barrier, no atomics: the launch never waits for anything, and it runs alone
// on the batch's stream behind the decode.
#include <hip/hip_runtime.h>

#include "xlz_pack_dev.h"

using namespace xlzpack;

namespace xlz {

__global__ __launch_bounds__(256) void xlz_pack_kernel(const uint8_t *__restrict__ arena, uint64_t arena_bytes, uint8_t *__restrict__ dst,
                                                       const DevItem *__restrict__ items, uint32_t n_items, uint64_t tile0, uint64_t n_tiles)
{
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) tile_lane(arena, arena_bytes, dst, items, n_items, tile0 + t, threadIdx.x);
}

// Queues the pack of `n_items` items (sorted by dst, disjoint, none empty; `items` on the device) on `stream`; tile0 and
// n_tiles: xlzpack::first_tile / tile_count of the table.  A memory-bound kernel: at most kPackWgPerCu workgroups per CU,
// the tiles grid-stride.  -> 0, or -1.
constexpr uint32_t kPackWgPerCu = 8;
int pack_launch(const uint8_t *arena, uint64_t arena_bytes, uint8_t *dst, const DevItem *items, uint32_t n_items, uint64_t tile0,
                uint64_t n_tiles, int num_cus, hipStream_t stream)
{
    if (!n_items || !n_tiles) return 0;
    const uint64_t cap = (uint64_t)(num_cus > 0 ? num_cus : 1) * kPackWgPerCu;
    const uint32_t grid = (uint32_t)(n_tiles < cap ? n_tiles : cap);
    hipLaunchKernelGGL(xlz_pack_kernel, dim3(grid), dim3(kThreads), 0, stream, arena, arena_bytes, dst, items, n_items, tile0, n_tiles);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace xlz
