// xlz_filter_dev.hip -- the .xz / .7z filters in front of an LZMA coder (Delta, BCJ), applied in place to streams of a
// batch's output arena, where the decode left the bytes and before the checks and the download read them.  The schemes are
// xlz_filter_dev.h (they also run on the CPU: tests/c/filter_dev_selftest.cpp); this file holds the kernels and their
// launch.  The reference has no filters.
//
// One launch applies ONE step of many streams.  Every kernel finds the step of its tile by a binary search over the
// launch's table (DevStep::first ascends), like the check kernels find their range.
//  * xlz_filter_bcj_kernel (ARM, ARM-Thumb, PowerPC, SPARC, IA-64): a workgroup of 256 lanes takes kBcjTileBytes; a lane
//    loads, converts and stores aligned 16-byte chunks of consecutive addresses across the wave (streams start at
//    multiples of 256 in the arena).  Only a stream's last chunk is touched byte by byte.
//  * xlz_filter_x86_mark_kernel, xlz_filter_x86_walk_kernel: a lane per window of kX86Window bytes; the first notes every
//    window's first sync point from the original bytes, the second runs the serial decoder from sync point to sync point.
//    Two launches because a converted operand can make or unmake an E8.
//  * xlz_filter_delta_sums_kernel, xlz_filter_delta_scan_kernel + xlz_filter_delta_scan2_kernel,
//    xlz_filter_delta_apply_kernel: a workgroup per chunk of kDeltaChunk bytes held in LDS (16 KiB); column sums per chunk,
//    exclusive prefixes over a stream's chunks (a thread per residue; inside groups of kDeltaGroup chunks, then over the
//    groups), carried-in sums plus a scan by doubling.  Separate launches and no look-back: no workgroup ever waits for
//    another one, so the pass cannot stall next to a resident decode grid.
#include <hip/hip_runtime.h>

#include "xlz_filter_dev.h"

using namespace xlzflt;

namespace xlz {

__device__ __forceinline__ uint32_t find_step(const DevStep *__restrict__ steps, uint32_t n_steps, uint32_t tile)
{
    uint32_t lo = 0, hi = n_steps - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (steps[mid].first <= tile) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// n (< 16) bytes at p, byte by byte, into / out of four words
__device__ __forceinline__ void load_tail(const uint8_t *p, uint32_t n, uint32_t w[4])
{
    w[0] = w[1] = w[2] = w[3] = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++)
        if (k < n) w[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
}
__device__ __forceinline__ void store_tail(uint8_t *p, uint32_t lo, uint32_t n, const uint32_t w[4])
{
#pragma unroll
    for (uint32_t k = 0; k < 16; k++)
        if (k >= lo && k < n) p[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
}

__global__ __launch_bounds__(256) void xlz_filter_bcj_kernel(uint8_t *__restrict__ arena, const DevStep *__restrict__ steps, uint32_t n_steps)
{
    const DevStep S = steps[find_step(steps, n_steps, blockIdx.x)];
    uint8_t *buf = arena + S.off;
    const uint64_t tile0 = (uint64_t)(blockIdx.x - S.first) * kBcjTileBytes;
#pragma unroll
    for (uint32_t q = 0; q < kBcjTileBytes / (256 * kLaneBytes); q++) {
        const uint64_t pos = tile0 + ((uint64_t)q * 256 + threadIdx.x) * kLaneBytes;
        if (pos >= S.len) break;
        const uint64_t left = S.len - pos;
        const uint32_t whole = left < 16 ? (uint32_t)left : 16u;
        uint32_t w[4];
        if (whole == 16) {
            const uint4 v = *reinterpret_cast<const uint4 *>(buf + pos);
            w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
        } else {
            load_tail(buf + pos, whole, w);
        }
        uint32_t flags = 0, next_out = 0;
        if (S.id == kARMThumb) {
            // these two halfwords may be stored by a neighbouring lane or workgroup meanwhile: a formal data race that is relied
            // upon.  Where another lane stores one, only its top five bits are used here, and the conversion keeps those (next_h is
            // used in full only as this lane's own second half, which this lane alone stores): do not widen these loads
            const uint32_t prev_h = pos ? ((uint32_t)buf[pos - 2] | (uint32_t)buf[pos - 1] << 8) : 0u;
            const uint32_t next_h = left >= 18 ? ((uint32_t)buf[pos + 16] | (uint32_t)buf[pos + 17] << 8) : 0u;
            flags = thumb_chunk16(S.param + (uint32_t)pos, w, left >= 18 ? 18u : whole, prev_h, next_h, &next_out);
        } else {
            bcj_chunk16(S.id, S.param + (uint32_t)pos, w, whole);
        }
        if (whole == 16 && !(flags & 1)) {
            *reinterpret_cast<uint4 *>(buf + pos) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            store_tail(buf + pos, (flags & 1) ? 2u : 0u, whole, w);
        }
        if (flags & 2) buf[pos + 16] = (uint8_t)next_out, buf[pos + 17] = (uint8_t)(next_out >> 8);
    }
}

__global__ __launch_bounds__(256) void xlz_filter_x86_mark_kernel(const uint8_t *__restrict__ arena, const DevStep *__restrict__ steps, uint32_t n_steps,
                                                                  uint16_t *__restrict__ sync)
{
    const DevStep S = steps[find_step(steps, n_steps, blockIdx.x)];
    const uint64_t j = (uint64_t)(blockIdx.x - S.first) * kX86TileWindows + threadIdx.x;
    if (j >= x86_windows(S.len)) return;
    sync[S.aux + j] = x86_first_sync(arena + S.off, S.len, j);
}
__global__ __launch_bounds__(256) void xlz_filter_x86_walk_kernel(uint8_t *__restrict__ arena, const DevStep *__restrict__ steps, uint32_t n_steps,
                                                                  const uint16_t *__restrict__ sync)
{
    const DevStep S = steps[find_step(steps, n_steps, blockIdx.x)];
    const uint64_t j = (uint64_t)(blockIdx.x - S.first) * kX86TileWindows + threadIdx.x, n_win = x86_windows(S.len);
    if (j >= n_win) return;
    x86_lane(arena + S.off, S.len, S.param, sync + S.aux, n_win, j);
}

// a chunk into LDS as words, zeros behind its n bytes
__device__ __forceinline__ void delta_load(const uint8_t *__restrict__ p, uint32_t n, uint32_t *x)
{
#pragma unroll
    for (uint32_t q = 0; q < kDeltaChunk / (kDeltaThreads * 16); q++) {
        const uint32_t c = q * kDeltaThreads + threadIdx.x, at = c * 16;
        uint32_t w[4];
        if (at + 16 <= n) {
            const uint4 v = *reinterpret_cast<const uint4 *>(p + at);
            w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
        } else {
            load_tail(p + at, at < n ? n - at : 0u, w);
        }
        x[4 * c] = w[0], x[4 * c + 1] = w[1], x[4 * c + 2] = w[2], x[4 * c + 3] = w[3];
    }
}

__global__ __launch_bounds__(256) void xlz_filter_delta_sums_kernel(const uint8_t *__restrict__ arena, const DevStep *__restrict__ steps, uint32_t n_steps,
                                                                    uint8_t *__restrict__ sums)
{
    __shared__ uint32_t x[kDeltaWords];
    const DevStep S = steps[find_step(steps, n_steps, blockIdx.x)];
    const uint32_t c = blockIdx.x - S.first;
    if (c + 1 >= S.n_tiles) return; // (nothing follows the last chunk)
    const uint64_t P = (uint64_t)c * kDeltaChunk;
    const uint32_t d = S.param;
    uint32_t n = kDeltaChunk; // (every chunk but the last is whole)
    delta_load(arena + S.off + P, n, x);
    __syncthreads();
    while (n > d) {
        const uint32_t h = delta_fold_at(n, d), words = (n - h + 3) / 4;
        uint32_t v[kDeltaWords / 2 / kDeltaThreads];
#pragma unroll
        for (uint32_t q = 0; q < kDeltaWords / 2 / kDeltaThreads; q++) {
            const uint32_t j = q * kDeltaThreads + threadIdx.x;
            v[q] = j < words ? delta_fold_word(x, n, h, j) : 0u;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t q = 0; q < kDeltaWords / 2 / kDeltaThreads; q++) {
            const uint32_t j = q * kDeltaThreads + threadIdx.x;
            if (j < words) x[j] = v[q];
        }
        __syncthreads();
        n = h;
    }
    const uint32_t k = threadIdx.x; // column k of the chunk is residue (P + k) mod d of the stream
    if (k < d) sums[(S.aux + c) * kDeltaMaxDist + (uint32_t)((P + k) % d)] = (uint8_t)(x[k >> 2] >> (8 * (k & 3)));
}

// one workgroup per group of kDeltaGroup chunks of a stream, a thread per residue (delta_group_scan) ...
__global__ __launch_bounds__(256) void xlz_filter_delta_scan_kernel(const DevStep *__restrict__ steps, uint32_t n_steps, uint8_t *__restrict__ sums,
                                                                    uint8_t *__restrict__ gsums)
{
    uint32_t lo = 0, hi = n_steps - 1; // the step whose groups include blockIdx.x (aux2 ascends)
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (steps[mid].aux2 <= blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const DevStep S = steps[lo];
    if (threadIdx.x >= S.param) return;
    delta_group_scan(sums + S.aux * kDeltaMaxDist, gsums + (uint64_t)blockIdx.x * kDeltaMaxDist, S.n_tiles, blockIdx.x - (uint32_t)S.aux2, threadIdx.x);
}
// ... and one workgroup per stream over its groups' totals
__global__ __launch_bounds__(256) void xlz_filter_delta_scan2_kernel(const DevStep *__restrict__ steps, uint8_t *__restrict__ gsums)
{
    const DevStep S = steps[blockIdx.x];
    if (threadIdx.x >= S.param) return;
    delta_groups_scan(gsums + S.aux2 * kDeltaMaxDist, (uint32_t)delta_groups(S.n_tiles), threadIdx.x);
}

__global__ __launch_bounds__(256) void xlz_filter_delta_apply_kernel(uint8_t *__restrict__ arena, const DevStep *__restrict__ steps, uint32_t n_steps,
                                                                     const uint8_t *__restrict__ sums, const uint8_t *__restrict__ gsums)
{
    __shared__ uint32_t x[kDeltaWords];
    const DevStep S = steps[find_step(steps, n_steps, blockIdx.x)];
    const uint32_t c = blockIdx.x - S.first;
    const uint64_t P = (uint64_t)c * kDeltaChunk;
    const uint32_t d = S.param;
    const uint32_t n = S.len - P < kDeltaChunk ? (uint32_t)(S.len - P) : kDeltaChunk;
    uint8_t *p = arena + S.off + P;
    delta_load(p, n, x);
    __syncthreads();
    if (c && 4 * threadIdx.x < d) { // the carried-in sums onto the chunk's first d bytes (bytes behind n: never stored)
        uint32_t carry = 0;
#pragma unroll
        for (uint32_t b = 0; b < 4; b++) {
            const uint32_t k = 4 * threadIdx.x + b;
            if (k < d) carry |= (delta_carry(sums + S.aux * kDeltaMaxDist, gsums + S.aux2 * kDeltaMaxDist, c, (uint32_t)((P + k) % d)) & 0xFF) << (8 * b);
        }
        x[threadIdx.x] = add_bytes(x[threadIdx.x], carry);
    }
    __syncthreads();
    for (uint32_t s = d; s < n; s *= 2) {
        uint32_t v[kDeltaWords / kDeltaThreads];
#pragma unroll
        for (uint32_t q = 0; q < kDeltaWords / kDeltaThreads; q++) v[q] = delta_scan_word(x, s, q * kDeltaThreads + threadIdx.x);
        __syncthreads();
#pragma unroll
        for (uint32_t q = 0; q < kDeltaWords / kDeltaThreads; q++) x[q * kDeltaThreads + threadIdx.x] = v[q];
        __syncthreads();
    }
#pragma unroll
    for (uint32_t q = 0; q < kDeltaChunk / (kDeltaThreads * 16); q++) {
        const uint32_t ch = q * kDeltaThreads + threadIdx.x, at = ch * 16;
        if (at >= n) break;
        const uint32_t w[4] = {x[4 * ch], x[4 * ch + 1], x[4 * ch + 2], x[4 * ch + 3]};
        if (at + 16 <= n) *reinterpret_cast<uint4 *>(p + at) = make_uint4(w[0], w[1], w[2], w[3]);
        else store_tail(p + at, 0, n - at, w);
    }
}

// Queues one step of n_steps streams of one class on `stream`: cls 0 the fixed-width BCJ filters, 1 x86, 2 Delta.
// steps: the device table (sorted by `first`, `total_tiles` tiles in all); scratch: cls 1 the window table (uint16 per
// window), cls 2 the rows of sums (kDeltaMaxDist bytes per chunk) and, in scratch2, the `total_groups` rows of group
// totals.  -> the kernels queued, or -1.
int filter_launch(int cls, uint8_t *arena, const DevStep *steps, uint32_t n_steps, uint32_t total_tiles, void *scratch, void *scratch2,
                  uint32_t total_groups, hipStream_t stream)
{
    if (!n_steps || !total_tiles) return 0;
    int launches = 0;
    if (cls == 0) {
        hipLaunchKernelGGL(xlz_filter_bcj_kernel, dim3(total_tiles), dim3(256), 0, stream, arena, steps, n_steps);
        launches = 1;
    } else if (cls == 1) {
        hipLaunchKernelGGL(xlz_filter_x86_mark_kernel, dim3(total_tiles), dim3(256), 0, stream, (const uint8_t *)arena, steps, n_steps, (uint16_t *)scratch);
        hipLaunchKernelGGL(xlz_filter_x86_walk_kernel, dim3(total_tiles), dim3(256), 0, stream, arena, steps, n_steps, (const uint16_t *)scratch);
        launches = 2;
    } else {
        hipLaunchKernelGGL(xlz_filter_delta_sums_kernel, dim3(total_tiles), dim3(kDeltaThreads), 0, stream, (const uint8_t *)arena, steps, n_steps,
                           (uint8_t *)scratch);
        hipLaunchKernelGGL(xlz_filter_delta_scan_kernel, dim3(total_groups), dim3(kDeltaThreads), 0, stream, steps, n_steps, (uint8_t *)scratch,
                           (uint8_t *)scratch2);
        hipLaunchKernelGGL(xlz_filter_delta_scan2_kernel, dim3(n_steps), dim3(kDeltaThreads), 0, stream, steps, (uint8_t *)scratch2);
        hipLaunchKernelGGL(xlz_filter_delta_apply_kernel, dim3(total_tiles), dim3(kDeltaThreads), 0, stream, arena, steps, n_steps,
                           (const uint8_t *)scratch, (const uint8_t *)scratch2);
        launches = 4;
    }
    return hipGetLastError() == hipSuccess ? launches : -1;
}

} // namespace xlz
