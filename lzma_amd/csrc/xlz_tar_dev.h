// xlz_tar_dev.h -- the two device steps of listing a .tar image that lies in HBM (xlz_tar_dev.hip), in a form that compiles
// both as device code and as plain C++: a g++ program runs the lane scheme lane by lane on the CPU
// (tests/c/tar_dev_selftest.cpp).  The reference has no tar code; the judge of the rules is Python's tarfile.
//
// CLASSIFY.  A tar image is a chain of 512-byte blocks: header, data, header, data, ..., zero blocks.  Where the next header
// lies follows from the size field of the one before, a serial chain -- but WHICH blocks can be headers at all is a
// property of each block alone: the field at bytes 148-155 holds, in octal, the sum of the block's bytes (with the field
// itself counted as eight spaces).  flags[b] of every complete block: 2 -- every byte is zero; 1 -- a header candidate:
// the field parses (field_value) and equals the unsigned byte sum or the signed one (every byte >= 0x80 counts as
// byte - 256; tarfile and GNU tar accept both); 0 -- anything else.  A trailing partial block is never loaded.
//
// The lane scheme: a wave of 64 lanes takes a PAIR of blocks per load instruction, lane l the sixteen bytes at
// 16 * (l mod 32) of block 2 * pair + l / 32 -- consecutive lanes load consecutive 16 bytes, 1 KiB per instruction.  A lane
// folds its bytes into one word, the byte sum in bits 0-19 (at most 512 * 255) and the count of bytes >= 0x80 in bits
// 20-29 (at most 512), and five xor-shuffles (1, 2, 4, 8, 16: they never leave a half of the wave) leave the block's
// totals in all 32 lanes of its half; one ballot says which halves saw a non-zero byte.  The checksum field is bytes 4-11
// of lane 9's sixteen (148 = 9 * 16 + 4), so lane 9 of each half holds the field in its own registers: it swaps in spaces
// for the sum, parses the field, compares and stores the flag byte.  The parse is a short serial loop that only lane 9
// enters, and only when no byte of the field has a bit of 0xC8 set (NUL, space and '0'-'7' have none): for file data a
// wave skips it.  No LDS, no scratch, no atomics, no lane read beyond the shuffles.  A kernel round issues the loads of
// two pairs before it reduces either.
//
// GATHER.  Copies block idx[k] of the image to block k of a dense staging buffer, chunk c = 32 * k + (lane of the block)
// by thread c mod (threads of the grid): consecutive threads load and store consecutive 16 bytes.  Source and destination
// are 16-byte aligned.
//
// Every load goes through load16, which in the plain C++ build asserts that it lies inside the complete blocks of
// [image, image + len).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define XLZ_TAR_HD __host__ __device__ inline
#else
#include <assert.h>
#define XLZ_TAR_HD inline
#endif

namespace xlztar {

constexpr uint32_t kThreads = 256;     // a workgroup: four waves
constexpr uint32_t kBlockBytes = 512;  // a tar block
constexpr uint32_t kBlockLanes = 32;   // lanes that hold one block, 16 bytes each
constexpr uint32_t kFieldLane = 9;     // the lane of a block that holds bytes 148-155 (its bytes 4-11)
constexpr uint32_t kSumBits = 20;      // the packed word: byte sum below, count of high bytes above

struct Quad {
    uint32_t w[4]; // bytes 0-3, 4-7, 8-11, 12-15 (little-endian)
};

// the aligned sixteen bytes at image + off: inside the complete 512-byte blocks of the image, or the plain build aborts
XLZ_TAR_HD Quad load16(const uint8_t *image, uint64_t len, uint64_t off)
{
    Quad q;
#if defined(__HIP_DEVICE_COMPILE__)
    (void)len;
    const uint4 v = *reinterpret_cast<const uint4 *>(image + off);
    q.w[0] = v.x, q.w[1] = v.y, q.w[2] = v.z, q.w[3] = v.w;
#else
#if !defined(__HIPCC__)
    assert((off & 15) == 0 && off < (len & ~(uint64_t)511) && (len & ~(uint64_t)511) - off >= 16);
#endif
    (void)len;
    memcpy(q.w, image + off, 16);
#endif
    return q;
}
XLZ_TAR_HD void store16(uint8_t *dst, uint64_t off, Quad q)
{
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<uint4 *>(dst + off) = make_uint4(q.w[0], q.w[1], q.w[2], q.w[3]);
#else
#if !defined(__HIPCC__)
    assert((off & 15) == 0);
#endif
    memcpy(dst + off, q.w, 16);
#endif
}

// the sum of the four bytes of w
XLZ_TAR_HD uint32_t bytes_sum(uint32_t w)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u8(w, 0u, 0u); // the sum of |byte - 0| over the four bytes: one instruction
#else
    const uint32_t pairs = (w & 0x00FF00FFu) + ((w >> 8) & 0x00FF00FFu);
    return (pairs & 0xFFFFu) + (pairs >> 16);
#endif
}

struct Part {
    uint32_t packed; // byte sum | count of bytes >= 0x80 << kSumBits, the checksum field counted as eight spaces
    uint32_t any;    // the OR of the sixteen bytes as loaded: zero only for sixteen zero bytes
};

// what lane `sub` (0-31) of a block makes of its sixteen bytes
XLZ_TAR_HD Part lane_part(Quad q, uint32_t sub)
{
    Part p;
    p.any = q.w[0] | q.w[1] | q.w[2] | q.w[3];
    const bool field = sub == kFieldLane;
    const uint32_t w1 = field ? 0x20202020u : q.w[1], w2 = field ? 0x20202020u : q.w[2];
    const uint32_t sum = bytes_sum(q.w[0]) + bytes_sum(w1) + bytes_sum(w2) + bytes_sum(q.w[3]);
    const uint32_t high = (uint32_t)__builtin_popcount(q.w[0] & 0x80808080u) + (uint32_t)__builtin_popcount(w1 & 0x80808080u) +
                          (uint32_t)__builtin_popcount(w2 & 0x80808080u) + (uint32_t)__builtin_popcount(q.w[3] & 0x80808080u);
    p.packed = sum | high << kSumBits;
    return p;
}

// The checksum field, bytes 148-151 in lo and 152-155 in hi: optional leading spaces, one to seven octal digits, then
// only NUL or space up to the field's end -> the value; anything else (all spaces, all NUL, eight digits, a digit 8, a
// byte behind the terminator that is neither) -> -1.
XLZ_TAR_HD int32_t field_value(uint32_t lo, uint32_t hi)
{
    if (((lo | hi) & 0xC8C8C8C8u) != 0 || (lo | hi) == 0) return -1; // (a byte that is not 0x00-07, 0x10-17, 0x20-27, 0x30-37)
    const uint64_t f = (uint64_t)lo | (uint64_t)hi << 32;
    uint32_t i = 0, digits = 0;
    int32_t v = 0;
    while (i < 8 && (uint8_t)(f >> (8 * i)) == 0x20) i++;
    while (i < 8 && ((uint8_t)(f >> (8 * i)) & 0xF8) == 0x30) v = v * 8 + (int32_t)((f >> (8 * i)) & 7), digits++, i++;
    if (digits == 0 || digits > 7) return -1;
    for (; i < 8; i++) {
        const uint8_t b = (uint8_t)(f >> (8 * i));
        if (b != 0 && b != 0x20) return -1;
    }
    return v;
}

// the flag of a block from its reduced word, whether any lane of it saw a non-zero byte, and the field as lane 9 loaded it
XLZ_TAR_HD uint8_t block_flag(uint32_t packed, bool any, uint32_t field_lo, uint32_t field_hi)
{
    if (!any) return 2;
    const int32_t v = field_value(field_lo, field_hi);
    if (v < 0) return 0;
    const int32_t sum = (int32_t)(packed & ((1u << kSumBits) - 1)), high = (int32_t)(packed >> kSumBits);
    return v == sum || v == sum - 256 * high ? 1 : 0;
}

XLZ_TAR_HD uint64_t pair_count(uint64_t len) { return ((len >> 9) + 1) >> 1; }

#if !defined(__HIPCC__)
// What one wave does with pair `pair` of the image, all 64 lanes in turn: the loads, the five xor-shuffles, the ballot and
// lane 9's finish -- the same helpers in the same order as xlz_tar_classify_kernel.
inline void wave_pair(const uint8_t *image, uint64_t len, uint64_t pair, uint8_t *flags)
{
    const uint64_t n_blocks = len >> 9;
    Quad q[64];
    Part p[64];
    for (uint32_t lane = 0; lane < 64; lane++) {
        const uint64_t blk = 2 * pair + lane / kBlockLanes;
        const uint32_t sub = lane % kBlockLanes;
        q[lane] = Quad{{0, 0, 0, 0}};
        if (blk < n_blocks) q[lane] = load16(image, len, blk * kBlockBytes + 16 * sub);
        p[lane] = lane_part(q[lane], sub);
    }
    for (uint32_t x = 1; x < kBlockLanes; x <<= 1) {
        uint32_t next[64];
        for (uint32_t lane = 0; lane < 64; lane++) next[lane] = p[lane].packed + p[lane ^ x].packed;
        for (uint32_t lane = 0; lane < 64; lane++) p[lane].packed = next[lane];
    }
    uint64_t ballot = 0;
    for (uint32_t lane = 0; lane < 64; lane++) ballot |= (uint64_t)(p[lane].any != 0) << lane;
    for (uint32_t lane = 0; lane < 64; lane++) {
        const uint64_t blk = 2 * pair + lane / kBlockLanes;
        if (lane % kBlockLanes != kFieldLane || blk >= n_blocks) continue;
        const bool any = (uint32_t)(ballot >> (lane & kBlockLanes)) != 0;
        flags[blk] = block_flag(p[lane].packed, any, q[lane].w[1], q[lane].w[2]);
    }
}
#endif

// gather: what the thread that has chunk c does (c < 32 * n; every idx[k] < len / 512, the launch checks it)
XLZ_TAR_HD void gather_chunk(const uint8_t *image, uint64_t len, const uint64_t *idx, uint8_t *staging, uint64_t c)
{
    const uint64_t k = c / kBlockLanes, at = 16 * (c % kBlockLanes);
    store16(staging, k * kBlockBytes + at, load16(image, len, idx[k] * kBlockBytes + at));
}

} // namespace xlztar
