// xlz_sha256_dev.h -- SHA-256 (FIPS 180-4) of ranges of a batch's output arena as the device computes it
// (xlz_sha256_dev.hip), in a form that compiles both as device code and as plain C++: a g++ program runs one lane's code
// on the CPU (tests/c/sha256_dev_selftest.cpp).  Also the constants of the host-only plan that decides which ranges the
// device takes (xlz_sha256_plan, xlz_host.hip).  The reference has no container code and no checks.
//
// SHA-256 is a serial chain over the 64-byte blocks of ONE message; a batch has many messages.  ONE LANE takes one range:
// 64 ranges ride in a wave, and a wave is a workgroup, so the waves of a launch spread over all SIMDs.  A lane walks its
// range block by block:
//   * the sixteen message words of a block come from seventeen dwords of the arena, read at `off` rounded down to 4: the
//     last dword of the block before (carried in a register) and sixteen fresh ones (four 16-byte loads, dword aligned).
//     Word i is bytes s .. s + 3 (s = off & 3) of the dword pair (i, i + 1) in big-endian order: one byte permute
//     (v_perm_b32) does the misalignment and the byte swap at once.  The loads of block j + 1 are issued before block j
//     is compressed;
//   * the sixteen-word window of the message schedule is a circular buffer w[i & 15]; the 64 rounds are fully unrolled, so
//     every index is static and the window lives in registers -- there is no W array in memory;
//   * rotates are v_alignbit_b32, Ch and Maj are one v_bfi_b32 each ((x & y) | (~x & z)), the XORs of three fold to
//     v_xor3_b32 and the sums to v_add3_u32;
//   * blocks whose seventeen dwords would reach past the arena (the last one or two of the whole arena), and the bytes
//     behind the last full block, are read byte by byte, inside [off, off + len) only; the 0x80 byte, the zero fill and the
//     64-bit bit count are put into the window in registers, for one or two final blocks.
// A full block's aligned loads may FETCH up to three bytes in front of the range and four behind it (inside the arena
// allocation: `arena_bytes` bounds them); the permute selects none of them, so no byte outside [off, off + len) reaches a
// digest.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define XLZ_SHA_HD __host__ __device__ inline
#else
#define XLZ_SHA_HD inline
#endif
#if defined(__clang__)
#define XLZ_SHA_UNROLL _Pragma("unroll")
#elif defined(__GNUC__)
#define XLZ_SHA_UNROLL _Pragma("GCC unroll 64")
#else
#define XLZ_SHA_UNROLL
#endif

namespace xlzsha {

constexpr uint32_t kLanes = 64; // ranges per wave = per workgroup

// ---- the plan's constants -------------------------------------------------------------------------------------------
// NOT MEASURED YET: the instruction-count estimate.  A block is about 1660 vector instructions (the code object's
// disassembly); one wave alone on a SIMD issues one per 4 cycles, at 2.4 GHz that is 64 bytes per 6640 cycles = 23 MB/s per
// lane, rounded to 25; the host's rate is what a portable scalar SHA-256 does on one core of a current server CPU.
// tools/sha256_bench.py measures both on an MI355X box and writes profiles/device_sha256.txt: these two constants are to
// be replaced by its "rates for the plan" line (what one lane sustains when every SIMD has up to kWavesPerSimd waves of
// the kernel; what one host thread of sixteen sustains with xlzcheck::sha256).
constexpr double kLaneBytesPerS = 25.0e6;
constexpr double kHostBytesPerSPerThread = 350.0e6;
constexpr uint32_t kSimds = 1024;      // 256 CUs x 4
constexpr uint32_t kWavesPerSimd = 2;  // a SIMD issues a wave's vector instruction in 2 cycles, one wave alone one per 4
constexpr uint32_t kRoundLanes = kLanes * kSimds * kWavesPerSimd; // lanes that run side by side at the lane rate
constexpr double kMaxLaunchS = 0.5;    // no launch is planned to run longer at the built-in lane rate
constexpr uint64_t kMaxDeviceLen = (uint64_t)(kMaxLaunchS * kLaneBytesPerS); // ... so no range longer than this is the device's
constexpr uint32_t kHostThreads = 16;  // the front-ends' check threads

XLZ_SHA_HD uint32_t rotr(uint32_t x, uint32_t k)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(x, x, k);
#else
    return (x >> k) | (x << (32 - k));
#endif
}
// byte i of the result = byte sel.byte[i] of the eight bytes hi:lo (0-3 = lo, 4-7 = hi): v_perm_b32
XLZ_SHA_HD uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t v = (uint64_t)hi << 32 | lo;
    uint32_t r = 0;
    for (int i = 0; i < 4; i++) r |= (uint32_t)((v >> (8 * ((sel >> (8 * i)) & 7))) & 0xFF) << (8 * i);
    return r;
#endif
}
// the selector that makes the big-endian word of bytes s .. s + 3 of a dword pair
XLZ_SHA_HD uint32_t be_selector(uint32_t s) { return 0x00010203u + s * 0x01010101u; }

XLZ_SHA_HD constexpr uint32_t round_k(int i)
{
    constexpr uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
        0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
        0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
        0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
        0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
        0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
        0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    return K[i];
}

XLZ_SHA_HD void init(uint32_t h[8])
{
    h[0] = 0x6a09e667, h[1] = 0xbb67ae85, h[2] = 0x3c6ef372, h[3] = 0xa54ff53a;
    h[4] = 0x510e527f, h[5] = 0x9b05688c, h[6] = 0x1f83d9ab, h[7] = 0x5be0cd19;
}

// one block: w[] holds its sixteen words and is used up as the schedule's window
XLZ_SHA_HD void block(uint32_t h[8], uint32_t w[16])
{
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    XLZ_SHA_UNROLL
    for (int i = 0; i < 64; i++) {
        if (i >= 16) {
            const uint32_t x = w[(i + 1) & 15], y = w[(i + 14) & 15];
            const uint32_t s0 = rotr(x, 7) ^ rotr(x, 18) ^ (x >> 3), s1 = rotr(y, 17) ^ rotr(y, 19) ^ (y >> 10);
            w[i & 15] = w[i & 15] + s0 + w[(i + 9) & 15] + s1;
        }
        const uint32_t S1 = rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25), ch = g ^ (e & (f ^ g));
        const uint32_t S0 = rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22), maj = (a & c) | (b & (a | c));
        const uint32_t t1 = hh + S1 + ch + round_k(i) + w[i & 15], t2 = S0 + maj;
        hh = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;
    }
    h[0] += a, h[1] += b, h[2] += c, h[3] += d, h[4] += e, h[5] += f, h[6] += g, h[7] += hh;
}

// sixteen dwords at p (a multiple of 4)
XLZ_SHA_HD void load16(const uint8_t *p, uint32_t d[16])
{
#if defined(__HIP_DEVICE_COMPILE__)
    struct __attribute__((packed, aligned(4))) Quad {
        uint32_t x, y, z, w;
    };
    const Quad *q = reinterpret_cast<const Quad *>(p);
    XLZ_SHA_UNROLL
    for (int k = 0; k < 4; k++) {
        const Quad v = q[k];
        d[4 * k] = v.x, d[4 * k + 1] = v.y, d[4 * k + 2] = v.z, d[4 * k + 3] = v.w;
    }
#else
    memcpy(d, p, 64); // (little-endian hosts, like the device)
#endif
}
XLZ_SHA_HD uint32_t load1(const uint8_t *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return *reinterpret_cast<const uint32_t *>(p);
#else
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
#endif
}
// the words of a full block from its seventeen dwords: carry = dword 0, d = dwords 1 .. 16
XLZ_SHA_HD void words(uint32_t carry, const uint32_t d[16], uint32_t sel, uint32_t w[16])
{
    w[0] = perm(d[0], carry, sel);
    XLZ_SHA_UNROLL
    for (int i = 1; i < 16; i++) w[i] = perm(d[i], d[i - 1], sel);
}
// n <= 64 bytes at p, one by one, as big-endian words; the rest of the window is zero.  Without branches (an index behind
// the n bytes reads byte 0 again and drops it), so that the window stays in registers.
XLZ_SHA_HD void load_bytes(const uint8_t *p, uint32_t n, uint32_t w[16])
{
    XLZ_SHA_UNROLL
    for (int i = 0; i < 16; i++) {
        uint32_t v = 0;
        if (n) {
            XLZ_SHA_UNROLL
            for (int k = 0; k < 4; k++) {
                const uint32_t at = (uint32_t)(4 * i + k);
                const uint32_t byte = p[at < n ? at : 0];
                v |= (at < n ? byte : 0u) << (24 - 8 * k);
            }
        }
        w[i] = v;
    }
}
// w: the r < 64 bytes behind the last full block (load_bytes); len: the whole message.  Padding, bit count, last block(s).
XLZ_SHA_HD void finish(uint32_t h[8], uint32_t w[16], uint32_t r, uint64_t len)
{
    const uint32_t mark = 0x80u << (24 - 8 * (r & 3));
    XLZ_SHA_UNROLL
    for (int i = 0; i < 16; i++)
        w[i] |= (uint32_t)i == (r >> 2) ? mark : 0u;
    if (r >= 56) {
        block(h, w);
        XLZ_SHA_UNROLL
        for (int i = 0; i < 16; i++) w[i] = 0;
    }
    w[14] = (uint32_t)(len >> 29), w[15] = (uint32_t)(len << 3);
    block(h, w);
}

// One lane: the state after the range [off, off + len) of an arena of arena_bytes (off + len <= arena_bytes; the arena
// starts at a multiple of 4).  Nothing outside the arena is read.
XLZ_SHA_HD void lane_digest(const uint8_t *arena, uint64_t arena_bytes, uint64_t off, uint64_t len, uint32_t h[8])
{
    init(h);
    const uint64_t a = off & ~3ull, n_full = len >> 6;
    const uint32_t sel = be_selector((uint32_t)(off & 3));
    // fast blocks: those whose seventeen dwords [a + 64 j, a + 64 j + 68) lie inside the arena
    uint64_t n_fast = arena_bytes >= a + 68 ? (arena_bytes - a - 68) / 64 + 1 : 0;
    if (n_fast > n_full) n_fast = n_full;
    uint32_t w[16];
    if (n_fast) {
        uint32_t carry = load1(arena + a), cur[16], nxt[16] = {};
        const uint8_t *p = arena + a + 4;
        load16(p, cur);
        for (uint64_t j = 0; j < n_fast; j++, p += 64) {
            if (j + 1 < n_fast) load16(p + 64, nxt);
            words(carry, cur, sel, w);
            carry = cur[15];
            block(h, w);
            XLZ_SHA_UNROLL
            for (int i = 0; i < 16; i++) cur[i] = nxt[i];
        }
    }
    const uint8_t *q = arena + off + 64 * n_fast;
    for (uint64_t j = n_fast; j < n_full; j++, q += 64) {
        load_bytes(q, 64, w);
        block(h, w);
    }
    const uint32_t r = (uint32_t)(len & 63);
    load_bytes(q, r, w);
    finish(h, w, r, len);
}

// the digest's 32 bytes in FIPS order, as dwords of a little-endian memory image
XLZ_SHA_HD uint32_t digest_word(uint32_t x) { return perm(0, x, 0x00010203u); }

// one range as the device sees it (sorted by len, longest first)
struct DevRange {
    uint64_t off, len;  // bytes of the arena
    uint32_t out_index; // its digest: eight dwords at 8 * out_index
    uint32_t reserved;
};

} // namespace xlzsha
