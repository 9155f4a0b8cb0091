// xlz_adler_dev.h -- the arithmetic of Adler-32 over ranges of a device buffer (xlz_adler_dev.hip), in a form that compiles
// both as device code and as plain C++: a g++ program runs the 64-lane scheme lane by lane on the CPU
// (tests/c/adler_dev_selftest.cpp).  Written from RFC 1950 section 8.2; the reference has no checks, and none of zlib's
// code is here.
//
// Adler-32 of bytes d_0 .. d_(n-1):  A = 1 + SUM d_i,  B = SUM over i of the running A = n + SUM (n - i) d_i, both mod
// 65521; the digest is B << 16 | A.  Two facts carry the scheme.  A zero byte IN FRONT of the data changes neither sum of
// the "raw" pair  S = SUM d_i,  W = SUM (n - i) d_i  (its weight is multiplied by 0), and zero bytes BEHIND the data leave S
// as it is and add pad * S to W: masked bytes are free or cheap, as in the CRC kernels.  And the digests of two
// neighbours combine:  A = A1 + A2 - 1,  B = B1 + B2 + len2 (A1 - 1).
//
// The geometry is the CRC kernels' (xlz_check_dev.h): a range [off, off + len) is read in ROWS of 64 lanes x 16 bytes, the
// first row at `off` rounded down to 128; lane l of a row loads the aligned sixteen bytes at row + 16 l -- or, where they
// straddle an end of the range, the bytes inside it one by one -- and nothing else; rows are grouped into SEGMENTS of
// kSegRows rows, one wave each.  Per line a lane forms  s = SUM d_j  and  w = SUM (16 - j) d_j  (the weight of a byte
// counted to the END of its line), and carries three sums over the rows r = 0 .. R-1 of its segment:
//     S_l = SUM_r s,     W_l = SUM_r w,     T_l = SUM_r s * (R - 1 - r)     (T += S, then S += s: a sum of prefix sums)
// Behind lane l's line lie (63 - l) * 16 bytes of its row, behind row r lie (R - 1 - r) * 1024 bytes of the segment, so
//     lane:     B_l = W_l + 16 (63 - l) S_l + 1024 T_l
//     segment:  S = SUM_l S_l,   W = SUM_l B_l - pad * S       (pad: the masked bytes behind the range in the last row)
//               A = 1 + S,       B = n + W                      (n: the bytes of the range inside the segment)
// -- the Adler-32 of the range's bytes inside the segment.  A range's segments are folded by the combine rule, spelled out
// over all of them at once (it is associative):  A = 1 + SUM_s (A_s - 1),  B = SUM_s [B_s + (A_s - 1) * behind_s],
// behind_s = the range's bytes behind segment s.  That is a plain sum: 64 threads take every 64th segment each and the
// parts are added by shuffles -- no serial walk over the segments of a long range, no LDS.
//
// THE MODULO IS DEFERRED, and this is the arithmetic, every byte taken as 0xFF.  All sums are uint32_t.
//   line     s <= 16 * 255 = 4080;  w <= 255 * (16 + 15 + ... + 1) = 255 * 136 = 34 680.
//   lane     after R rows  S_l <= 4080 R,  W_l <= 34 680 R,  T_l <= 4080 * R (R - 1) / 2.  T_l is the one that binds:
//            4080 * R (R - 1) / 2 < 2^32  <=>  R (R - 1) < 2 105 376.9  <=>  R <= 1451  (1451 * 1450 = 2 103 950; 1452 *
//            1451 = 2 106 852).  A lane may take kMaxLaneRows = 1451 rows = 23 216 bytes before a reduction is due.
//   wave     that is 1451 rows x 1024 = 1 485 824 bytes per wave.  A SEGMENT is kSegRows = 128 rows = 131 072 bytes, eleven
//            times below it: S_l <= 522 240, W_l <= 4 439 040, T_l <= 4080 * 8128 = 33 162 240.  The code reduces at the
//            end of every segment and never inside one.
//   finish   1024 * T_l would pass 2^32, so T_l is reduced first: 1024 * 65 520 = 67 092 480;  16 * 63 * S_l <=
//            1008 * 522 240 = 526 417 920;  B_l <= 4 439 040 + 526 417 920 + 67 092 480 = 597 949 440 < 2^32.  B_l is then
//            reduced, and the sums over the 64 lanes are at most 64 * 522 240 = 33 423 360 (S) and 64 * 65 520 = 4 193 280.
//   segment  pad < 1024 and S mod 65521:  pad * S <= 1023 * 65 520 = 67 026 960;  n <= 131 072 is reduced before it is added.
//   fold     every factor is reduced first: 65 520 * 65 520 = 4 292 870 400 < 2^32 = 4 294 967 296, but not with two more
//            terms added; the fold's sums are uint64_t and are reduced after every term.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "xlz_check_dev.h"

#define XLZ_ADL_HD XLZ_CHK_HD

namespace xlzadl {

using xlzchk::Chunk;
using xlzchk::kLaneBytes;
using xlzchk::kLanes;
using xlzchk::kRowBytes;
using xlzchk::kSegBytes;
using xlzchk::kSegRows;
using xlzchk::load_chunk;
using xlzchk::range_base;
using xlzchk::range_segments;
using xlzchk::seg_geom;
using xlzchk::SegGeom;

constexpr uint32_t kMod = 65521;       // the largest prime below 2^16
constexpr uint32_t kMaxLaneRows = 1451; // rows of 0xFF bytes a lane's uint32_t sums hold (the arithmetic is above)
constexpr uint32_t kFoldThreads = 64;   // threads that fold the segment values of one range: one wave
static_assert(4080ull * kMaxLaneRows * (kMaxLaneRows - 1) / 2 < (1ull << 32) && 4080ull * (kMaxLaneRows + 1) * kMaxLaneRows / 2 >= (1ull << 32),
              "kMaxLaneRows is the bound of T_l");
static_assert(kSegRows <= kMaxLaneRows, "a lane reduces at the end of a segment: a segment must not pass the bound");
static_assert(4439040ull + 1008ull * 4080 * kSegRows + 1024ull * (kMod - 1) < (1ull << 32), "B_l of a segment fits uint32_t");

// the two sums of one 16-byte line: s = SUM d_j, w = SUM (16 - j) d_j
struct LineSums {
    uint32_t s, w;
};
XLZ_ADL_HD LineSums line_sums(const Chunk &c)
{
    LineSums r = {0, 0};
#if defined(__HIP_DEVICE_COMPILE__) && __has_builtin(__builtin_amdgcn_udot4)
    // v_dot4_u32_u8: four byte products and their sum in one instruction; byte k of word q is d_(4 q + k)
    r.s = __builtin_amdgcn_udot4(c.w[0], 0x01010101u, r.s, false);
    r.s = __builtin_amdgcn_udot4(c.w[1], 0x01010101u, r.s, false);
    r.s = __builtin_amdgcn_udot4(c.w[2], 0x01010101u, r.s, false);
    r.s = __builtin_amdgcn_udot4(c.w[3], 0x01010101u, r.s, false);
    r.w = __builtin_amdgcn_udot4(c.w[0], 0x0D0E0F10u, r.w, false);
    r.w = __builtin_amdgcn_udot4(c.w[1], 0x090A0B0Cu, r.w, false);
    r.w = __builtin_amdgcn_udot4(c.w[2], 0x05060708u, r.w, false);
    r.w = __builtin_amdgcn_udot4(c.w[3], 0x01020304u, r.w, false);
#else
    for (uint32_t q = 0; q < 4; q++)
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t d = (c.w[q] >> (8 * k)) & 0xFF;
            r.s += d, r.w += (16 - (4 * q + k)) * d;
        }
#endif
    return r;
}

// what a lane carries through its segment
struct LaneAcc {
    uint32_t S, W, T;
};
XLZ_ADL_HD void lane_step(LaneAcc &a, const Chunk &c)
{
    const LineSums v = line_sums(c);
    a.T += a.S, a.S += v.s, a.W += v.w;
}

// lane `lane` of one segment: its sums after the segment's last row (no reduction inside: g.rows <= kSegRows <= kMaxLaneRows)
XLZ_ADL_HD LaneAcc seg_lane(const uint8_t *buf, const SegGeom &g, uint64_t lo, uint64_t hi, uint32_t lane)
{
    LaneAcc acc = {0, 0, 0};
    uint64_t a = g.base + (uint64_t)lane * kLaneBytes;
    uint32_t r = 0;
    for (; r + 4 <= g.rows; r += 4, a += 4 * kRowBytes) { // (four rows' loads in flight)
        const Chunk c0 = load_chunk(buf, a, lo, hi), c1 = load_chunk(buf, a + kRowBytes, lo, hi),
                    c2 = load_chunk(buf, a + 2 * kRowBytes, lo, hi), c3 = load_chunk(buf, a + 3 * kRowBytes, lo, hi);
        lane_step(acc, c0);
        lane_step(acc, c1);
        lane_step(acc, c2);
        lane_step(acc, c3);
    }
    for (; r < g.rows; r++, a += kRowBytes) lane_step(acc, load_chunk(buf, a, lo, hi));
    return acc;
}

// a lane's share of its segment: S_l as it is (64 of them fit) and B_l mod 65521; ADD each over the 64 lanes
struct LanePart {
    uint32_t s, b;
};
XLZ_ADL_HD LanePart lane_finish(const LaneAcc &a, uint32_t lane)
{
    LanePart p;
    p.s = a.S;
    p.b = (a.W + kLaneBytes * (kLanes - 1 - lane) * a.S + kRowBytes * (a.T % kMod)) % kMod;
    return p;
}
// the sums over the lanes -> the Adler-32 of the range's bytes inside the segment (n of them, pad masked bytes behind them)
XLZ_ADL_HD uint32_t seg_finish(uint32_t s_sum, uint32_t b_sum, uint32_t n, uint32_t pad)
{
    const uint32_t S = s_sum % kMod;
    const uint32_t W = (b_sum % kMod + kMod - pad * S % kMod) % kMod;
    return ((n % kMod + W) % kMod) << 16 | (1 + S) % kMod;
}
// the bytes of the range inside segment s of m, and the bytes of the range behind it
XLZ_ADL_HD uint64_t seg_begin(uint64_t off, uint64_t s) { return s ? range_base(off) + s * kSegBytes : off; }
XLZ_ADL_HD uint64_t seg_end(uint64_t off, uint64_t len, uint64_t s, uint64_t m) { return s + 1 < m ? range_base(off) + (s + 1) * kSegBytes : off + len; }

// one range as the device sees it (the CRC kernels' table)
using xlzchk::DevRange;

// thread t of kFoldThreads: its part of the fold of the segment digests v[0 .. m); ADD the parts of all threads mod 65521
struct FoldPart {
    uint32_t a, b; // SUM (A_s - 1), SUM [B_s + (A_s - 1) behind_s]
};
XLZ_ADL_HD FoldPart fold_thread(const uint32_t *v, uint64_t m, uint64_t off, uint64_t len, uint32_t t)
{
    uint64_t a = 0, b = 0;
    for (uint64_t s = t; s < m; s += kFoldThreads) {
        const uint64_t a1 = ((v[s] & 0xFFFF) + kMod - 1) % kMod, behind = (off + len - seg_end(off, len, s, m)) % kMod;
        a = (a + a1) % kMod;
        b = (b + (v[s] >> 16) + a1 * behind) % kMod;
    }
    FoldPart p = {(uint32_t)a, (uint32_t)b};
    return p;
}
XLZ_ADL_HD uint32_t range_finish(uint32_t a_sum, uint32_t b_sum) { return (b_sum % kMod) << 16 | (1 + a_sum % kMod) % kMod; }

// ---- host only: the serial digest and the combine rule (xlz_adler32_host / xlz_adler32_combine) ----
// `adler`: the digest so far (1 for none); the sums are reduced every kHostRun bytes: 255 * n (n + 1) / 2 + (n + 1) * 65520
// < 2^32 for n <= 5552
constexpr size_t kHostRun = 5552;
inline uint32_t host_update(uint32_t adler, const uint8_t *p, size_t n)
{
    uint32_t a = adler & 0xFFFF, b = adler >> 16;
    while (n) {
        const size_t k = n < kHostRun ? n : kHostRun;
        for (size_t i = 0; i < k; i++) a += p[i], b += a;
        a %= kMod, b %= kMod, p += k, n -= k;
    }
    return b << 16 | a;
}
// adler(X || Y) from adler(X), adler(Y) and |Y|
inline uint32_t combine(uint32_t x, uint32_t y, uint64_t len_y)
{
    const uint64_t a1 = ((x & 0xFFFF) % kMod + kMod - 1) % kMod, n = len_y % kMod;
    const uint64_t a = (a1 + (y & 0xFFFF)) % kMod, b = ((x >> 16) + (y >> 16) + n * a1) % kMod;
    return (uint32_t)(b << 16 | a);
}

} // namespace xlzadl
