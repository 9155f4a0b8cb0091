// xlz_check_dev.h -- the arithmetic of the CRC32 / CRC64 checks that run on the device next to the decode
// (xlz_check_dev.hip), in a form that compiles both as device code and as plain C++: a g++ program runs the 64-lane
// scheme lane by lane on the CPU (tests/c/check_dev_selftest.cpp).  The reference has no container code and no checks.
//
// Both CRCs are reflected (bit 0 of a register is the coefficient of the highest power); every value here is a RAW
// register: start value 0, no final inversion.  Raw registers are linear in the message, leading zero bytes do not
// change them, and  raw(A || B) = raw(A) * x^(8 |B|) mod P  ^  raw(B).  The start value and the final inversion of the
// published CRCs are put on once per range (range_finish).
//
// A range [off, off + len) of the output arena is read in ROWS of 64 lanes x 16 bytes, the first row starting at `off`
// rounded down to kBaseAlign: bytes in front of the range are taken as zero (free in a raw register), bytes behind it too
// (the last row's padding is taken back by a multiplication with x^-(8 pad)).  Lane l of a row reads the aligned sixteen
// bytes at row + 16 l and nothing else; a lane whose sixteen bytes straddle an end of the range reads the bytes inside it
// one by one.  Rows are grouped into SEGMENTS of kSegRows rows, one wave each.  Inside a segment lane l carries the
// register U_l of the strided sub-sequence (its chunk of every row) and moves it over one row per step,
//     U' = T(chunk ^ U),   T(v) = raw register of the 16 bytes v followed by 1008 zero bytes
// (sixteen table lookups, the tables in LDS): U_l is always 1008 = 63 x 16 bytes "ahead", so after the last row the
// segment's value is  XOR_l U_l * x^-(128 l)  (lane_finish, then a XOR over the lanes).  The segment values of a range are
// folded by fold_thread / range_finish: 256 threads each take every 256th segment (Horner with X^256, X = x^(8 kSegBytes)),
// scale their part by X^t and the parts are XORed -- no serial walk over the segments of a long range.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define XLZ_CHK_HD __host__ __device__ inline
#else
#define XLZ_CHK_HD inline
#endif

namespace xlzchk {

constexpr uint32_t kLanes = 64;
constexpr uint32_t kLaneBytes = 16;
constexpr uint32_t kRowBytes = kLanes * kLaneBytes;   // 1024
constexpr uint32_t kSegRows = 128;
constexpr uint32_t kSegBytes = kSegRows * kRowBytes;  // 128 KiB: one wave's share
constexpr uint64_t kBaseAlign = 128;                  // rows of a range start at its offset rounded down to this
constexpr uint32_t kFoldThreads = 256;                // threads that fold the segment values of one range
constexpr uint32_t kTabEntries = 16 * 256;

template <int W> struct Crc;
template <> struct Crc<32> {
    typedef uint32_t tab_t;
    static constexpr uint64_t poly = 0xEDB88320ull, ones = 0xFFFFFFFFull;
};
template <> struct Crc<64> {
    typedef uint64_t tab_t;
    static constexpr uint64_t poly = 0xC96C5795D7870F42ull, ones = ~0ull;
};

// a * b mod P on raw registers (x^0 is the top bit of the register)
template <int W> XLZ_CHK_HD uint64_t mulmod(uint64_t a, uint64_t b)
{
    uint64_t p = 0;
    for (int i = W - 1; i >= 0; i--) {
        p ^= b & (0ull - ((a >> i) & 1));
        b = (b >> 1) ^ (Crc<W>::poly & (0ull - (b & 1)));
    }
    return p;
}

template <int W> struct Consts {
    uint64_t x2n[64];                    // x^(2^k)
    uint64_t xinv2n[16];                 // x^-(2^k)
    uint64_t lane_k[kLanes];             // x^-(128 l)
    uint64_t seg_pow[kFoldThreads + 1];  // X^t, X = x^(8 kSegBytes)
};

template <int W> XLZ_CHK_HD uint64_t xpow(const Consts<W> &c, uint64_t bits)
{
    uint64_t r = 1ull << (W - 1);
    for (int k = 0; bits; k++, bits >>= 1)
        if (bits & 1) r = mulmod<W>(r, c.x2n[k]);
    return r;
}
// x^(8 n) for a byte count of any size
template <int W> XLZ_CHK_HD uint64_t xpow_bytes(const Consts<W> &c, uint64_t n)
{
    uint64_t r = 1ull << (W - 1);
    for (int k = 3; n && k < 64; k++, n >>= 1)
        if (n & 1) r = mulmod<W>(r, c.x2n[k]);
    if (n) { // (byte counts of 2^61 and more: the remaining factors by squaring)
        uint64_t s = mulmod<W>(c.x2n[63], c.x2n[63]);
        for (; n; n >>= 1, s = mulmod<W>(s, s))
            if (n & 1) r = mulmod<W>(r, s);
    }
    return r;
}
template <int W> XLZ_CHK_HD uint64_t xinvpow(const Consts<W> &c, uint32_t bits) // bits < 65536
{
    uint64_t r = 1ull << (W - 1);
    for (int k = 0; bits && k < 16; k++, bits >>= 1)
        if (bits & 1) r = mulmod<W>(r, c.xinv2n[k]);
    return r;
}

template <int W> inline void build_consts(Consts<W> &c)
{
    const uint64_t one = 1ull << (W - 1), mask = Crc<W>::ones;
    uint64_t p = one >> 1; // x
    for (int k = 0; k < 64; k++, p = mulmod<W>(p, p)) c.x2n[k] = p;
    // x^-1: undo "shift right, XOR the polynomial if a bit fell out" on the register of x^0 (the polynomial's top bit is set)
    uint64_t q = (((one ^ Crc<W>::poly) << 1) | 1) & mask;
    for (int k = 0; k < 16; k++, q = mulmod<W>(q, q)) c.xinv2n[k] = q;
    c.lane_k[0] = one;
    for (uint32_t l = 1; l < kLanes; l++) c.lane_k[l] = mulmod<W>(c.lane_k[l - 1], c.xinv2n[7]);
    const uint64_t X = xpow_bytes<W>(c, kSegBytes);
    c.seg_pow[0] = one;
    for (uint32_t t = 1; t <= kFoldThreads; t++) c.seg_pow[t] = mulmod<W>(c.seg_pow[t - 1], X);
}

// T[j][v]: the raw register of byte v followed by (15 - j) + 1008 zero bytes
template <int W> inline void build_tables(const Consts<W> &c, typename Crc<W>::tab_t *T)
{
    for (uint32_t j = 0; j < 16; j++) {
        const uint64_t shift = xpow_bytes<W>(c, 15 - j + (kRowBytes - kLaneBytes));
        for (uint32_t v = 0; v < 256; v++) {
            uint64_t r = v;
            for (int k = 0; k < 8; k++) r = (r >> 1) ^ (Crc<W>::poly & (0ull - (r & 1)));
            T[j * 256 + v] = (typename Crc<W>::tab_t)mulmod<W>(r, shift);
        }
    }
}

struct Chunk {
    uint32_t w[4];
};

// the sixteen bytes at arena + a (a: a multiple of 16) with everything outside [lo, hi) read as zero -- and not read at all
XLZ_CHK_HD Chunk load_chunk(const uint8_t *arena, uint64_t a, uint64_t lo, uint64_t hi)
{
    Chunk c;
    c.w[0] = c.w[1] = c.w[2] = c.w[3] = 0;
    if (a >= lo && a + kLaneBytes <= hi) {
#if defined(__HIP_DEVICE_COMPILE__)
        const uint4 v = *reinterpret_cast<const uint4 *>(arena + a);
        c.w[0] = v.x, c.w[1] = v.y, c.w[2] = v.z, c.w[3] = v.w;
#else
        memcpy(c.w, arena + a, kLaneBytes);
#endif
    } else if (a + kLaneBytes > lo && a < hi) {
        for (uint32_t k = 0; k < kLaneBytes; k++)
            if (a + k >= lo && a + k < hi) c.w[k >> 2] |= (uint32_t)arena[a + k] << (8 * (k & 3));
    }
    return c;
}

// one lane's step over one row: U' = T(chunk ^ U)
template <int W, class Tab> XLZ_CHK_HD uint64_t lane_step(uint64_t U, const Chunk &c, const Tab *T)
{
    uint64_t r = 0;
    for (uint32_t k = 0; k < 4; k++) {
        uint32_t w = c.w[k];
        if (k == 0) w ^= (uint32_t)U;
        if (k == 1 && W == 64) w ^= (uint32_t)(U >> 32);
        r ^= (uint64_t)T[(4 * k + 0) * 256 + (w & 0xFF)] ^ (uint64_t)T[(4 * k + 1) * 256 + ((w >> 8) & 0xFF)] ^
             (uint64_t)T[(4 * k + 2) * 256 + ((w >> 16) & 0xFF)] ^ (uint64_t)T[(4 * k + 3) * 256 + (w >> 24)];
    }
    return r;
}

struct SegGeom {
    uint64_t base; // arena offset of the segment's first row
    uint32_t rows;
    uint32_t pad;  // bytes of the last row behind the range's end (last segment only)
};
XLZ_CHK_HD uint64_t range_base(uint64_t off) { return off & ~(kBaseAlign - 1); }
XLZ_CHK_HD uint64_t range_segments(uint64_t off, uint64_t len)
{
    return len ? (off + len - range_base(off) + kSegBytes - 1) / kSegBytes : 0;
}
XLZ_CHK_HD SegGeom seg_geom(uint64_t off, uint64_t len, uint64_t s)
{
    SegGeom g;
    g.base = range_base(off) + s * kSegBytes;
    const uint64_t rem = off + len - g.base;
    if (rem >= kSegBytes) {
        g.rows = kSegRows, g.pad = 0;
    } else {
        g.rows = (uint32_t)((rem + kRowBytes - 1) / kRowBytes);
        g.pad = (uint32_t)((uint64_t)g.rows * kRowBytes - rem);
    }
    return g;
}

// lane `lane` of one segment: its register after the segment's last row
template <int W, class Tab>
XLZ_CHK_HD uint64_t seg_lane(const uint8_t *arena, const SegGeom &g, uint64_t lo, uint64_t hi, uint32_t lane, const Tab *T)
{
    uint64_t U = 0;
    uint64_t a = g.base + (uint64_t)lane * kLaneBytes;
    uint32_t r = 0;
    for (; r + 4 <= g.rows; r += 4, a += 4 * kRowBytes) { // (four rows' loads in flight)
        const Chunk c0 = load_chunk(arena, a, lo, hi), c1 = load_chunk(arena, a + kRowBytes, lo, hi),
                    c2 = load_chunk(arena, a + 2 * kRowBytes, lo, hi), c3 = load_chunk(arena, a + 3 * kRowBytes, lo, hi);
        U = lane_step<W>(U, c0, T);
        U = lane_step<W>(U, c1, T);
        U = lane_step<W>(U, c2, T);
        U = lane_step<W>(U, c3, T);
    }
    for (; r < g.rows; r++, a += kRowBytes) U = lane_step<W>(U, load_chunk(arena, a, lo, hi), T);
    return U;
}
// a lane's share of its segment's value: XOR these over the 64 lanes ...
template <int W> XLZ_CHK_HD uint64_t lane_finish(const Consts<W> &c, uint64_t U, uint32_t lane) { return mulmod<W>(U, c.lane_k[lane]); }
// ... and take the last row's padding back: the raw register of the range's bytes inside this segment
template <int W> XLZ_CHK_HD uint64_t seg_finish(const Consts<W> &c, uint64_t x, uint32_t pad)
{
    return pad ? mulmod<W>(x, xinvpow<W>(c, 8 * pad)) : x;
}

// thread t of kFoldThreads: its part of the fold of the FULL segments v[0 .. m - 2] (every one kSegBytes long; the last
// segment, v[m - 1], is put on by range_finish); XOR the parts of all threads
template <int W> XLZ_CHK_HD uint64_t fold_thread(const Consts<W> &c, const uint64_t *v, uint64_t m, uint32_t t)
{
    if (m < 2 || t > m - 2) return 0;
    // j = segments between segment i and the last one = m - 2 - i; this thread: j = t, t + 256, ... from the largest down
    uint64_t j = t + (m - 2 - t) / kFoldThreads * kFoldThreads;
    uint64_t acc = 0;
    for (;; j -= kFoldThreads) {
        acc = mulmod<W>(acc, c.seg_pow[kFoldThreads]) ^ v[m - 2 - j];
        if (j == t) break;
    }
    return mulmod<W>(acc, c.seg_pow[t]);
}
// F: the XOR of all threads' parts -> the published CRC of the range (start value all ones, inverted at the end)
template <int W> XLZ_CHK_HD uint64_t range_finish(const Consts<W> &c, uint64_t F, const uint64_t *v, uint64_t m, uint64_t off, uint64_t len)
{
    if (!len || !m) return 0;
    const uint64_t len_last = off + len - (range_base(off) + (m - 1) * kSegBytes);
    const uint64_t raw = mulmod<W>(F, xpow_bytes<W>(c, len_last)) ^ v[m - 1];
    return raw ^ mulmod<W>(Crc<W>::ones, xpow_bytes<W>(c, len)) ^ Crc<W>::ones;
}

// crc(A || B) from crc(A), crc(B) and |B| (published CRCs: the start values and inversions cancel)
template <int W> inline uint64_t combine(const Consts<W> &c, uint64_t a, uint64_t b, uint64_t len_b)
{
    return (mulmod<W>(a & Crc<W>::ones, xpow_bytes<W>(c, len_b)) ^ b) & Crc<W>::ones;
}

// one range as the device sees it
struct DevRange {
    uint64_t off, len;   // bytes of the arena, len > 0
    uint32_t seg_first;  // index of its first segment value
    uint32_t n_segs;
    uint32_t out_index;  // where its digest goes
    uint32_t reserved;
};

} // namespace xlzchk
