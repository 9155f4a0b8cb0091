// xlz_inflate_dev.h -- a raw-deflate decoder (xlz_inflate_dev.hip), in a form that compiles both as device code and as
// plain C++: a g++ program runs the wave scheme lane by lane on the CPU (tests/c/inflate_dev_selftest.cpp), and
// host_inflate() below is the serial twin the library exports as xlz_inflate_host.  Written from RFC 1951; the reference
// has no deflate code, and none of zlib's is here.
//
// DEFLATE (RFC 1951).  A stream is a sequence of blocks, bits packed from the least significant bit of each byte.  A block
// begins with BFINAL (1 bit) and BTYPE (2 bits):
//   0  stored: the rest of the byte is skipped, LEN and NLEN = ~LEN (16 bits each, little-endian), LEN bytes as they are;
//   1  fixed codes: literal/length lengths 8 (0-143), 9 (144-255), 7 (256-279), 8 (280-287); thirty-two distance codes of 5;
//   2  dynamic codes: HLIT (5 bits, + 257), HDIST (5, + 1), HCLEN (4, + 4); HCLEN x 3 bits of code-length code lengths in
//      the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15; then HLIT + HDIST code lengths in that code: 0 - 15 as
//      they are, 16 = the length before 3 - 6 times (2 bits), 17 = zero 3 - 10 times (3 bits), 18 = zero 11 - 138 times (7);
//   3  an error.
// Codes are canonical Huffman codes (shorter first, then by symbol), sent most significant bit first.  Symbols: 0 - 255 a
// literal, 256 the end of the block, 257 - 285 a length 3 - 258 (with 0 - 5 extra bits) followed by a distance code 0 - 29
// (1 - 32 768, with 0 - 13 extra bits): copy `length` bytes from `distance` bytes back, byte by byte (they may overlap).
//
// WHAT IS AN ERROR, and in which order, is taken from how zlib 1.2.11 behaves, observed from outside (the tests compare
// with Python's zlib on every case): the first defect in stream order decides.
//   kStResult  block type 3; NLEN != ~LEN; HLIT > 29 or HDIST > 29; a repeat 16 with nothing in front of it, a repeat that
//              runs over HLIT + HDIST; an over-subscribed set of lengths; an incomplete one -- but a literal/length or a
//              distance set that is ONE code of length 1, or a distance set without any code, is accepted, and so is a
//              code-length set without any code (every symbol then reads as one bit and means length 0); no code for
//              end-of-block; a bit pattern that is no code; literal/length symbols 286, 287 and distance symbols 30, 31;
//              a distance greater than the bytes produced so far;
//   kStEof     the input ends first: a field or a code that the bits at hand do not settle;
//   kStOutCap  the output would pass out_cap.  The decoder that is the yardstick is given room for out_cap + 1 bytes, and
//              it goes on behind the byte that filled them until it has something to WRITE: a defect in the header of a
//              block, or a bit pattern that is no code, right behind that byte is still kStResult.  So this decoder counts
//              one byte more than it stores ("the byte of grace") before it gives up.
//   kStOk      the end-of-block of the final block; what follows in the input is ignored, *consumed = the bytes used
//              (the one that holds the last bit included).
//
// THE WAVE SCHEME.  One 64-lane workgroup -- one wave -- per stream.  Decoding a symbol is WAVE-UNIFORM: bit buffer, input
// position, output position and every decision are the same in all lanes (the compiler is told so where a value comes
// out of LDS, and keeps them in scalar registers); there is no lane 0 that the others wait for.  The lanes differ in the
// byte traffic:
//   input    a window of 64 aligned 16-byte lines in LDS, lane l loading line l; the bit buffer is filled from it by whole
//            32-bit words, bytes at and behind in_len read as zero and are never counted as available;
//   tables   per block, from the code lengths in LDS: lanes 1 - 15 count the codes of their length, then place the
//            symbols of their length in canonical order; then ALL lanes fill the first-level table, entry e (the next bits
//            of the stream) by walking the counts: u16 entries, symbol << 4 | length, 0 = longer than the table.
//            Literal/length 10 bits, distance 8, code lengths 7.  A longer code is found by the canonical walk over
//            count / first / symbol (one LDS read per bit);
//   literals go to the lane whose number is the count of pending ones -- a register, not memory -- and leave as ONE store
//            of up to 64 consecutive bytes: when 64 are pending, before a copy, at the end;
//   matches  64 bytes per step: lane l reads byte (i mod distance) of the source for i = step * 64 + l -- for a distance
//            below the length that is the replication the byte-by-byte copy produces, and the source never includes a
//            byte this match writes;
//   stored   blocks are copied sixteen bytes per lane: single bytes up to the destination's next 16-byte boundary, then
//            aligned 16-byte stores built from two aligned source lines by a byte shift, single bytes for the tail.
// THE WINDOW IS THE OUTPUT ITSELF: a match reads the destination in HBM through the same pointer it is written through,
// with plain loads and stores.  A wave's memory operations are issued in program order and go through one L1, so a load
// sees the wave's own earlier stores -- as the copy path of the decode kernels (xlz_kernel.hip: wave_copy) relies on.
// SAFETY: a word of input is taken from LDS only if it begins in front of in_len, and is masked to the bytes in front of
// it; every store lies in [dst, dst + out_cap): the position never passes out_cap, the byte of grace is only counted; a
// distance greater than the bytes THIS stream has produced is an error, so no load lies in front of dst; every turn of
// every loop consumes at least one bit of input or ends, so a damaged stream ends after at most 8 x in_len turns.
// Every stream pointer is a multiple of 16 and its allocation reaches the next multiple of 16 behind its length
// (xlz_inflate_batch's upload sees to that).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define XLZ_INF_HD __host__ __device__ inline
#define XLZ_INF_UNROLL _Pragma("unroll")
#else
#define XLZ_INF_HD inline
#define XLZ_INF_UNROLL
#endif

// How a piece of the scheme that the LANES run is written: XLZ_INF_LANES(lane) { ... } is the body of every lane -- on the
// device the lane's own, on the CPU a loop over all 64, one after the other; XLZ_INF_SYNC() stands between two such pieces
// where one reads LDS that the other wrote.  No piece reads what another lane writes in the same piece.
#if defined(__HIP_DEVICE_COMPILE__)
#define XLZ_INF_LANES(lane) for (uint32_t lane = threadIdx.x, once_ = 1; once_; once_ = 0)
#define XLZ_INF_SYNC() __syncthreads()
#define XLZ_INF_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define XLZ_INF_LANES(lane) for (uint32_t lane = 0; lane < xlzinf::kLanes; lane++)
#define XLZ_INF_SYNC() ((void)0)
#define XLZ_INF_UNI(x) ((uint32_t)(x))
#endif

namespace xlzinf {

constexpr uint32_t kLanes = 64;
constexpr uint32_t kLineBytes = 16;
constexpr uint32_t kWindow = kLanes * kLineBytes; // input bytes in LDS
constexpr uint32_t kLitBits = 10, kDistBits = 8, kClBits = 7; // first-level table widths
constexpr uint32_t kMaxLitSyms = 288, kMaxDistSyms = 32, kClSyms = 19;
constexpr uint32_t kStreamAlign = 16; // where xlz_inflate_batch puts the inputs it uploads

// What one wave inflates per second, in bytes of OUTPUT.  MEASURED on an MI355X by tools/inflate_bench.py
// (profiles/device_inflate.txt): a lone wave inflates 4 MiB of text (zlib level 6) in 582 ms, 7.2 MB/s.  The estimate that
// stood here before the tool had run was 20 MB/s -- a symbol taken as one LDS round trip for the table, a handful of
// scalar operations and, for a match, a flush, a load and a store in HBM, 150 ns per symbol of three bytes; the wave
// needs some 400 ns.  The launch-length rule (never a launch of more than half a second, as xlz_sha256_plan has it)
// follows from it: an item whose input or room is longer than kMaxDeviceLen is inflated on the host.
constexpr double kWaveBytesPerS = 7.2e6;
constexpr uint64_t kMaxDeviceLen = (uint64_t)(0.5 * kWaveBytesPerS);

constexpr int kStOk = 0, kStResult = -1, kStEof = -5, kStOutCap = -6; // XLZ_OK, XLZ_ERR_RESULT, _UNEXPECTED_EOF, _OUT_CAP

XLZ_INF_HD uint32_t len_base(uint32_t k) { return k < 8 ? 3 + k : k == 28 ? 258 : 3 + ((4 + (k & 3)) << ((k >> 2) - 1)); } // k = symbol - 257
XLZ_INF_HD uint32_t len_extra(uint32_t k) { return k < 8 || k == 28 ? 0 : (k >> 2) - 1; }
XLZ_INF_HD uint32_t dist_base(uint32_t d) { return d < 4 ? 1 + d : 1 + ((2 + (d & 1)) << ((d >> 1) - 1)); }
XLZ_INF_HD uint32_t dist_extra(uint32_t d) { return d < 4 ? 0 : (d >> 1) - 1; }
XLZ_INF_HD uint32_t cl_order(uint32_t i)
{ // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
    return i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 8 - ((i - 3) >> 1) : 8 + ((i - 4) >> 1);
}
XLZ_INF_HD uint32_t fixed_lit_len(uint32_t s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }

// ---- the serial twin: what xlz_inflate_host runs, and what the wave scheme is compared with ----
struct HostTable {
    uint16_t fast[1u << kLitBits];
    uint16_t sym[kMaxLitSyms];
    uint16_t cnt[16];
    uint32_t bits;
};
// -> 0, 1: over-subscribed, 2: incomplete; *max: the longest code
inline int host_build(HostTable &t, const uint8_t *lens, uint32_t n, uint32_t bits, uint32_t *max)
{
    uint16_t off[16];
    for (uint32_t l = 0; l < 16; l++) t.cnt[l] = 0;
    for (uint32_t s = 0; s < n; s++) t.cnt[lens[s]]++;
    t.cnt[0] = 0, t.bits = bits, *max = 0;
    int left = 1;
    for (uint32_t l = 1; l < 16; l++) {
        left = (left << 1) - t.cnt[l];
        if (left < 0) return 1;
        if (t.cnt[l]) *max = l;
    }
    off[1] = 0;
    for (uint32_t l = 1; l < 15; l++) off[l + 1] = (uint16_t)(off[l] + t.cnt[l]);
    for (uint32_t s = 0; s < n; s++)
        if (lens[s]) t.sym[off[lens[s]]++] = (uint16_t)s;
    memset(t.fast, 0, sizeof(uint16_t) << bits);
    uint32_t code = 0, idx = 0;
    for (uint32_t l = 1; l <= bits; l++) { // the codes of length l are code ... code + cnt[l] - 1, for sym[idx ...]
        for (uint32_t k = 0; k < t.cnt[l]; k++, code++, idx++) {
            uint32_t r = 0;
            for (uint32_t b = 0; b < l; b++) r |= (code >> b & 1) << (l - 1 - b);
            for (uint32_t e = r; e < 1u << bits; e += 1u << l) t.fast[e] = (uint16_t)(t.sym[idx] << 4 | l);
        }
        code <<= 1;
    }
    return left > 0 ? 2 : 0;
}

struct HostBits {
    const uint8_t *in;
    size_t len, pos; // pos: the next byte to take
    uint64_t hold;
    uint32_t n;      // bits in hold, all of them real
    void fill()
    {
        while (n <= 56 && pos < len) hold |= (uint64_t)in[pos++] << n, n += 8;
    }
    bool need(uint32_t k) // k <= 32
    {
        if (n < k) fill();
        return n >= k;
    }
    uint32_t peek(uint32_t k) const { return (uint32_t)(hold & ((1ull << k) - 1)); }
    void drop(uint32_t k) { hold >>= k, n -= k; }
    size_t used() const { return pos - n / 8; } // the bytes that hold a bit that was dropped
};
constexpr int kSymInvalid = -1, kSymEof = -2;
inline int host_sym(HostBits &b, const HostTable &t)
{
    b.fill();
    const uint32_t e = t.fast[(uint32_t)b.hold & ((1u << t.bits) - 1)];
    if (e & 15) {
        if ((e & 15) > b.n) return kSymEof;
        b.drop(e & 15);
        return (int)(e >> 4);
    }
    int code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l < 16; l++) {
        code |= (int)(b.hold >> (l - 1) & 1);
        const int count = t.cnt[l];
        if (code - count < first) {
            if (l > b.n) return kSymEof;
            b.drop(l);
            return t.sym[index + (code - first)];
        }
        index += count, first += count, first <<= 1, code <<= 1;
    }
    return b.n ? kSymInvalid : kSymEof;
}

// -> kStOk / kStResult / kStEof / kStOutCap; *produced (optional) = bytes written to out (0 unless kStOk), *consumed
// (optional) = bytes of input used (0 unless kStOk)
inline int host_inflate(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap, size_t *produced, size_t *consumed)
{
    if (produced) *produced = 0;
    if (consumed) *consumed = 0;
    HostBits b = {in, in_len, 0, 0, 0};
    HostTable lit, dist;
    uint8_t lens[kMaxLitSyms + kMaxDistSyms];
    size_t pv = 0; // bytes produced, the byte of grace among them (pv <= out_cap + 1; only the first out_cap are stored)
    const size_t room = out_cap + 1;
    auto eof = [&] { return pv > out_cap ? kStOutCap : kStEof; };
    bool have_fixed = false;
    for (;;) {
        if (!b.need(3)) return eof();
        const uint32_t last = b.peek(1), type = b.peek(3) >> 1;
        b.drop(3);
        if (type == 3) return kStResult;
        if (type == 0) {
            b.drop(b.n & 7);
            if (!b.need(32)) return eof();
            const uint32_t v = b.peek(32);
            b.drop(32);
            if ((v & 0xFFFF) != ((v >> 16) ^ 0xFFFF)) return kStResult;
            const size_t n = v & 0xFFFF, at = b.used(), have = n < in_len - at ? n : in_len - at;
            if (n) {
                if (pv == room) return kStOutCap;
                if (have > room - pv || (have == room - pv && have < n)) return kStOutCap;
                if (have < n) return pv + have > out_cap ? kStOutCap : kStEof;
                const size_t store = pv + n > out_cap ? out_cap - pv : n;
                memcpy(out + pv, in + at, store);
                pv += n;
                b.pos = at + n, b.hold = 0, b.n = 0;
            }
        } else {
            if (type == 1) {
                if (!have_fixed) {
                    uint32_t mx;
                    for (uint32_t s = 0; s < kMaxLitSyms; s++) lens[s] = (uint8_t)fixed_lit_len(s);
                    host_build(lit, lens, kMaxLitSyms, kLitBits, &mx);
                    for (uint32_t s = 0; s < kMaxDistSyms; s++) lens[s] = 5;
                    host_build(dist, lens, kMaxDistSyms, kDistBits, &mx);
                    have_fixed = true;
                }
            } else {
                have_fixed = false;
                if (!b.need(14)) return eof();
                const uint32_t nlen = b.peek(5) + 257, ndist = (b.peek(10) >> 5) + 1, ncode = (b.peek(14) >> 10) + 4;
                b.drop(14);
                if (nlen > 286 || ndist > 30) return kStResult;
                uint8_t cl[kClSyms] = {};
                for (uint32_t i = 0; i < ncode; i++) {
                    if (!b.need(3)) return eof();
                    cl[cl_order(i)] = (uint8_t)b.peek(3);
                    b.drop(3);
                }
                uint32_t mx;
                HostTable &clt = dist; // (not needed yet)
                const int rc = host_build(clt, cl, kClSyms, kClBits, &mx);
                if (rc == 1 || (rc == 2 && mx != 0)) return kStResult; // (incomplete is an error here, but for no code at all)
                for (uint32_t have = 0; have < nlen + ndist;) {
                    int s;
                    if (mx == 0) { // no code at all: a symbol is one bit and means 0
                        if (!b.need(1)) return eof();
                        b.drop(1);
                        s = 0;
                    } else {
                        s = host_sym(b, clt);
                        if (s == kSymEof) return eof();
                        if (s == kSymInvalid) return kStResult; // (cannot be: the set is complete)
                    }
                    if (s < 16) {
                        lens[have++] = (uint8_t)s;
                        continue;
                    }
                    const uint32_t xb = s == 16 ? 2 : s == 17 ? 3 : 7;
                    if (!b.need(xb)) return eof();
                    const uint32_t rep = (s == 18 ? 11 : 3) + b.peek(xb);
                    b.drop(xb);
                    if (s == 16 && have == 0) return kStResult;
                    if (have + rep > nlen + ndist) return kStResult;
                    const uint8_t v = s == 16 ? lens[have - 1] : 0;
                    for (uint32_t k = 0; k < rep; k++) lens[have++] = v;
                }
                if (lens[256] == 0) return kStResult;
                int r = host_build(lit, lens, nlen, kLitBits, &mx);
                if (r == 1 || (r == 2 && mx != 1)) return kStResult;
                r = host_build(dist, lens + nlen, ndist, kDistBits, &mx);
                if (r == 1 || (r == 2 && mx > 1)) return kStResult;
            }
            for (;;) {
                const int s = host_sym(b, lit);
                if (s == kSymEof) return eof();
                if (s == kSymInvalid || s >= 286) return kStResult;
                if (s == 256) break;
                if (s < 256) {
                    if (pv == room) return kStOutCap;
                    if (pv < out_cap) out[pv] = (uint8_t)s;
                    pv++;
                    continue;
                }
                uint32_t xb = len_extra((uint32_t)s - 257);
                if (!b.need(xb)) return eof();
                const uint32_t len = len_base((uint32_t)s - 257) + b.peek(xb);
                b.drop(xb);
                const int d = host_sym(b, dist);
                if (d == kSymEof) return eof();
                if (d == kSymInvalid || d >= 30) return kStResult;
                xb = dist_extra((uint32_t)d);
                if (!b.need(xb)) return eof();
                const size_t distance = dist_base((uint32_t)d) + b.peek(xb);
                b.drop(xb);
                if (pv == room) return kStOutCap;
                if (distance > pv) return kStResult;
                if (len > room - pv) return kStOutCap;
                for (uint32_t k = 0; k < len && pv + k < out_cap; k++) out[pv + k] = out[pv + k - distance];
                pv += len;
            }
        }
        if (last) break;
    }
    if (pv > out_cap) return kStOutCap;
    if (produced) *produced = pv;
    if (consumed) *consumed = b.used();
    return kStOk;
}

// ---- the wave scheme ----
struct DevItem {
    const uint8_t *in; // a multiple of 16 (see the head of this file)
    uint32_t in_len;
    uint32_t out_cap;  // (an item of 0xFFFF0000 bytes and more, in or out, never gets here)
    uint64_t dst;      // where the item's output goes, from the destination pointer
};
struct DevResult {
    uint32_t produced, consumed; // 0 unless kStOk
    int32_t status;
    uint32_t reserved;
};

// what a workgroup keeps in LDS
struct Wave {
    alignas(16) uint32_t win[kWindow / 4]; // the window of the input
    uint16_t lit_fast[1u << kLitBits], dist_fast[1u << kDistBits], cl_fast[1u << kClBits];
    uint16_t lit_sym[kMaxLitSyms], dist_sym[kMaxDistSyms], cl_sym[kClSyms + 1];
    uint16_t lit_cnt[16], dist_cnt[16], cl_cnt[16];
    uint8_t lens[kMaxLitSyms + kMaxDistSyms]; // literal/length lengths, the distance lengths behind them
    uint8_t cl_lens[kClSyms + 1];
};

// a value every lane holds a copy of its own of: the pending literal
#if defined(__HIP_DEVICE_COMPILE__)
struct LaneU32 {
    uint32_t v;
    XLZ_INF_HD uint32_t &at(uint32_t) { return v; }
};
#else
struct LaneU32 {
    uint32_t v[kLanes];
    XLZ_INF_HD uint32_t &at(uint32_t l) { return v[l]; }
};
#endif

XLZ_INF_HD void copy_line(uint32_t *to, const uint8_t *from) // sixteen bytes, both multiples of 16
{
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<uint4 *>(to) = *reinterpret_cast<const uint4 *>(from);
#else
    memcpy(to, from, 16);
#endif
}

// the wave's state: the same in every lane
struct Dec {
    const uint8_t *in;
    uint8_t *out; // NOT restrict: matches read what was stored through it
    uint32_t in_len, out_cap;
    // the bit buffer: `n` bits in hold, of which those behind in_len are zeros that avail() does not count
    uint64_t hold;
    uint32_t n;
    uint32_t next;     // the input word that goes into hold next: a multiple of 4
    uint32_t win_base; // the window holds [win_base, win_base + kWindow)
    // the output
    uint32_t pv;    // bytes produced, the byte of grace among them: <= out_cap + 1
    uint32_t wpos;  // bytes stored
    uint32_t npend; // literals pending in the lanes: wpos + npend = min(pv, out_cap)
};

XLZ_INF_HD void load_window(Wave &w, Dec &d, uint32_t base)
{
    d.win_base = base;
    XLZ_INF_SYNC();
    XLZ_INF_LANES(lane)
    {
        const uint32_t at = base + kLineBytes * lane;
        if (at < d.in_len) copy_line(w.win + 4 * lane, d.in + at); // (the line that holds the stream's last byte is read whole)
    }
    XLZ_INF_SYNC();
}
XLZ_INF_HD uint32_t input_word(Wave &w, Dec &d, uint32_t pos) // pos: a multiple of 4
{
    if (pos >= d.in_len) return 0;
    if (pos - d.win_base >= kWindow) load_window(w, d, pos & ~(kWindow - 1));
    uint32_t v = XLZ_INF_UNI(w.win[(pos - d.win_base) >> 2]);
    const uint32_t left = d.in_len - pos;
    if (left < 4) v &= (1u << (8 * left)) - 1;
    return v;
}
XLZ_INF_HD void fill(Wave &w, Dec &d)
{
    if (d.n <= 32) {
        d.hold |= (uint64_t)input_word(w, d, d.next) << d.n;
        d.n += 32, d.next += 4;
    }
}
XLZ_INF_HD uint64_t used_bits(const Dec &d) { return 8ull * d.next - d.n; }
XLZ_INF_HD uint64_t avail(const Dec &d) { return 8ull * d.in_len - used_bits(d); } // real bits in hold and behind it
XLZ_INF_HD bool need(Wave &w, Dec &d, uint32_t k)                                    // k <= 32
{
    fill(w, d);
    return avail(d) >= k;
}
XLZ_INF_HD uint32_t peek(const Dec &d, uint32_t k) { return (uint32_t)(d.hold & ((1ull << k) - 1)); }
XLZ_INF_HD void drop(Dec &d, uint32_t k) { d.hold >>= k, d.n -= k; }
XLZ_INF_HD void seek(Wave &w, Dec &d, uint32_t byte_pos) // <= in_len
{
    d.hold = 0, d.n = 0, d.next = byte_pos & ~3u;
    fill(w, d);
    drop(d, 8 * (byte_pos & 3));
}

// The tables of one code from lens[0 .. n): cnt[l] = the codes of length l, sym[] = the symbols in canonical order,
// fast[e] for every e < 1 << bits.  -> 0, 1: over-subscribed (nothing else is built), 2: incomplete; *max = the longest code
template <uint32_t bits> XLZ_INF_HD int build(const uint8_t *lens, uint32_t n, uint16_t *fast, uint16_t *sym, uint16_t *cnt, uint32_t *max)
{
    XLZ_INF_SYNC();
    XLZ_INF_LANES(lane)
    {
        if (lane < 16) {
            uint32_t c = 0;
            for (uint32_t s = 0; s < n && lane; s++) c += lens[s] == lane;
            cnt[lane] = (uint16_t)c;
        }
    }
    XLZ_INF_SYNC();
    uint32_t c[16]; // (every loop over it is unrolled: it stays in registers)
    XLZ_INF_UNROLL
    for (uint32_t l = 0; l < 16; l++) c[l] = XLZ_INF_UNI(cnt[l]);
    int left = 1;
    *max = 0;
    XLZ_INF_UNROLL
    for (uint32_t l = 1; l < 16; l++) {
        left = (left << 1) - (int)c[l];
        if (left < 0) return 1;
        if (c[l]) *max = l;
    }
    XLZ_INF_LANES(lane)
    {
        if (lane >= 1 && lane < 16) {
            uint32_t at = 0;
    XLZ_INF_UNROLL
            for (uint32_t l = 1; l < 16; l++) at += l < lane ? c[l] : 0;
            for (uint32_t s = 0; s < n; s++)
                if (lens[s] == lane) sym[at++] = (uint16_t)s; // (at most n symbols in all: inside sym[])
        }
    }
    XLZ_INF_SYNC();
    XLZ_INF_LANES(lane)
    {
        for (uint32_t e = lane; e < 1u << bits; e += kLanes) {
            int code = 0, first = 0, index = 0;
            uint32_t at = 0, len = 0; // the first length at which the bits are a code, and that code's place in sym[]
    XLZ_INF_UNROLL
            for (uint32_t l = 1; l <= bits; l++) {
                code |= (int)(e >> (l - 1) & 1);
                const int count = (int)c[l];
                const bool hit = !len && code - count < first;
                at = hit ? (uint32_t)(index + (code - first)) : at, len = hit ? l : len;
                index += count, first += count, first <<= 1, code <<= 1;
            }
            fast[e] = (uint16_t)(len ? (uint32_t)sym[at] << 4 | len : 0);
        }
    }
    XLZ_INF_SYNC();
    return left > 0 ? 2 : 0;
}

// the next symbol of a code, or kSymInvalid / kSymEof
XLZ_INF_HD int wave_sym(Wave &w, Dec &d, const uint16_t *fast, uint32_t bits, const uint16_t *cnt, const uint16_t *sym)
{
    fill(w, d);
    const uint64_t av = avail(d);
    const uint32_t e = XLZ_INF_UNI(fast[(uint32_t)d.hold & ((1u << bits) - 1)]);
    if (e & 15) {
        if ((e & 15) > av) return kSymEof;
        drop(d, e & 15);
        return (int)(e >> 4);
    }
    int code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l < 16; l++) {
        code |= (int)(d.hold >> (l - 1) & 1);
        const int count = (int)XLZ_INF_UNI(cnt[l]);
        if (code - count < first) {
            if (l > av) return kSymEof;
            drop(d, l);
            return (int)XLZ_INF_UNI(sym[index + (code - first)]);
        }
        index += count, first += count, first <<= 1, code <<= 1;
    }
    return av ? kSymInvalid : kSymEof;
}

// the pending literals leave as one store
XLZ_INF_HD void flush(Dec &d, LaneU32 &lit)
{
    if (!d.npend) return;
    XLZ_INF_LANES(lane)
    {
        if (lane < d.npend) d.out[d.wpos + lane] = (uint8_t)lit.at(lane);
    }
    d.wpos += d.npend, d.npend = 0;
}

// len bytes from `distance` back (0 < distance <= wpos, wpos + len <= out_cap, nothing pending)
XLZ_INF_HD void copy_match(Dec &d, uint32_t distance, uint32_t len)
{
    uint8_t *const to = d.out + d.wpos;
    const uint8_t *const from = to - distance;
    XLZ_INF_LANES(lane)
    {
        if (distance >= len) {
            for (uint32_t i = lane; i < len; i += kLanes) to[i] = from[i];
        } else if (distance == 1) {
            const uint8_t v = from[0];
            for (uint32_t i = lane; i < len; i += kLanes) to[i] = v;
        } else {
            for (uint32_t i = lane; i < len; i += kLanes) to[i] = from[i % distance];
        }
    }
    d.wpos += len;
}

XLZ_INF_HD void load_line(uint32_t q[4], const uint8_t *from) // sixteen bytes from a multiple of 16, into registers
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 v = *reinterpret_cast<const uint4 *>(from);
    q[0] = v.x, q[1] = v.y, q[2] = v.z, q[3] = v.w;
#else
    memcpy(q, from, 16);
#endif
}
XLZ_INF_HD void store_line(uint8_t *to, uint32_t y0, uint32_t y1, uint32_t y2, uint32_t y3) // `to`: a multiple of 16
{
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<uint4 *>(to) = make_uint4(y0, y1, y2, y3);
#else
    const uint32_t y[4] = {y0, y1, y2, y3};
    memcpy(to, y, 16);
#endif
}
// n bytes of the input at byte `at` (at + n <= in_len) to the output (wpos + n <= out_cap, nothing pending)
XLZ_INF_HD void copy_stored(Dec &d, uint32_t at, uint32_t n)
{
    uint8_t *const to = d.out + d.wpos;
    uint32_t head = (uint32_t)(0 - (uintptr_t)to) & 15;
    if (head > n) head = n;
    const uint32_t lines = (n - head) >> 4, tail = n - head - 16 * lines;
    XLZ_INF_LANES(lane)
    {
        if (lane < head) to[lane] = d.in[at + lane];
        for (uint32_t c = lane; c < lines; c += kLanes) {
            const uint32_t so = at + head + 16 * c, a = so & ~15u, sh = 8 * (so & 3), ws = (so & 15) >> 2;
            uint32_t p[4], q[4] = {0, 0, 0, 0};
            load_line(p, d.in + a);
            if (so & 15) load_line(q, d.in + a + 16); // (the second line holds bytes of this chunk, all in front of in_len)
            // words ws ... ws + 4 of the two lines, by a shifter of two stages (no indexed array: registers, not scratch)
            const bool one = ws & 1, two = ws & 2;
            const uint32_t z0 = one ? p[1] : p[0], z1 = one ? p[2] : p[1], z2 = one ? p[3] : p[2], z3 = one ? q[0] : p[3];
            const uint32_t z4 = one ? q[1] : q[0], z5 = one ? q[2] : q[1], z6 = one ? q[3] : q[2];
            const uint32_t u0 = two ? z2 : z0, u1 = two ? z3 : z1, u2 = two ? z4 : z2, u3 = two ? z5 : z3, u4 = two ? z6 : z4;
            const uint32_t up = 32 - sh;
            if (sh)
                store_line(to + head + 16 * c, u0 >> sh | u1 << up, u1 >> sh | u2 << up, u2 >> sh | u3 << up, u3 >> sh | u4 << up);
            else
                store_line(to + head + 16 * c, u0, u1, u2, u3);
        }
        if (lane < tail) to[head + 16 * lines + lane] = d.in[at + head + 16 * lines + lane];
    }
    d.wpos += n;
}

XLZ_INF_HD DevResult wave_fail(int status)
{
    DevResult r;
    r.produced = 0, r.consumed = 0, r.status = status, r.reserved = 0;
    return r;
}

// One stream, by one wave: every lane calls it with the same arguments and gets the same result.
XLZ_INF_HD DevResult wave_inflate(Wave &w, const DevItem &it, uint8_t *dst)
{
    Dec d;
    d.in = it.in, d.out = dst + it.dst, d.in_len = it.in_len, d.out_cap = it.out_cap;
    d.hold = 0, d.n = 0, d.next = 0, d.win_base = 0u - kWindow; // (no position is inside that window)
    d.pv = d.wpos = d.npend = 0;
    LaneU32 lit;
    XLZ_INF_LANES(lane) { lit.at(lane) = 0; }
    const uint32_t room = d.out_cap + 1;
    bool have_fixed = false;
#define XLZ_INF_EOF() wave_fail(d.pv > d.out_cap ? kStOutCap : kStEof)
    for (;;) {
        if (!need(w, d, 3)) return XLZ_INF_EOF();
        const uint32_t last = peek(d, 1), type = peek(d, 3) >> 1;
        drop(d, 3);
        if (type == 3) return wave_fail(kStResult);
        if (type == 0) {
            drop(d, d.n & 7);
            if (!need(w, d, 32)) return XLZ_INF_EOF();
            const uint32_t v = peek(d, 32);
            drop(d, 32);
            if ((v & 0xFFFF) != ((v >> 16) ^ 0xFFFF)) return wave_fail(kStResult);
            const uint32_t n = v & 0xFFFF, at = (uint32_t)(used_bits(d) >> 3), have = n < d.in_len - at ? n : d.in_len - at;
            if (n) {
                if (d.pv == room) return wave_fail(kStOutCap);
                if (have > room - d.pv || (have == room - d.pv && have < n)) return wave_fail(kStOutCap);
                if (have < n) return wave_fail(kStEof); // (pv + have <= out_cap)
                if (d.pv + n > d.out_cap) {
                    d.pv += n; // the block's last byte is the byte of grace: nothing of it is stored any more
                } else {
                    flush(d, lit);
                    copy_stored(d, at, n);
                    d.pv += n;
                }
                seek(w, d, at + n);
            }
        } else {
            if (type == 1) {
                if (!have_fixed) {
                    uint32_t mx;
                    XLZ_INF_SYNC();
                    XLZ_INF_LANES(lane)
                    {
                        for (uint32_t s = lane; s < kMaxLitSyms + kMaxDistSyms; s += kLanes)
                            w.lens[s] = (uint8_t)(s < kMaxLitSyms ? fixed_lit_len(s) : 5);
                    }
                    build<kLitBits>(w.lens, kMaxLitSyms, w.lit_fast, w.lit_sym, w.lit_cnt, &mx);
                    build<kDistBits>(w.lens + kMaxLitSyms, kMaxDistSyms, w.dist_fast, w.dist_sym, w.dist_cnt, &mx);
                    have_fixed = true;
                }
            } else {
                have_fixed = false;
                if (!need(w, d, 14)) return XLZ_INF_EOF();
                const uint32_t nlen = peek(d, 5) + 257, ndist = (peek(d, 10) >> 5) + 1, ncode = (peek(d, 14) >> 10) + 4;
                drop(d, 14);
                if (nlen > 286 || ndist > 30) return wave_fail(kStResult);
                XLZ_INF_SYNC();
                XLZ_INF_LANES(lane)
                {
                    if (lane <= kClSyms) w.cl_lens[lane] = 0;
                }
                XLZ_INF_SYNC();
                for (uint32_t i = 0; i < ncode; i++) {
                    if (!need(w, d, 3)) return XLZ_INF_EOF();
                    const uint32_t v = peek(d, 3), s = cl_order(i);
                    drop(d, 3);
                    XLZ_INF_LANES(lane)
                    {
                        if (lane == s) w.cl_lens[lane] = (uint8_t)v;
                    }
                }
                uint32_t mx;
                const int rc = build<kClBits>(w.cl_lens, kClSyms, w.cl_fast, w.cl_sym, w.cl_cnt, &mx);
                if (rc == 1 || (rc == 2 && mx != 0)) return wave_fail(kStResult); // (incomplete is an error here, but for no code at all)
                const uint32_t total = nlen + ndist;
                uint32_t prev = 0; // the length in front of `have`
                for (uint32_t have = 0; have < total;) {
                    int s;
                    if (mx == 0) { // no code at all: a symbol is one bit and means 0
                        if (!need(w, d, 1)) return XLZ_INF_EOF();
                        drop(d, 1);
                        s = 0;
                    } else {
                        s = wave_sym(w, d, w.cl_fast, kClBits, w.cl_cnt, w.cl_sym);
                        if (s == kSymEof) return XLZ_INF_EOF();
                        if (s == kSymInvalid) return wave_fail(kStResult); // (cannot be: the set is complete)
                    }
                    uint32_t rep = 1, val = (uint32_t)s;
                    if (s >= 16) {
                        const uint32_t xb = s == 16 ? 2 : s == 17 ? 3 : 7;
                        if (!need(w, d, xb)) return XLZ_INF_EOF();
                        rep = (s == 18 ? 11 : 3) + peek(d, xb);
                        drop(d, xb);
                        if (s == 16 && have == 0) return wave_fail(kStResult);
                        if (have + rep > total) return wave_fail(kStResult);
                        val = s == 16 ? prev : 0;
                    }
                    XLZ_INF_LANES(lane) // (a repeat is at most 138 long)
                    {
                        for (uint32_t k = lane; k < rep; k += kLanes) w.lens[have + k] = (uint8_t)val;
                    }
                    have += rep, prev = val;
                }
                XLZ_INF_SYNC();
                if (XLZ_INF_UNI(w.lens[256]) == 0) return wave_fail(kStResult);
                int r = build<kLitBits>(w.lens, nlen, w.lit_fast, w.lit_sym, w.lit_cnt, &mx);
                if (r == 1 || (r == 2 && mx != 1)) return wave_fail(kStResult);
                r = build<kDistBits>(w.lens + nlen, ndist, w.dist_fast, w.dist_sym, w.dist_cnt, &mx);
                if (r == 1 || (r == 2 && mx > 1)) return wave_fail(kStResult);
            }
            for (;;) {
                const int s = wave_sym(w, d, w.lit_fast, kLitBits, w.lit_cnt, w.lit_sym);
                if (s == kSymEof) return XLZ_INF_EOF();
                if (s == kSymInvalid || s >= 286) return wave_fail(kStResult);
                if (s == 256) break;
                if (s < 256) {
                    if (d.pv == room) return wave_fail(kStOutCap);
                    if (d.pv < d.out_cap) {
                        XLZ_INF_LANES(lane)
                        {
                            if (lane == d.npend) lit.at(lane) = (uint32_t)s;
                        }
                        if (++d.npend == kLanes) flush(d, lit);
                    }
                    d.pv++;
                    continue;
                }
                uint32_t xb = len_extra((uint32_t)s - 257);
                if (!need(w, d, xb)) return XLZ_INF_EOF();
                const uint32_t len = len_base((uint32_t)s - 257) + peek(d, xb);
                drop(d, xb);
                const int ds = wave_sym(w, d, w.dist_fast, kDistBits, w.dist_cnt, w.dist_sym);
                if (ds == kSymEof) return XLZ_INF_EOF();
                if (ds == kSymInvalid || ds >= 30) return wave_fail(kStResult);
                xb = dist_extra((uint32_t)ds);
                if (!need(w, d, xb)) return XLZ_INF_EOF();
                const uint32_t distance = dist_base((uint32_t)ds) + peek(d, xb);
                drop(d, xb);
                if (d.pv == room) return wave_fail(kStOutCap);
                if (distance > d.pv) return wave_fail(kStResult);
                if (len > room - d.pv) return wave_fail(kStOutCap);
                if (d.pv + len <= d.out_cap) { // (else its last byte is the byte of grace: nothing of it is stored any more)
                    flush(d, lit);
                    copy_match(d, distance, len);
                }
                d.pv += len;
            }
        }
        if (last) break;
    }
#undef XLZ_INF_EOF
    if (d.pv > d.out_cap) return wave_fail(kStOutCap);
    flush(d, lit);
    DevResult r;
    r.produced = d.pv, r.consumed = (uint32_t)((used_bits(d) + 7) >> 3), r.status = kStOk, r.reserved = 0;
    return r;
}

// the sizes xlz_inflate_batch lays an input out by: its place is a multiple of kStreamAlign, the next one behind its last line
XLZ_INF_HD uint64_t padded(uint64_t len) { return (len + kStreamAlign - 1) / kStreamAlign * kStreamAlign; }

} // namespace xlzinf
