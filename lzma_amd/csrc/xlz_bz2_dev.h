// xlz_bz2_dev.h -- the bzip2 block decoder: the serial twin (xlz_bz2_decode_host runs it block by block) and the LANE
// SCHEME that xlz_bz2.hip's kernels run, one 64-lane workgroup per block candidate.  Compiles as device code and as
// plain C++: tests/c/bz2_dev_selftest.cpp runs the lane scheme lane by lane on the CPU.  Written from the public
// description of the format; the reference has nothing of the kind.
//
// THE FORMAT.  Bits are read most significant first.
//   stream   "BZh" + '1'..'9'; the block size is level x 100 000
//   block    magic 0x314159265359 | 32-bit block CRC | 1 bit "randomised" | 24-bit origPtr | a 16-bit map of the used
//            sixteenths of the byte values and one 16-bit map per used sixteenth
//   tables   3 bits nGroups (2..6) | 15 bits nSelectors (>= 1; above 18002 the surplus is read and dropped) | the selectors,
//            unary (fewer ones than nGroups) through a move-to-front list | per group a 5-bit start length and per symbol
//            steps "1x" (10: +1, 11: -1) ended by a 0; every length is 1..20; the codes are canonical
//   symbols  0 / 1 = RUNA / RUNB: a run of the front byte whose length is a bijective base-2 number, least digit first |
//            k >= 2: the byte at place k - 1 of the move-to-front list, which goes to the front | the last symbol ends the
//            block.  A new selector every 50 symbols.
//   bytes    the inverse Burrows-Wheeler transform from origPtr, then the first-stage run-length code: four equal bytes are
//            followed by a count 0..251 (any byte value is taken as written) of further copies
//   end      0x177245385090 | the combined CRC (rotl1(combined) ^ blockCRC per block) | zero bits to a byte
//   CRC      CRC-32/BZIP2: polynomial 0x04C11DB7, not reflected, initial value and final xor 0xFFFFFFFF
// A randomised block (bit set) is XLZ_ERR_UNSUPPORTED: no encoder has written one since 1998.
//
// THE SCHEME.  Four phases over three kernels (a launch stays below half a second: see the rate constants).
//   A  symbols (bz2_symbols_kernel).  Symbol decode is wave-uniform: the bit buffer, the group and the run state are the
//      same in every lane; the input window (1 KiB), the six first-level tables (10 bits), the code lengths, the selectors
//      and the move-to-front list live in LDS.  The lanes refill the window, build the tables, shift the move-to-front
//      list (a word of four places each, double buffered) and spread the runs.  Out: the last column ll[] in scratch.
//   B  the successor vector (bz2_walk_kernel).  A histogram of ll[] by LDS atomics, its prefix sums, then the stable
//      counting sort a row of 64 places at a time: the rank among equal bytes inside a row comes from ballots, the running
//      counts live in LDS.  tt[j] = the place that follows j.
//   C  the walk (same kernel).  Up to kMarks marks at a power-of-two stride of the index space, plus the head tt[origPtr].
//      Every lane walks segments -- from a mark to the next mark or the head -- and leaves in tt[p] WHERE p lies: (segment,
//      step).  One pass over the at most kMarks + 1 segments, following where each ended, gives every segment of the head's
//      cycle its offset; then ALL places are scattered in parallel, pre[offset + step] = ll[p].  The successor vector need
//      not be one cycle (periodic content): the head's cycle of length L < nblock is then repeated, pre[j] = pre[j % L],
//      and marks on other cycles are walked but never placed.
//      The run-length code is then measured: each lane runs its 64th of pre[] from the five entry states there are
//      (fresh; one, two or three bytes equal to the chunk's first seen; a count expected), the 64 transfer tables are
//      composed in order, and every chunk knows its entry state and output offset -- whatever the content, no
//      resynchronisation point is needed.  Each lane then runs its chunk once more from the state it is entered in and
//      forms the CRC of what it expands to; the 64 parts are folded by multiplication by x^(8 length) modulo the
//      polynomial.  Out: the expanded length and its CRC -- the file's verdict is known before a byte is written.
//   D  expansion (bz2_expand_kernel) of the chain's blocks, each lane its chunk, straight into the destination window, and
//      the block CRCs once more over the destination (bz2_crc_kernel: 64 partial CRCs per block, folded the same way):
//      one that differs from phase C's is the device's fault, not the file's, and fails the call.
//
// SAFETY.  Every load of input goes through the LDS window, whose refill reads only lines that begin in front of in_len
// (the file's end; the upload pads every file to a multiple of 16), and bits behind in_len count as absent.  Every store
// of A, B and C lies in the candidate's own scratch: ll[], tt[] and pre[] hold `cap` places, nblock <= cap is tested before
// a byte or a run is stored, every tt value that is followed is < nblock by construction of the sort.  Every store of D
// lies in [dst_off, dst_off + out_len) of the block, which the host has placed inside the file's window.  Every loop
// consumes input bits, or advances a counter bounded by nblock (the walk: also by the cycle it is on), or ends.  A
// candidate that is no block -- a false magic -- ends as a status like any damaged stream.
//
// STATUSES, in stream order (the first defect decides, as for a serial reader; the input ending in front of it is
// XLZ_ERR_UNEXPECTED_EOF): origPtr > 10 + cap, an empty map, nGroups outside 2..6, nSelectors 0, a selector >= nGroups, a
// length outside 1..20, a bit pattern that is no code, a run symbol behind a run of 2^21 and more, a byte or run past the
// block size, origPtr >= nblock: XLZ_ERR_RESULT.  The randomised bit: XLZ_ERR_UNSUPPORTED.
//
// RATE CONSTANTS, measured on an MI355X by tools/bz2_bench.py on ONE full level-9 block of text (profiles/device_bz2.txt;
// they replace the estimates of 400 ns per symbol and 1 us per load): phase A 178.5 ms = at most 200 ns per block byte
// (symbols are fewer than bytes); phases B and C with the measuring and the CRC 39.8 ms = about 1400 ns per dependent load
// at two passes over nblock / 64 places per lane.  Content other than text has not been measured.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define XLZ_BZ2_HD __host__ __device__ inline
#else
#define XLZ_BZ2_HD inline
#endif

// XLZ_BZ2_LANES(lane) { ... } is the body of every lane -- on the device the lane's own, on the CPU a loop over all 64, one
// after the other; XLZ_BZ2_SYNC() stands between two such pieces where one reads what the other wrote.  No piece reads what
// another lane writes in the same piece.
#if defined(__HIP_DEVICE_COMPILE__)
#define XLZ_BZ2_LANES(lane) for (uint32_t lane = threadIdx.x, once_ = 1; once_; once_ = 0)
#define XLZ_BZ2_SYNC() __syncthreads()
#define XLZ_BZ2_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#define XLZ_BZ2_COUNT(p) atomicAdd((p), 1u)
#else
#define XLZ_BZ2_LANES(lane) for (uint32_t lane = 0; lane < xlzbz2::kLanes; lane++)
#define XLZ_BZ2_SYNC() ((void)0)
#define XLZ_BZ2_UNI(x) ((uint32_t)(x))
#define XLZ_BZ2_COUNT(p) (++*(p))
#endif

namespace xlzbz2 {

constexpr uint32_t kLanes = 64;
constexpr uint32_t kWindow = 1024; // input bytes in LDS
constexpr uint32_t kLevelBytes = 100000, kMaxBlock = 9 * kLevelBytes;
constexpr uint32_t kMaxSelectors = 18002, kMaxGroups = 6, kMaxAlpha = 258, kMaxCodeLen = 20, kGroupSyms = 50;
constexpr uint32_t kFastBits = 10;
constexpr uint32_t kMarks = 1024;          // at most: the stride is a power of two
constexpr uint32_t kRunLimit = 1u << 21;   // a run symbol of this weight is a defect
constexpr uint32_t kInputAlign = 16;       // where the upload puts the files
constexpr uint32_t kMaxInput = 0x7FFFFFF0; // bytes of its file that a candidate is given at most
constexpr uint64_t kBlockMagic = 0x314159265359ull, kEndMagic = 0x177245385090ull;
constexpr int kStOk = 0, kStResult = -1, kStEof = -5, kStUnsupported = -9; // include/xlz.h
constexpr int kStSlow = 2; // not a file's status: the walk gave the block up (see kWalkShare), the host decodes it

// Measured (see above).  A launch must stay below half a second, and a kernel's workgroups take candidates in turn: a
// round of candidates is cut (xlz_bz2.hip) where the sum of cap x kSymbolNs over its candidates exceeds what the grid's
// workgroups can do in kLaunchCapNs.  The walk's 1400 ns per load bound no round: phase A is the longer kernel.
constexpr double kSymbolNs = 200.0, kLaunchCapNs = 0.5e9;
// The walk's marks sit at a fixed stride, and a successor vector can be made to avoid them (1024 x 'b' then 898 975 x 'a' in
// the last column: tt[j] = j + 1024, which meets every mark in one sweep and then none for a thousand sweeps), so that ONE
// lane would chase most of the block's dependent loads.  No lane therefore walks more than nblock / kWalkShare + kWalkSlack
// places in all -- eight times a lane's fair share --; a block that needs more is given up (kStSlow) and decoded by the
// host's twin.  Text, noise and periodic content stay far below it.
constexpr uint32_t kWalkShare = 8, kWalkSlack = 4096;

// ---------------------------------------------------------------- CRC-32/BZIP2 ----
constexpr uint32_t kPoly = 0x04C11DB7u;
XLZ_BZ2_HD uint32_t crc_entry(uint32_t i)
{
    uint32_t c = i << 24;
    for (int k = 0; k < 8; k++) c = (c << 1) ^ ((c & 0x80000000u) ? kPoly : 0);
    return c;
}
XLZ_BZ2_HD uint32_t gf_mul(uint32_t a, uint32_t b) // a * b modulo the polynomial, bit 31 = x^31
{
    uint32_t r = 0;
    for (int i = 31; i >= 0; i--) {
        r = (r << 1) ^ ((r & 0x80000000u) ? kPoly : 0);
        if ((b >> i) & 1) r ^= a;
    }
    return r;
}
XLZ_BZ2_HD uint32_t gf_xpow(uint64_t n) // x^n
{
    uint32_t r = 1, base = 2;
    for (; n; n >>= 1) {
        if (n & 1) r = gf_mul(r, base);
        base = gf_mul(base, base);
    }
    return r;
}
struct CrcTable {
    uint32_t t[256];
    CrcTable()
    {
        for (uint32_t i = 0; i < 256; i++) t[i] = crc_entry(i);
    }
};
inline const uint32_t *crc_table()
{
    static const CrcTable table; // (made once, by whichever thread comes first: host threads share it)
    return table.t;
}
inline uint32_t host_crc(uint32_t crc, const uint8_t *p, size_t n) // of crc's bytes followed by p[0 .. n); crc = 0: of p alone
{
    const uint32_t *t = crc_table();
    uint32_t r = ~crc;
    for (size_t i = 0; i < n; i++) r = (r << 8) ^ t[(r >> 24) ^ p[i]];
    return ~r;
}

// ---------------------------------------------------------------- the serial twin ----
struct BlockInfo {
    int status;
    uint32_t nblock, orig, crc; // crc: the stored one
    uint64_t end_bit;           // where the block ended, in bits of `in`
    uint32_t out_len;           // bytes behind the run-length stage
    uint32_t calc_crc;          // their CRC as formed (host_decode)
};

struct HostBits {
    const uint8_t *in;
    uint64_t len_bits, pos;
    bool eof = false;
    uint32_t get(uint32_t k) // k <= 32; behind the end: eof, zeros
    {
        uint32_t v = 0;
        for (uint32_t i = 0; i < k; i++) {
            if (pos >= len_bits) {
                eof = true;
                return 0;
            }
            v = (v << 1) | ((in[pos >> 3] >> (7 - (pos & 7))) & 1);
            pos++;
        }
        return v;
    }
};

// One block that begins (with its magic) at bit `start_bit` of in[0 .. in_len): ll[] and tt[] hold `cap` places each, pre[]
// too; out (may be NULL: measure only) gets at most out_cap bytes of the expansion.  -> status; *bi is filled.
inline int host_block(const uint8_t *in, uint64_t in_len, uint64_t start_bit, uint32_t cap, uint8_t *ll, uint32_t *tt, uint8_t *pre, BlockInfo *bi)
{
    *bi = BlockInfo{};
    HostBits b{in, 8 * in_len, start_bit};
#define XLZ_BZ2_GET(var, k)                \
    const uint32_t var = b.get(k);         \
    if (b.eof) return bi->status = kStEof;
    for (int i = 5; i >= 0; i--) {
        XLZ_BZ2_GET(m, 8)
        if (m != ((kBlockMagic >> (8 * i)) & 255)) return bi->status = kStResult;
    }
    XLZ_BZ2_GET(crc, 32)
    bi->crc = crc;
    XLZ_BZ2_GET(rnd, 1)
    if (rnd) return bi->status = kStUnsupported;
    XLZ_BZ2_GET(orig, 24)
    bi->orig = orig;
    if (orig > 10 + cap) return bi->status = kStResult;
    XLZ_BZ2_GET(map16, 16)
    uint8_t seq[256];
    uint32_t n_used = 0;
    for (uint32_t i = 0; i < 16; i++)
        if (map16 & (0x8000u >> i)) {
            XLZ_BZ2_GET(m, 16)
            for (uint32_t j = 0; j < 16; j++)
                if (m & (0x8000u >> j)) seq[n_used++] = (uint8_t)(16 * i + j);
        }
    if (!n_used) return bi->status = kStResult;
    const uint32_t alpha = n_used + 2;
    XLZ_BZ2_GET(n_groups, 3)
    if (n_groups < 2 || n_groups > kMaxGroups) return bi->status = kStResult;
    XLZ_BZ2_GET(n_sel_read, 15)
    if (n_sel_read < 1) return bi->status = kStResult;
    static thread_local uint8_t sel[kMaxSelectors];
    {
        uint8_t pos[kMaxGroups] = {0, 1, 2, 3, 4, 5};
        for (uint32_t i = 0; i < n_sel_read; i++) {
            uint32_t j = 0;
            for (;;) {
                XLZ_BZ2_GET(bit, 1)
                if (!bit) break;
                if (++j >= n_groups) return bi->status = kStResult;
            }
            if (i < kMaxSelectors) {
                const uint8_t v = pos[j];
                for (; j; j--) pos[j] = pos[j - 1];
                sel[i] = pos[0] = v;
            }
        }
    }
    const uint32_t n_sel = n_sel_read < kMaxSelectors ? n_sel_read : kMaxSelectors;
    uint8_t len[kMaxGroups][kMaxAlpha];
    for (uint32_t t = 0; t < n_groups; t++) {
        XLZ_BZ2_GET(start, 5)
        uint32_t curr = start;
        for (uint32_t i = 0; i < alpha; i++) {
            for (;;) {
                if (curr < 1 || curr > kMaxCodeLen) return bi->status = kStResult;
                XLZ_BZ2_GET(more, 1)
                if (!more) break;
                XLZ_BZ2_GET(down, 1)
                curr += down ? -1 : 1;
            }
            len[t][i] = (uint8_t)curr;
        }
    }
    // canonical codes: cnt[t][l] codes of length l, perm[t][] the symbols by (length, symbol)
    uint16_t cnt[kMaxGroups][kMaxCodeLen + 2], perm[kMaxGroups][kMaxAlpha];
    for (uint32_t t = 0; t < n_groups; t++) {
        memset(cnt[t], 0, sizeof cnt[t]);
        uint32_t at = 0;
        for (uint32_t l = 1; l <= kMaxCodeLen; l++)
            for (uint32_t i = 0; i < alpha; i++)
                if (len[t][i] == l) perm[t][at++] = (uint16_t)i, cnt[t][l]++;
    }
    uint8_t mtf[256];
    for (uint32_t i = 0; i < 256; i++) mtf[i] = (uint8_t)i;
    uint32_t nblock = 0, group = 0, left = 0, run = 0, weight = 1;
    bool in_run = false;
    const uint32_t eob = n_used + 1;
    for (;;) {
        if (!left) {
            if (group >= n_sel) return bi->status = kStResult;
            left = kGroupSyms;
            group++;
        }
        left--;
        const uint32_t t = sel[group - 1];
        int code = 0, first = 0, index = 0;
        uint32_t sym = kMaxAlpha;
        for (uint32_t l = 1; l <= kMaxCodeLen + 1; l++) {
            XLZ_BZ2_GET(bit, 1)
            if (l > kMaxCodeLen) return bi->status = kStResult;
            code = (code << 1) | (int)bit;
            const int c = cnt[t][l];
            if (code - c < first) {
                if (code < first) return bi->status = kStResult;
                sym = perm[t][index + (code - first)];
                break;
            }
            index += c, first = (first + c) << 1;
        }
        if (sym <= 1) {
            if (!in_run) in_run = true, run = 0, weight = 1;
            if (weight >= kRunLimit) return bi->status = kStResult;
            run += weight << sym, weight <<= 1;
            continue;
        }
        if (in_run) {
            in_run = false;
            if (run > cap - nblock) return bi->status = kStResult;
            memset(ll + nblock, seq[mtf[0]], run);
            nblock += run;
        }
        if (sym == eob) break;
        if (nblock >= cap) return bi->status = kStResult;
        const uint32_t nn = sym - 1;
        const uint8_t v = mtf[nn];
        memmove(mtf + 1, mtf, nn);
        mtf[0] = v;
        ll[nblock++] = seq[v];
    }
#undef XLZ_BZ2_GET
    bi->nblock = nblock, bi->end_bit = b.pos;
    if (orig >= nblock) return bi->status = kStResult;
    uint32_t cf[257] = {0};
    for (uint32_t i = 0; i < nblock; i++) cf[ll[i] + 1]++;
    for (uint32_t i = 0; i < 256; i++) cf[i + 1] += cf[i];
    for (uint32_t i = 0; i < nblock; i++) tt[cf[ll[i]]++] = i;
    uint32_t p = tt[orig], r = 0, last = 0;
    uint64_t out_len = 0;
    for (uint32_t i = 0; i < nblock; i++) {
        const uint8_t x = ll[p];
        p = tt[p];
        pre[i] = x;
        if (r == 4) {
            out_len += x, r = 0;
        } else if (r && x == last) {
            r++, out_len++;
        } else {
            last = x, r = 1, out_len++;
        }
    }
    bi->out_len = (uint32_t)out_len; // (at most 900 000 / 5 x 259)
    return bi->status = kStOk;
}
// the run-length stage of pre[0 .. n) -> out[0 .. out_len)
inline void host_expand(const uint8_t *pre, uint32_t n, uint8_t *out)
{
    uint32_t r = 0, last = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint8_t x = pre[i];
        if (r == 4) {
            memset(out, (int)last, x);
            out += x, r = 0;
        } else if (r && x == last) {
            r++, *out++ = x;
        } else {
            last = x, r = 1, *out++ = x;
        }
    }
}

// ---------------------------------------------------------------- the lane scheme ----
struct DevCand {
    uint64_t in_off;      // of the gathered image: a multiple of kInputAlign
    uint32_t in_len;      // bytes from there to the file's end, at most kMaxInput
    uint32_t start_bit;   // of the magic, from in_off
    uint32_t cap;         // level x 100 000 of the stream it is taken to lie in
    uint32_t reserved;
    uint64_t scratch_off; // a multiple of 16
};
struct DevState { // one per candidate
    int32_t status;
    uint32_t nblock, orig, crc;
    uint64_t end_bit; // from in_off
    uint32_t out_len, calc_crc; // of the expansion: its length and its CRC as formed (crc: as stored)
};
struct DevChunk { // one per lane and candidate: where lane's 64th of pre[] enters the run-length stage
    uint32_t out_off, run, last, reserved;
};
struct DevPlace { // one per chain block: what D expands and whose CRC is formed
    uint32_t cand, out_len;
    uint64_t dst_off;
};
XLZ_BZ2_HD uint64_t round16(uint64_t x) { return (x + 15) & ~(uint64_t)15; }
// the scratch of a candidate of `cap` places: tt | ll | pre | chunks
XLZ_BZ2_HD uint64_t scratch_bytes(uint32_t cap) { return round16(4ull * cap) + 2 * round16(cap) + kLanes * sizeof(DevChunk); }
struct Scratch {
    uint32_t *tt;
    uint8_t *ll, *pre;
    DevChunk *chunks;
};
XLZ_BZ2_HD Scratch scratch_of(uint8_t *base, uint32_t cap)
{
    Scratch s;
    s.tt = reinterpret_cast<uint32_t *>(base);
    s.ll = base + round16(4ull * cap);
    s.pre = s.ll + round16(cap);
    s.chunks = reinterpret_cast<DevChunk *>(s.pre + round16(cap));
    return s;
}

// LDS of phase A
struct WaveA {
    uint32_t win[kWindow / 4];
    uint16_t fast[kMaxGroups][1u << kFastBits]; // symbol | length << 9; 0: longer than kFastBits; symbol 511: no code
    uint16_t perm[kMaxGroups][kMaxAlpha + 2];
    uint16_t cnt[kMaxGroups][kMaxCodeLen + 4];
    uint8_t len[kMaxGroups][kMaxAlpha + 2];
    uint8_t sel[kMaxSelectors + 2];
    uint8_t seq[256];
    uint32_t mtf[2][kLanes]; // place 4 w + k is byte k of word w
    uint8_t pend[kLanes];
};
constexpr uint32_t kNoCode = 511;

struct Bits { // the same in every lane
    const uint8_t *in;
    uint32_t in_len;
    uint64_t hold; // the next bit is bit 63
    uint32_t n, next, win_base;
};
XLZ_BZ2_HD void load_window(WaveA &w, Bits &b, uint32_t base)
{
    b.win_base = base;
    XLZ_BZ2_SYNC();
    XLZ_BZ2_LANES(lane)
    {
        const uint32_t at = base + 16 * lane;
        if (at < b.in_len) {
#if defined(__HIP_DEVICE_COMPILE__)
            *reinterpret_cast<uint4 *>(w.win + 4 * lane) = *reinterpret_cast<const uint4 *>(b.in + at);
#else
            memcpy(w.win + 4 * lane, b.in + at, 16);
#endif
        }
    }
    XLZ_BZ2_SYNC();
}
XLZ_BZ2_HD uint32_t input_word(WaveA &w, Bits &b, uint32_t pos) // pos: a multiple of 4 -> its four bytes, the first on top
{
    if (pos >= b.in_len) return 0;
    if (pos - b.win_base >= kWindow) load_window(w, b, pos & ~(kWindow - 1));
    uint32_t v = __builtin_bswap32(XLZ_BZ2_UNI(w.win[(pos - b.win_base) >> 2]));
    const uint32_t left = b.in_len - pos;
    if (left < 4) v &= ~(0xFFFFFFFFu >> (8 * left));
    return v;
}
XLZ_BZ2_HD void fill(WaveA &w, Bits &b)
{
    if (b.n <= 32) {
        b.hold |= (uint64_t)input_word(w, b, b.next) << (32 - b.n);
        b.n += 32, b.next += 4;
    }
}
XLZ_BZ2_HD uint64_t used_bits(const Bits &b) { return 8ull * b.next - b.n; }
XLZ_BZ2_HD uint64_t avail(const Bits &b)
{
    const uint64_t all = 8ull * b.in_len, used = used_bits(b);
    return used < all ? all - used : 0;
}
XLZ_BZ2_HD uint32_t peek(const Bits &b, uint32_t k) { return (uint32_t)(b.hold >> (64 - k)); } // 1 <= k <= 32, behind a fill
XLZ_BZ2_HD void drop(Bits &b, uint32_t k) { b.hold <<= k, b.n -= k; }
XLZ_BZ2_HD void seek(WaveA &w, Bits &b, uint32_t bit_pos)
{
    b.hold = 0, b.n = 0, b.next = (bit_pos >> 3) & ~3u;
    const uint32_t skip = bit_pos - 8 * b.next; // < 32
    load_window(w, b, b.next & ~(kWindow - 1));
    fill(w, b);
    if (skip) drop(b, skip);
}
// k <= 32 bits -> *v; false: the input ends in front of them
XLZ_BZ2_HD bool get(WaveA &w, Bits &b, uint32_t k, uint32_t *v)
{
    fill(w, b);
    if (avail(b) < k) return false;
    *v = peek(b, k);
    drop(b, k);
    return true;
}

// the tables of group t from w.len[t][0 .. alpha)
XLZ_BZ2_HD void build_group(WaveA &w, uint32_t t, uint32_t alpha)
{
    XLZ_BZ2_SYNC();
    XLZ_BZ2_LANES(lane)
    {
        if (lane <= kMaxCodeLen) {
            uint32_t c = 0;
            for (uint32_t s = 0; s < alpha && lane; s++) c += w.len[t][s] == lane;
            w.cnt[t][lane] = (uint16_t)c;
        }
    }
    XLZ_BZ2_SYNC();
    XLZ_BZ2_LANES(lane)
    {
        if (lane >= 1 && lane <= kMaxCodeLen) {
            uint32_t at = 0;
            for (uint32_t l = 1; l < lane; l++) at += w.cnt[t][l];
            for (uint32_t s = 0; s < alpha; s++)
                if (w.len[t][s] == lane) w.perm[t][at++] = (uint16_t)s; // (alpha symbols in all: inside perm[])
        }
    }
    XLZ_BZ2_SYNC();
    XLZ_BZ2_LANES(lane)
    {
        for (uint32_t e = lane; e < 1u << kFastBits; e += kLanes) {
            int code = 0, first = 0, index = 0;
            uint32_t entry = 0;
            for (uint32_t l = 1; l <= kFastBits; l++) {
                code = (code << 1) | (int)((e >> (kFastBits - l)) & 1);
                const int c = w.cnt[t][l];
                if (code - c < first) {
                    entry = (code < first ? kNoCode : (uint32_t)w.perm[t][index + (code - first)]) | l << 9;
                    break;
                }
                index += c, first = (first + c) << 1;
            }
            w.fast[t][e] = (uint16_t)entry;
        }
    }
    XLZ_BZ2_SYNC();
}
// the next symbol of group t -> *sym; else the status
XLZ_BZ2_HD int decode_symbol(WaveA &w, Bits &b, uint32_t t, uint32_t *sym)
{
    fill(w, b);
    const uint64_t have = avail(b);
    const uint32_t entry = XLZ_BZ2_UNI(w.fast[t][peek(b, kFastBits)]);
    if (entry) {
        const uint32_t l = entry >> 9;
        if (have < l) return kStEof;
        drop(b, l);
        *sym = entry & 511;
        return *sym == kNoCode ? kStResult : kStOk;
    }
    const uint32_t bits = peek(b, kMaxCodeLen + 1);
    int code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l <= kMaxCodeLen; l++) {
        if (have < l) return kStEof;
        code = (code << 1) | (int)((bits >> (kMaxCodeLen + 1 - l)) & 1);
        const int c = (int)XLZ_BZ2_UNI(w.cnt[t][l]);
        if (code - c < first) {
            if (code < first) return kStResult;
            *sym = XLZ_BZ2_UNI(w.perm[t][index + (code - first)]);
            drop(b, l);
            return kStOk;
        }
        index += c, first = (first + c) << 1;
    }
    return have < kMaxCodeLen + 1 ? kStEof : kStResult; // (a serial reader takes one more bit before it gives up)
}

XLZ_BZ2_HD void flush_pending(WaveA &w, uint8_t *ll, uint32_t nblock, uint32_t npend) // the npend bytes in front of nblock
{
    XLZ_BZ2_SYNC();
    XLZ_BZ2_LANES(lane)
    {
        if (lane < npend) ll[nblock - npend + lane] = w.pend[lane];
    }
    XLZ_BZ2_SYNC();
}

// PHASE A: the candidate's header, tables and symbols -> ll[0 .. nblock) and *st (status, nblock, orig, crc, end_bit)
XLZ_BZ2_HD void wave_symbols(WaveA &w, const DevCand &c, const uint8_t *image, uint8_t *scratch, DevState *out)
{
    DevState st = {};
    Bits b;
    b.in = image + c.in_off, b.in_len = c.in_len;
    const Scratch sc = scratch_of(scratch + c.scratch_off, c.cap);
    seek(w, b, c.start_bit);
    uint32_t v = 0, n_used = 0, n_groups = 0, n_sel = 0, alpha = 0, nblock = 0;
    int status = kStOk;
#define XLZ_BZ2_NEED(k)             \
    if (!get(w, b, (k), &v)) {      \
        status = kStEof;            \
        break;                      \
    }
#define XLZ_BZ2_FAIL(s) \
    {                   \
        status = (s);   \
        break;          \
    }
    do {
        XLZ_BZ2_NEED(24)
        if (v != (uint32_t)(kBlockMagic >> 24)) XLZ_BZ2_FAIL(kStResult)
        XLZ_BZ2_NEED(24)
        if (v != (uint32_t)(kBlockMagic & 0xFFFFFF)) XLZ_BZ2_FAIL(kStResult)
        XLZ_BZ2_NEED(32)
        st.crc = v;
        XLZ_BZ2_NEED(1)
        if (v) XLZ_BZ2_FAIL(kStUnsupported)
        XLZ_BZ2_NEED(24)
        st.orig = v;
        if (v > 10 + c.cap) XLZ_BZ2_FAIL(kStResult)
        XLZ_BZ2_NEED(16)
        const uint32_t map16 = v;
        for (uint32_t i = 0; i < 16 && status == kStOk; i++)
            if (map16 & (0x8000u >> i)) {
                if (!get(w, b, 16, &v)) {
                    status = kStEof;
                    break;
                }
                XLZ_BZ2_SYNC();
                for (uint32_t j = 0; j < 16; j++)
                    if (v & (0x8000u >> j)) w.seq[n_used++] = (uint8_t)(16 * i + j); // (every lane writes the same)
            }
        if (status != kStOk) break;
        if (!n_used) XLZ_BZ2_FAIL(kStResult)
        alpha = n_used + 2;
        XLZ_BZ2_NEED(3)
        n_groups = v;
        if (n_groups < 2 || n_groups > kMaxGroups) XLZ_BZ2_FAIL(kStResult)
        XLZ_BZ2_NEED(15)
        if (v < 1) XLZ_BZ2_FAIL(kStResult)
        const uint32_t n_sel_read = v;
        n_sel = n_sel_read < kMaxSelectors ? n_sel_read : kMaxSelectors;
        {
            uint32_t order = 0x543210; // the selectors' move-to-front list, a nibble a place
            for (uint32_t i = 0; i < n_sel_read && status == kStOk; i++) {
                uint32_t j = 0;
                for (;;) {
                    if (!get(w, b, 1, &v)) {
                        status = kStEof;
                        break;
                    }
                    if (!v) break;
                    if (++j >= n_groups) {
                        status = kStResult;
                        break;
                    }
                }
                if (status != kStOk || i >= kMaxSelectors) continue;
                const uint32_t g = (order >> (4 * j)) & 15, low = order & ((1u << (4 * j)) - 1);
                order = (order & ~((1u << (4 * j + 4)) - 1)) | low << 4 | g;
                w.sel[i] = (uint8_t)g;
            }
        }
        if (status != kStOk) break;
        for (uint32_t t = 0; t < n_groups && status == kStOk; t++) {
            if (!get(w, b, 5, &v)) {
                status = kStEof;
                break;
            }
            uint32_t curr = v;
            for (uint32_t i = 0; i < alpha && status == kStOk; i++) {
                for (;;) {
                    if (curr < 1 || curr > kMaxCodeLen) {
                        status = kStResult;
                        break;
                    }
                    if (!get(w, b, 1, &v)) {
                        status = kStEof;
                        break;
                    }
                    if (!v) break;
                    if (!get(w, b, 1, &v)) {
                        status = kStEof;
                        break;
                    }
                    curr += v ? 0xFFFFFFFFu : 1u;
                }
                w.len[t][i] = (uint8_t)curr;
            }
        }
        if (status != kStOk) break;
        for (uint32_t t = 0; t < n_groups; t++) build_group(w, t, alpha);
        XLZ_BZ2_LANES(lane) { w.mtf[0][lane] = 0x03020100u + 0x04040404u * lane; }
        XLZ_BZ2_SYNC();
        uint32_t cur = 0, group = 0, left = 0, run = 0, weight = 1, npend = 0, t = 0;
        bool in_run = false;
        const uint32_t eob = n_used + 1;
        for (;;) {
            if (!left) {
                if (group >= n_sel) XLZ_BZ2_FAIL(kStResult)
                t = XLZ_BZ2_UNI(w.sel[group]);
                left = kGroupSyms, group++;
            }
            left--;
            uint32_t sym = 0;
            status = decode_symbol(w, b, t, &sym);
            if (status != kStOk) break;
            if (sym <= 1) {
                if (!in_run) in_run = true, run = 0, weight = 1;
                if (weight >= kRunLimit) XLZ_BZ2_FAIL(kStResult)
                run += weight << sym, weight <<= 1;
                continue;
            }
            if (in_run) {
                in_run = false;
                if (run > c.cap - nblock) XLZ_BZ2_FAIL(kStResult)
                if (npend) flush_pending(w, sc.ll, nblock, npend), npend = 0;
                const uint8_t x = (uint8_t)XLZ_BZ2_UNI(w.seq[XLZ_BZ2_UNI(w.mtf[cur][0]) & 255]);
                XLZ_BZ2_LANES(lane)
                {
                    for (uint32_t k = lane; k < run; k += kLanes) sc.ll[nblock + k] = x;
                }
                nblock += run;
            }
            if (sym == eob) break;
            if (nblock >= c.cap) XLZ_BZ2_FAIL(kStResult)
            const uint32_t nn = sym - 1; // >= 1
            uint32_t place;
            if (nn < 4) { // inside the first word: no lane work
                const uint32_t w0 = XLZ_BZ2_UNI(w.mtf[cur][0]), low = 0xFFFFFFFFu >> (8 * (3 - nn)); // places 0 .. nn
                place = (w0 >> (8 * nn)) & 255;
                w.mtf[cur][0] = (w0 & ~low) | ((w0 << 8) & low) | place; // (every lane writes the same)
            } else {
                place = (XLZ_BZ2_UNI(w.mtf[cur][nn >> 2]) >> (8 * (nn & 3))) & 255;
                XLZ_BZ2_LANES(lane)
                {
                    const uint32_t mine = w.mtf[cur][lane], prev = lane ? w.mtf[cur][lane - 1] : 0;
                    const uint32_t moved = mine << 8 | (lane ? prev >> 24 : place);
                    uint32_t to = mine;
                    if (4 * lane + 3 <= nn)
                        to = moved;
                    else if (4 * lane <= nn) { // the word the place lies in: its bytes up to nn & 3 move
                        const uint32_t m = 0xFFFFFFFFu >> (8 * (3 - (nn & 3)));
                        to = (mine & ~m) | (moved & m);
                    }
                    w.mtf[cur ^ 1][lane] = to;
                }
                cur ^= 1;
                XLZ_BZ2_SYNC();
            }
            w.pend[npend++] = (uint8_t)XLZ_BZ2_UNI(w.seq[place]); // (every lane writes the same)
            nblock++;
            if (npend == kLanes) flush_pending(w, sc.ll, nblock, npend), npend = 0;
        }
        if (status != kStOk) break;
        if (npend) flush_pending(w, sc.ll, nblock, npend);
        if (st.orig >= nblock) XLZ_BZ2_FAIL(kStResult)
    } while (0);
#undef XLZ_BZ2_NEED
#undef XLZ_BZ2_FAIL
    st.status = status, st.nblock = nblock, st.end_bit = used_bits(b);
    XLZ_BZ2_LANES(lane)
    {
        if (lane == 0) *out = st;
    }
}

// LDS of phases B and C
struct WaveW {
    uint32_t count[256];
    uint32_t seg_len[kMarks + 1], seg_end[kMarks + 1], seg_off[kMarks + 1];
    uint32_t ex_len[kLanes][5];
    uint8_t ex_run[kLanes][5], ex_last[kLanes][5], first[kLanes];
    uint32_t crc_table[256], crc_part[kLanes], crc_len[kLanes];
    uint32_t slow; // a lane has used up its share of the walk
};
constexpr uint32_t kPlaced = 0x80000000u, kNoOffset = 0xFFFFFFFFu;

// a row of the counting sort: places base + lane < nblock
XLZ_BZ2_HD void sort_row(WaveW &w, const uint8_t *ll, uint32_t *tt, uint32_t base, uint32_t nblock)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t lane = threadIdx.x, i = base + lane;
    const bool active = i < nblock;
    const uint32_t byte = active ? ll[i] : 256u;
    const uint32_t at = active ? w.count[byte] : 0; // (read by the whole row before any lane of it writes)
    uint64_t todo = __ballot(active);
    uint32_t rank = 0, total = 0;
    while (todo) {
        const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
        const uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)byte, (int)leader);
        const uint64_t same = __ballot(byte == x);
        if (byte == x) rank = (uint32_t)__popcll(same & ((1ull << lane) - 1)), total = (uint32_t)__popcll(same);
        todo &= ~same;
    }
    if (active) {
        tt[at + rank] = i;
        if (rank + 1 == total) w.count[byte] = at + total;
    }
#else
    // the same, lane by lane: a ballot is a loop over the 64 lanes' values
    uint32_t byte[kLanes], at[kLanes], rank[kLanes], total[kLanes];
    uint64_t todo = 0;
    for (uint32_t lane = 0; lane < kLanes; lane++) {
        const bool active = base + lane < nblock;
        byte[lane] = active ? ll[base + lane] : 256u;
        at[lane] = active ? w.count[byte[lane]] : 0;
        rank[lane] = total[lane] = 0;
        if (active) todo |= 1ull << lane;
    }
    while (todo) {
        const uint32_t x = byte[__builtin_ctzll(todo)];
        uint64_t same = 0;
        for (uint32_t lane = 0; lane < kLanes; lane++)
            if (byte[lane] == x) same |= 1ull << lane;
        for (uint32_t lane = 0; lane < kLanes; lane++)
            if (byte[lane] == x) rank[lane] = (uint32_t)__builtin_popcountll(same & ((1ull << lane) - 1)), total[lane] = (uint32_t)__builtin_popcountll(same);
        todo &= ~same;
    }
    for (uint32_t lane = 0; lane < kLanes; lane++)
        if (base + lane < nblock) {
            tt[at[lane] + rank[lane]] = base + lane;
            if (rank[lane] + 1 == total[lane]) w.count[byte[lane]] = at[lane] + total[lane];
        }
#endif
}

// PHASES B and C: ll[0 .. nblock) -> pre[0 .. nblock), the chunks' entry states, st->out_len and st->calc_crc
XLZ_BZ2_HD void wave_walk(WaveW &w, const DevCand &c, uint8_t *scratch, DevState *io)
{
    const Scratch sc = scratch_of(scratch + c.scratch_off, c.cap);
    const uint32_t nblock = XLZ_BZ2_UNI(io->nblock), orig = XLZ_BZ2_UNI(io->orig);
    if ((int)XLZ_BZ2_UNI(io->status) != kStOk || !nblock || nblock > c.cap || orig >= nblock) return;
    // ---- B
    XLZ_BZ2_LANES(lane)
    {
        for (uint32_t k = lane; k < 256; k += kLanes) w.count[k] = 0;
    }
    XLZ_BZ2_SYNC();
    XLZ_BZ2_LANES(lane)
    {
        for (uint32_t i = lane; i < nblock; i += kLanes) XLZ_BZ2_COUNT(&w.count[sc.ll[i]]);
    }
    XLZ_BZ2_SYNC();
    {
        uint32_t sum = 0; // (every lane forms the same sums and writes the same)
        for (uint32_t k = 0; k < 256; k++) {
            const uint32_t n = XLZ_BZ2_UNI(w.count[k]);
            w.count[k] = sum;
            sum += n;
        }
    }
    XLZ_BZ2_SYNC();
    for (uint32_t base = 0; base < nblock; base += kLanes) sort_row(w, sc.ll, sc.tt, base, nblock);
    XLZ_BZ2_SYNC();
    // ---- C: the segments
    uint32_t stride = 1;
    while ((uint64_t)stride * kMarks < nblock) stride <<= 1;
    const uint32_t n_marks = (nblock + stride - 1) / stride, mask = stride - 1; // <= kMarks
    const uint32_t head = XLZ_BZ2_UNI(sc.tt[orig]);
    const uint32_t head_seg = (head & mask) ? kMarks : head / stride;
    XLZ_BZ2_LANES(lane)
    {
        for (uint32_t s = lane; s <= kMarks; s += kLanes) w.seg_off[s] = kNoOffset, w.seg_len[s] = 0, w.seg_end[s] = 0;
        if (lane == 0) w.slow = 0;
    }
    XLZ_BZ2_SYNC();
    const uint32_t share = nblock / kWalkShare + kWalkSlack; // places a lane walks at most, over all its segments
    XLZ_BZ2_LANES(lane)
    {
        uint32_t walked = 0;
        for (uint32_t s = lane; s <= kMarks && walked < share; s += kLanes) {
            if (s < kMarks ? s >= n_marks : head_seg != kMarks) continue;
            uint32_t p = s < kMarks ? s * stride : head, k = 0;
            do {
                const uint32_t next = sc.tt[p]; // < nblock: the sort wrote it
                sc.tt[p] = kPlaced | s << 20 | k;
                k++, p = next;
            } while ((p & mask) && p != head && k < nblock && walked + k < share);
            walked += k;
            w.seg_len[s] = k, w.seg_end[s] = p;
        }
        if (walked >= share) w.slow = 1; // (whichever lanes write it, they write the same)
    }
    XLZ_BZ2_SYNC();
    if (XLZ_BZ2_UNI(w.slow)) { // the marks were avoided: not the device's block
        XLZ_BZ2_LANES(lane)
        {
            if (lane == 0) io->status = kStSlow;
        }
        return;
    }
    uint32_t cycle = 0;
    for (uint32_t s = head_seg, turns = 0; turns <= kMarks; turns++) { // (every lane the same)
        if (XLZ_BZ2_UNI(w.seg_off[s]) != kNoOffset) break;
        const uint32_t len = XLZ_BZ2_UNI(w.seg_len[s]), end = XLZ_BZ2_UNI(w.seg_end[s]);
        w.seg_off[s] = cycle;
        cycle += len;
        if (cycle >= nblock) break;
        s = end == head ? head_seg : end / stride;
    }
    XLZ_BZ2_SYNC();
    if (!cycle || cycle > nblock) cycle = nblock; // (cannot be: the segments of one cycle are disjoint)
    XLZ_BZ2_LANES(lane)
    {
        for (uint32_t p = lane; p < nblock; p += kLanes) {
            const uint32_t v = sc.tt[p];
            if (!(v & kPlaced)) continue; // on a cycle without a mark
            const uint32_t off = w.seg_off[(v >> 20) & 2047];
            if (off == kNoOffset) continue; // on a cycle that is not the head's
            const uint32_t at = off + (v & 0xFFFFF);
            if (at < nblock) sc.pre[at] = sc.ll[p];
        }
    }
    XLZ_BZ2_SYNC();
    if (cycle < nblock) {
        XLZ_BZ2_LANES(lane)
        {
            for (uint32_t j = cycle + lane; j < nblock; j += kLanes) sc.pre[j] = sc.pre[j % cycle];
        }
        XLZ_BZ2_SYNC();
    }
    // ---- the run-length code, measured: lane's chunk from each of the five entry states
    const uint32_t chunk = (nblock + kLanes - 1) / kLanes;
    XLZ_BZ2_LANES(lane)
    {
        const uint32_t from = lane * chunk < nblock ? lane * chunk : nblock, to = from + chunk < nblock ? from + chunk : nblock;
        uint32_t run[5] = {0, 1, 2, 3, 4}, last[5], len[5] = {0, 0, 0, 0, 0};
        const uint32_t x0 = from < to ? sc.pre[from] : 0;
        for (int e = 0; e < 5; e++) last[e] = x0;
        for (uint32_t i = from; i < to; i++) {
            const uint32_t x = sc.pre[i];
            for (int e = 0; e < 5; e++) {
                if (run[e] == 4)
                    len[e] += x, run[e] = 0;
                else if (run[e] && x == last[e])
                    run[e]++, len[e]++;
                else
                    last[e] = x, run[e] = 1, len[e]++;
            }
        }
        w.first[lane] = (uint8_t)x0;
        for (int e = 0; e < 5; e++) w.ex_len[lane][e] = len[e], w.ex_run[lane][e] = (uint8_t)run[e], w.ex_last[lane][e] = (uint8_t)last[e];
    }
    XLZ_BZ2_SYNC();
    XLZ_BZ2_LANES(lane)
    {
        if (lane == 0) {
            uint32_t run = 0, last = 0, off = 0;
            for (uint32_t k = 0; k < kLanes; k++) {
                sc.chunks[k] = DevChunk{off, run, last, 0};
                if (k * chunk >= nblock) continue;
                const uint32_t e = run == 4 ? 4 : (run && last == w.first[k]) ? run : 0;
                off += w.ex_len[k][e];
                run = w.ex_run[k][e], last = w.ex_last[k][e]; // (behind a count run is 0, and `last` then decides nothing)
            }
            io->out_len = off;
        }
    }
    // ---- and its CRC, so that the verdict is known before a byte is written: lane's chunk once more, from the state it is
    // entered in, the bytes it expands to going through the CRC instead of to memory; the 64 parts are folded by their lengths
    XLZ_BZ2_LANES(lane)
    {
        for (uint32_t k = lane; k < 256; k += kLanes) w.crc_table[k] = crc_entry(k);
    }
    XLZ_BZ2_SYNC();
    XLZ_BZ2_LANES(lane)
    {
        const uint32_t from = lane * chunk < nblock ? lane * chunk : nblock, to = from + chunk < nblock ? from + chunk : nblock;
        const DevChunk in = sc.chunks[lane];
        uint32_t run = in.run, last = in.last, n = 0, r = lane ? 0 : 0xFFFFFFFFu;
        for (uint32_t i = from; i < to; i++) {
            const uint32_t x = sc.pre[i];
            if (run == 4) {
                for (uint32_t k = 0; k < x; k++) r = (r << 8) ^ w.crc_table[(r >> 24) ^ last];
                n += x, run = 0;
            } else {
                if (run && x == last)
                    run++;
                else
                    last = x, run = 1;
                r = (r << 8) ^ w.crc_table[(r >> 24) ^ x];
                n++;
            }
        }
        w.crc_part[lane] = r, w.crc_len[lane] = n;
    }
    XLZ_BZ2_SYNC();
    XLZ_BZ2_LANES(lane)
    {
        if (lane == 0) {
            uint32_t r = w.crc_part[0];
            for (uint32_t k = 1; k < kLanes; k++)
                if (w.crc_len[k]) r = gf_mul(r, gf_xpow(8ull * w.crc_len[k])) ^ w.crc_part[k];
            io->calc_crc = ~r;
        }
    }
}

// PHASE D: chunk `lane` of pre[] -> dst[0 .. out_len)
XLZ_BZ2_HD void wave_expand(const DevCand &c, uint8_t *scratch, const DevState &st, uint8_t *dst, uint32_t out_len)
{
    const Scratch sc = scratch_of(scratch + c.scratch_off, c.cap);
    const uint32_t nblock = st.nblock, chunk = (nblock + kLanes - 1) / kLanes;
    XLZ_BZ2_LANES(lane)
    {
        const uint32_t from = lane * chunk < nblock ? lane * chunk : nblock, to = from + chunk < nblock ? from + chunk : nblock;
        const DevChunk in = sc.chunks[lane];
        uint32_t run = in.run, last = in.last, at = in.out_off;
        for (uint32_t i = from; i < to; i++) {
            const uint32_t x = sc.pre[i];
            if (run == 4) {
                for (uint32_t k = 0; k < x && at < out_len; k++) dst[at++] = (uint8_t)last;
                run = 0;
            } else {
                if (run && x == last)
                    run++;
                else
                    last = x, run = 1;
                if (at < out_len) dst[at++] = (uint8_t)x;
            }
        }
    }
}

// the CRC of p[0 .. len): 64 partial ones, folded.  table: 256 entries in LDS; part: kLanes entries
XLZ_BZ2_HD uint32_t wave_crc(uint32_t *table, uint32_t *part, const uint8_t *p, uint32_t len)
{
    XLZ_BZ2_SYNC();
    XLZ_BZ2_LANES(lane)
    {
        for (uint32_t k = lane; k < 256; k += kLanes) table[k] = crc_entry(k);
    }
    XLZ_BZ2_SYNC();
    const uint32_t chunk = (len + kLanes - 1) / kLanes;
    XLZ_BZ2_LANES(lane)
    {
        const uint32_t from = lane * chunk < len ? lane * chunk : len, to = from + chunk < len ? from + chunk : len;
        uint32_t r = lane ? 0 : 0xFFFFFFFFu;
        for (uint32_t i = from; i < to; i++) r = (r << 8) ^ table[(r >> 24) ^ p[i]];
        part[lane] = r;
    }
    XLZ_BZ2_SYNC();
    uint32_t r = XLZ_BZ2_UNI(part[0]);
    if (len > chunk) {
        const uint32_t whole = gf_xpow(8ull * chunk);
        for (uint32_t k = 1; k < kLanes && k * chunk < len; k++) {
            const uint32_t n = (k + 1) * chunk <= len ? chunk : len - k * chunk;
            r = gf_mul(r, n == chunk ? whole : gf_xpow(8ull * n)) ^ XLZ_BZ2_UNI(part[k]);
        }
    }
    return ~r;
}

} // namespace xlzbz2
