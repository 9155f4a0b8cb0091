// xlz_filter_dev.h -- the .xz / .7z filters that sit in front of an LZMA coder (Delta and the BCJ branch converters for
// x86, PowerPC, IA-64, ARM, ARM-Thumb and SPARC), decoder side, in a form that compiles both as device code
// (xlz_filter_dev.hip) and as plain C++: a g++ program runs the per-lane / per-window / per-chunk scheme on the CPU
// (tests/c/filter_dev_selftest.cpp), and host_apply() below is the serial twin the library exports as xlz_filter_host.
// Written from the published format descriptions ("The .xz File Format" 5.3; the branch/call/jump converters are
// described with 7-Zip's format notes); the reference has no filters.
//
// A STEP transforms [0, len) of one stream in place.  Positions are relative to the stream's first byte; the address a
// BCJ filter subtracts is start offset + position, 32 bits, wrapping.
//
//  * ARM, PowerPC, SPARC (4-byte words), IA-64 (16-byte bundles): every aligned slot converts by itself.  A lane takes the
//    sixteen bytes at a multiple of 16 (chunk16); a tail shorter than a slot stays as it is.
//  * ARM-Thumb: a BL is a pair of halfwords at 2-byte alignment, the first with the top bits 11110, the second 11111.  A
//    halfword cannot be both, so candidate pairs never overlap, and the conversion keeps those top bits: whether a
//    position converts can be read off the bytes at any time.  A pair belongs to the lane that holds its FIRST halfword.
//    The pair that starts in a lane's last halfword ends in the next lane's first one: the owner stores that halfword by
//    itself (its value is the original: the next lane never converts a second half), and the next lane keeps its hands
//    off it (thumb_chunk16: skip_first) -- so no byte is written by two lanes.
//  * x86 is a serial state machine (prev_mask, prev_pos), but its state is the fresh one at every position that follows
//    kX86Clean bytes without an E8 / E9 (a SYNC POINT; position 0 is one).  A first pass notes, on the ORIGINAL bytes, the
//    first sync point of every window of kX86Window bytes (x86_first_sync); a second pass has lane j run the serial
//    decoder from the first sync point at or after j * kX86Window to the first one at or after (j + 1) * kX86Window
//    (x86_walk).  Lanes write disjoint bytes: no conversion straddles a sync point.
//  * Delta, out[i] = in[i] + out[i - d], is a prefix sum per residue class mod d.  The stream is cut into chunks of
//    kDeltaChunk bytes held in LDS as words: pass 1 folds a chunk onto its first d bytes (delta_fold_word: halve the
//    length at multiples of d), which are its column sums; pass 2 turns the sums of a stream's chunks into exclusive
//    prefixes, in two levels so that a stream of a GiB (65 536 chunks) is no serial walk: inside groups of kDeltaGroup
//    chunks (delta_group_scan, one workgroup per group), then over the groups' totals (delta_groups_scan); pass 3 adds a
//    chunk's carried-in sums (delta_carry) to its first d bytes and scans it by doubling (delta_scan_word:
//    x[i] += x[i - s], s = d, 2d, 4d, ...).  Bytes are added four at a time inside a word (add_bytes).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define XLZ_FLT_HD __host__ __device__ inline
#else
#define XLZ_FLT_HD inline
#endif

namespace xlzflt {

enum : uint32_t { kDelta = 3, kX86 = 4, kPowerPC = 5, kIA64 = 6, kARM = 7, kARMThumb = 8, kSPARC = 9 }; // the .xz filter ids

constexpr uint32_t kLaneBytes = 16;
constexpr uint32_t kBcjTileBytes = 16384;  // one workgroup: 256 lanes x 4 chunks of 16 bytes
constexpr uint32_t kX86Window = 256;       // one lane's share of an x86 step
constexpr uint32_t kX86Clean = 9;          // bytes without E8 / E9 in front of a sync point
constexpr uint32_t kX86TileWindows = 256;  // one workgroup
constexpr uint16_t kNoSync = 0xFFFF;
constexpr uint32_t kDeltaChunk = 16384;    // bytes of one Delta chunk (LDS of one workgroup)
constexpr uint32_t kDeltaWords = kDeltaChunk / 4;
constexpr uint32_t kDeltaThreads = 256;
constexpr uint32_t kDeltaMaxDist = 256;
constexpr uint32_t kDeltaGroup = 256;      // chunks whose sums one workgroup of the second pass scans

// alignment of a filter's slots = what its start offset must be a multiple of; 0: not a filter id
XLZ_FLT_HD uint32_t alignment(uint32_t id)
{
    switch (id) {
    case kDelta: case kX86: return 1;
    case kARMThumb: return 2;
    case kPowerPC: case kARM: case kSPARC: return 4;
    case kIA64: return 16;
    default: return 0;
    }
}
// 0 when (id, param) is a step this code runs
XLZ_FLT_HD int bad_step(uint32_t id, uint32_t param)
{
    const uint32_t a = alignment(id);
    if (!a) return 1;
    if (id == kDelta) return param < 1 || param > kDeltaMaxDist;
    return (param & (a - 1)) != 0;
}

XLZ_FLT_HD uint32_t bswap32(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24); }

// ---- the fixed-width converters: one slot, `ip` = the address of the slot's first byte ----
XLZ_FLT_HD uint32_t arm_word(uint32_t w, uint32_t ip) // BL: cond = always (0xEB), 24-bit word offset from pc + 8
{
    if ((w >> 24) != 0xEB) return w;
    const uint32_t dest = (((w & 0xFFFFFFu) << 2) - (ip + 8)) >> 2;
    return 0xEB000000u | (dest & 0xFFFFFFu);
}
XLZ_FLT_HD uint32_t ppc_word(uint32_t w, uint32_t ip) // big endian: bl = 010010 .. AA = 0, LK = 1
{
    const uint32_t v = bswap32(w);
    if ((v & 0xFC000003u) != 0x48000001u) return w;
    const uint32_t dest = (v & 0x03FFFFFCu) - ip;
    return bswap32(0x48000001u | (dest & 0x03FFFFFCu));
}
XLZ_FLT_HD uint32_t sparc_word(uint32_t w, uint32_t ip) // big endian: call, 30-bit word displacement whose top bits are sign bits
{
    const uint32_t v = bswap32(w), b0 = v >> 24, t = (v >> 22) & 3;
    if (!((b0 == 0x40 && t == 0) || (b0 == 0x7F && t == 3))) return w;
    uint32_t dest = ((v << 2) - ip) >> 2;
    dest = (((0u - ((dest >> 22) & 1)) << 22) & 0x3FFFFFFFu) | (dest & 0x3FFFFFu) | 0x40000000u;
    return bswap32(dest);
}
// the slots of an IA-64 bundle that can hold a branch, by the bundle's template (its low five bits)
XLZ_FLT_HD uint32_t ia64_slots(uint32_t tmpl)
{
    switch (tmpl >> 1) {
    case 8: case 12: case 14: return 4; // MIB, MMB, MFB
    case 9: return 6;                   // MBB
    case 11: return 7;                  // BBB
    default: return 0;
    }
}
XLZ_FLT_HD uint64_t ia64_slot(uint64_t instruction, uint32_t bit_res, uint32_t ip) // the 48 bits that hold one 41-bit slot
{
    uint64_t norm = instruction >> bit_res;
    if (((norm >> 37) & 0xF) != 0x5 || ((norm >> 9) & 0x7) != 0) return instruction;
    uint32_t src = (uint32_t)((norm >> 13) & 0xFFFFF);
    src |= ((uint32_t)(norm >> 36) & 1) << 20;
    src <<= 4;
    const uint32_t dest = (src - ip) >> 4;
    norm &= ~((uint64_t)0x8FFFFF << 13);
    norm |= (uint64_t)(dest & 0xFFFFF) << 13;
    norm |= (uint64_t)(dest & 0x100000) << (36 - 20);
    return (instruction & ((1ull << bit_res) - 1)) | (norm << bit_res);
}
XLZ_FLT_HD void ia64_bundle(uint32_t w[4], uint32_t ip)
{
    const uint32_t mask = ia64_slots(w[0] & 0x1F);
    if (!mask) return;
    uint64_t lo = (uint64_t)w[0] | (uint64_t)w[1] << 32, hi = (uint64_t)w[2] | (uint64_t)w[3] << 32;
    const uint64_t m48 = (1ull << 48) - 1;
    if (mask & 1) { // bits 5 .. 45: bytes 0 .. 5
        const uint64_t v = ia64_slot(lo & m48, 5, ip);
        lo = (lo & ~m48) | (v & m48);
    }
    if (mask & 2) { // bits 46 .. 86: bytes 5 .. 10
        const uint64_t v = ia64_slot(((lo >> 40) | (hi << 24)) & m48, 6, ip);
        lo = (lo & ((1ull << 40) - 1)) | (v << 40);
        hi = (hi & ~((1ull << 24) - 1)) | ((v & m48) >> 24);
    }
    if (mask & 4) { // bits 87 .. 127: bytes 10 .. 15
        const uint64_t v = ia64_slot(hi >> 16, 7, ip);
        hi = (hi & 0xFFFF) | (v << 16);
    }
    w[0] = (uint32_t)lo, w[1] = (uint32_t)(lo >> 32), w[2] = (uint32_t)hi, w[3] = (uint32_t)(hi >> 32);
}
XLZ_FLT_HD bool thumb_first(uint32_t h) { return (h & 0xF800u) == 0xF000u; }
XLZ_FLT_HD bool thumb_second(uint32_t h) { return (h & 0xF800u) == 0xF800u; }
// the pair (h0, h1) is a BL (thumb_first(h0) && thumb_second(h1)); ip = the address of h0
XLZ_FLT_HD void thumb_pair(uint32_t &h0, uint32_t &h1, uint32_t ip)
{
    const uint32_t src = (((h0 & 0x7FFu) << 11) | (h1 & 0x7FFu)) << 1;
    const uint32_t dest = (src - (ip + 4)) >> 1;
    h0 = 0xF000u | ((dest >> 11) & 0x7FFu);
    h1 = 0xF800u | (dest & 0x7FFu);
}

// One lane's sixteen bytes of an ARM / PowerPC / SPARC / IA-64 step; ip = the address of w[0]; `whole`: bytes of the chunk
// inside the stream (16, or fewer in the stream's last chunk: only whole slots convert)
XLZ_FLT_HD void bcj_chunk16(uint32_t id, uint32_t ip, uint32_t w[4], uint32_t whole)
{
    if (id == kIA64) {
        if (whole >= 16) ia64_bundle(w, ip);
        return;
    }
    for (uint32_t k = 0; k < 4; k++) {
        if (4 * k + 4 > whole) break;
        w[k] = id == kARM ? arm_word(w[k], ip + 4 * k) : id == kPowerPC ? ppc_word(w[k], ip + 4 * k) : sparc_word(w[k], ip + 4 * k);
    }
}
// One lane's sixteen bytes of an ARM-Thumb step.  prev_h: the halfword in front of the chunk (only its top five bits are
// looked at; anything that is not a first half when the chunk starts the stream), next_h: the halfword behind it, valid
// when `whole` >= 18 = bytes of the stream from the chunk's start.  -> bit 0: the lane must not store its first halfword
// (it is the second half of the previous lane's pair); bit 1: the lane stores *next_out behind its chunk.
XLZ_FLT_HD uint32_t thumb_chunk16(uint32_t ip, uint32_t w[4], uint32_t whole, uint32_t prev_h, uint32_t next_h, uint32_t *next_out)
{
    uint32_t h[9];
    for (uint32_t k = 0; k < 4; k++) h[2 * k] = w[k] & 0xFFFFu, h[2 * k + 1] = w[k] >> 16;
    h[8] = next_h;
    uint32_t flags = (thumb_first(prev_h) && whole >= 2 && thumb_second(h[0])) ? 1u : 0u;
    for (uint32_t k = 0; k < 8; k++) {
        if (2 * k + 4 > whole) break;
        if (thumb_first(h[k]) && thumb_second(h[k + 1])) {
            thumb_pair(h[k], h[k + 1], ip + 2 * k);
            if (k == 7) flags |= 2;
        }
    }
    for (uint32_t k = 0; k < 4; k++) w[k] = h[2 * k] | h[2 * k + 1] << 16;
    *next_out = h[8];
    return flags;
}

// ---- x86 ----
XLZ_FLT_HD bool x86_op(uint32_t b) { return (b & 0xFE) == 0xE8; }
XLZ_FLT_HD bool x86_msb(uint32_t b) { return b == 0 || b == 0xFF; }
// 0x80 in every byte of w that is E8 or E9 (exact: no carries between the bytes)
XLZ_FLT_HD uint32_t x86_opmask(uint32_t w)
{
    const uint32_t x = (w & 0xFEFEFEFEu) ^ 0xE8E8E8E8u; // a zero byte where an opcode is
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
}
XLZ_FLT_HD uint32_t ctz32(uint32_t m)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__ffs((int)m) - 1;
#else
    return (uint32_t)__builtin_ctz(m);
#endif
}
// the first position in [i, end) that holds E8 / E9, or end
XLZ_FLT_HD uint64_t x86_next_op(const uint8_t *buf, uint64_t i, uint64_t end)
{
    while (i < end && ((uintptr_t)(buf + i) & 15)) {
        if (x86_op(buf[i])) return i;
        i++;
    }
    while (i + 16 <= end) {
        uint32_t w0, w1, w2, w3;
#if defined(__HIP_DEVICE_COMPILE__)
        const uint4 v = *reinterpret_cast<const uint4 *>(buf + i);
        w0 = v.x, w1 = v.y, w2 = v.z, w3 = v.w;
#else
        memcpy(&w0, buf + i, 4), memcpy(&w1, buf + i + 4, 4), memcpy(&w2, buf + i + 8, 4), memcpy(&w3, buf + i + 12, 4);
#endif
        const uint32_t m0 = x86_opmask(w0), m1 = x86_opmask(w1), m2 = x86_opmask(w2), m3 = x86_opmask(w3);
        if (m0) return i + (ctz32(m0) >> 3);
        if (m1) return i + 4 + (ctz32(m1) >> 3);
        if (m2) return i + 8 + (ctz32(m2) >> 3);
        if (m3) return i + 12 + (ctz32(m3) >> 3);
        i += 16;
    }
    while (i < end) {
        if (x86_op(buf[i])) return i;
        i++;
    }
    return end;
}
// The serial decoder over [from, to) of a stream of `len` bytes, entered with the fresh state: `from` is a sync point (or
// 0), `to` a sync point or len.  The last four bytes of the STREAM never convert.
XLZ_FLT_HD void x86_walk(uint8_t *buf, uint64_t len, uint32_t start_offset, uint64_t from, uint64_t to)
{
    if (len < 5) return;
    const uint64_t stop = to < len - 4 ? to : len - 4;
    uint32_t prev_mask = 0;
    uint64_t prev_pos = 0;
    bool far = true; // no opcode examined yet: the distance to the last one is "more than five"
    uint64_t i = from;
    for (;;) {
        i = x86_next_op(buf, i, stop);
        if (i >= stop) break;
        const uint64_t off = far ? 6 : i - prev_pos;
        far = false;
        prev_pos = i;
        if (off > 5) {
            prev_mask = 0;
        } else {
            for (uint32_t j = 0; j < (uint32_t)off; j++) prev_mask = (prev_mask & 0x77) << 1;
        }
        const uint32_t b4 = buf[i + 4];
        if (x86_msb(b4) && ((0x17u >> ((prev_mask >> 1) & 7)) & 1) && (prev_mask >> 1) < 0x10) {
            uint32_t src = (uint32_t)buf[i + 1] | (uint32_t)buf[i + 2] << 8 | (uint32_t)buf[i + 3] << 16 | b4 << 24;
            uint32_t dest;
            for (;;) {
                dest = src - (start_offset + (uint32_t)i + 5);
                if (prev_mask == 0) break;
                const uint32_t k = prev_mask >> 1;           // 1, 2 or 4 here (bit 0 of prev_mask is clear after a shift)
                const uint32_t bit = k >= 4 ? 3 : k;         // the byte of the operand the earlier opcode byte fell on
                const uint32_t b = (dest >> (24 - bit * 8)) & 0xFF;
                if (!x86_msb(b)) break;
                src = dest ^ ((1u << (32 - bit * 8)) - 1);
            }
            dest &= 0x01FFFFFFu;
            dest |= 0u - (dest & 0x01000000u);
            buf[i + 1] = (uint8_t)dest, buf[i + 2] = (uint8_t)(dest >> 8), buf[i + 3] = (uint8_t)(dest >> 16), buf[i + 4] = (uint8_t)(dest >> 24);
            i += 5;
            prev_mask = 0;
        } else {
            i++;
            prev_mask |= 1;
            if (x86_msb(b4)) prev_mask |= 0x10;
        }
    }
}
// window j of the stream: its first sync point, relative to the window's start, or kNoSync
XLZ_FLT_HD uint16_t x86_first_sync(const uint8_t *buf, uint64_t len, uint64_t j)
{
    if (j == 0) return 0;
    const uint64_t lo = j * kX86Window, hi = lo + kX86Window < len ? lo + kX86Window : len;
    uint32_t clean = 0;
    for (uint64_t p = lo - kX86Clean; p < hi; p++) {
        if (p >= lo && clean >= kX86Clean) return (uint16_t)(p - lo);
        clean = x86_op(buf[p]) ? 0 : clean + 1;
    }
    return kNoSync;
}
// lane j of the second pass; sync[]: the stream's window table, n_win = its windows
XLZ_FLT_HD void x86_lane(uint8_t *buf, uint64_t len, uint32_t start_offset, const uint16_t *sync, uint64_t n_win, uint64_t j)
{
    const uint16_t fs = sync[j];
    if (fs == kNoSync) return; // (the lane in front runs through this window)
    uint64_t k = j + 1;
    while (k < n_win && sync[k] == kNoSync) k++;
    x86_walk(buf, len, start_offset, j * kX86Window + fs, k < n_win ? k * kX86Window + sync[k] : len);
}
XLZ_FLT_HD uint64_t x86_windows(uint64_t len) { return (len + kX86Window - 1) / kX86Window; }

// ---- Delta ----
XLZ_FLT_HD uint32_t add_bytes(uint32_t a, uint32_t b) { return ((a & 0x7F7F7F7Fu) + (b & 0x7F7F7F7Fu)) ^ ((a ^ b) & 0x80808080u); }
// the four bytes at byte index a (any sign, any alignment) of the chunk x[kDeltaWords]; bytes outside it read as zero
XLZ_FLT_HD uint32_t delta_bytes_at(const uint32_t *x, int32_t a)
{
    const int32_t wi = a >> 2;
    const uint32_t sh = (uint32_t)a & 3;
    const uint32_t lo = (wi >= 0 && wi < (int32_t)kDeltaWords) ? x[wi] : 0;
    if (!sh) return lo;
    const uint32_t hi = (wi + 1 >= 0 && wi + 1 < (int32_t)kDeltaWords) ? x[wi + 1] : 0;
    return (lo >> (8 * sh)) | (hi << (32 - 8 * sh));
}
// the largest d * 2^k below n (n > d)
XLZ_FLT_HD uint32_t delta_fold_at(uint32_t n, uint32_t d)
{
    uint32_t h = d;
    while (2 * h < n) h *= 2;
    return h;
}
// one fold of a chunk of n bytes at h: x[i - h] += x[i] for i in [h, n); -> the new value of word j (j < words of n - h)
XLZ_FLT_HD uint32_t delta_fold_word(const uint32_t *x, uint32_t n, uint32_t h, uint32_t j)
{
    const uint32_t a = 4 * j + h;
    uint32_t v = delta_bytes_at(x, (int32_t)a);
    if (n - a < 4) v &= (1u << (8 * (n - a))) - 1;
    return add_bytes(x[j], v);
}
// one doubling step of the scan: x[i] += x[i - s]; -> the new value of word j
XLZ_FLT_HD uint32_t delta_scan_word(const uint32_t *x, uint32_t s, uint32_t j)
{
    if (4 * j + 3 < s) return x[j];
    return add_bytes(x[j], delta_bytes_at(x, (int32_t)(4 * j) - (int32_t)s));
}
XLZ_FLT_HD uint64_t delta_chunks(uint64_t len) { return (len + kDeltaChunk - 1) / kDeltaChunk; }
XLZ_FLT_HD uint64_t delta_groups(uint64_t chunks) { return (chunks + kDeltaGroup - 1) / kDeltaGroup; }
// Second pass, thread r (< d) of group gi's workgroup.  rows: the stream's rows of sums (kDeltaMaxDist bytes per chunk; the
// last chunk's row was never written and counts as zero); every row of the group becomes the sum of the group's rows in
// front of it, the group's total goes to grow[r].
XLZ_FLT_HD void delta_group_scan(uint8_t *rows, uint8_t *grow, uint32_t n_chunks, uint32_t gi, uint32_t r)
{
    const uint32_t lo = gi * kDeltaGroup, hi = lo + kDeltaGroup < n_chunks ? lo + kDeltaGroup : n_chunks;
    uint8_t *col = rows + r;
    uint32_t acc = 0, c = lo;
    for (; c + 8 <= hi && c + 8 <= n_chunks - 1; c += 8) { // (eight loads in flight)
        uint32_t a[8];
        for (uint32_t k = 0; k < 8; k++) a[k] = col[(uint64_t)(c + k) * kDeltaMaxDist];
        for (uint32_t k = 0; k < 8; k++) {
            col[(uint64_t)(c + k) * kDeltaMaxDist] = (uint8_t)acc;
            acc += a[k];
        }
    }
    for (; c < hi; c++) {
        const uint32_t a = c < n_chunks - 1 ? col[(uint64_t)c * kDeltaMaxDist] : 0u;
        col[(uint64_t)c * kDeltaMaxDist] = (uint8_t)acc;
        acc += a;
    }
    grow[r] = (uint8_t)acc;
}
// ... and thread r of the stream's workgroup over its n_groups rows of group totals: exclusive prefixes in place
XLZ_FLT_HD void delta_groups_scan(uint8_t *grows, uint32_t n_groups, uint32_t r)
{
    uint8_t *col = grows + r;
    uint32_t acc = 0;
    for (uint32_t g = 0; g < n_groups; g++) {
        const uint32_t a = col[(uint64_t)g * kDeltaMaxDist];
        col[(uint64_t)g * kDeltaMaxDist] = (uint8_t)acc;
        acc += a;
    }
}
// what chunk c carries in for residue `res`
XLZ_FLT_HD uint32_t delta_carry(const uint8_t *rows, const uint8_t *grows, uint32_t c, uint32_t res)
{
    return (uint32_t)rows[(uint64_t)c * kDeltaMaxDist + res] + grows[(uint64_t)(c / kDeltaGroup) * kDeltaMaxDist + res];
}

// ---- the serial twin: what xlz_filter_host runs, and what the lane schemes are compared with ----
inline void host_apply(uint32_t id, uint32_t param, uint8_t *buf, uint64_t len)
{
    if (id == kDelta) {
        for (uint64_t i = param; i < len; i++) buf[i] = (uint8_t)(buf[i] + buf[i - param]);
    } else if (id == kX86) {
        x86_walk(buf, len, param, 0, len);
    } else if (id == kARMThumb) {
        for (uint64_t i = 0; i + 4 <= len; i += 2) {
            uint32_t h0 = (uint32_t)buf[i] | (uint32_t)buf[i + 1] << 8, h1 = (uint32_t)buf[i + 2] | (uint32_t)buf[i + 3] << 8;
            if (!thumb_first(h0) || !thumb_second(h1)) continue;
            thumb_pair(h0, h1, param + (uint32_t)i);
            buf[i] = (uint8_t)h0, buf[i + 1] = (uint8_t)(h0 >> 8), buf[i + 2] = (uint8_t)h1, buf[i + 3] = (uint8_t)(h1 >> 8);
            i += 2;
        }
    } else {
        for (uint64_t i = 0; i < len; i += 16) {
            uint32_t w[4] = {0, 0, 0, 0};
            const uint32_t whole = len - i < 16 ? (uint32_t)(len - i) : 16u;
            memcpy(w, buf + i, whole);
            bcj_chunk16(id, param + (uint32_t)i, w, whole);
            memcpy(buf + i, w, whole);
        }
    }
}

// one step as the device sees it (tables are sorted by `first`)
struct DevStep {
    uint64_t off, len; // bytes of the arena, len > 0
    uint64_t aux;      // x86: the stream's first entry of the window table; Delta: its first chunk's row of sums
    uint64_t aux2;     // Delta: its first group's row of totals (ascends with `first`)
    uint32_t id, param;
    uint32_t first;    // index of its first tile in the launch (BCJ: kBcjTileBytes; x86: kX86TileWindows windows; Delta: chunks)
    uint32_t n_tiles;
};

} // namespace xlzflt
