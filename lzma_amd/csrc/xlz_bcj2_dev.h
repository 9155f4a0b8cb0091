// xlz_bcj2_dev.h -- the BCJ2 merge of a .7z folder (xlz_bcj2_dev.hip), in a form that compiles both as device code and as
// plain C++: a g++ program runs the wave scheme lane by lane on the CPU (tests/c/bcj2_dev_selftest.cpp), and host_merge()
// below is the serial twin the library exports as xlz_bcj2_host.  The reference has no container code and no filters.
//
// BCJ2 (7-Zip method 03 03 01 1B) is no in-place filter: the encoder took the operands of the x86 CALL (E8), JMP (E9) and
// Jcc (0F 8x) instructions it chose to convert OUT of the byte stream, into two streams of their own (call, jump; four
// bytes big-endian each, made absolute), and wrote one range-coded bit per candidate opcode into a fourth stream (rc).  The
// decoder interleaves them again, so its output is longer than the main stream.  Stated after 7-Zip 9.20's Bcj2_Decode:
//   IsJ(prev, b) = (b & 0xFE) == 0xE8 || (prev == 0x0F && (b & 0xF0) == 0x80)
//   range coder: LZMA's (11-bit probabilities from 1024, move 5 bits, top 1 << 24), normalised AFTER every bit; 258
//   probabilities: [prev] for E8, [256] for E9, [257] for 0F 8x
//   loop: copy main bytes (prev = b after each) up to and including one with IsJ(prev, b); out of main bytes or of room:
//   stop; the candidate was the last output byte: stop (no bit).  Bit 0: prev = b.  Bit 1: src = the next four bytes of
//   call (E8) or jump, big-endian; dest = src - (uint32)(outPos + 4), written little-endian as far as there is room;
//   prev = dest >> 24.  OK iff the output is full in the end; a call / jump / rc stream that runs out is an error.
// The byte behind a converted operand is tested with prev = dest >> 24: a scan of the main stream alone does not see the
// candidate 8x behind an operand whose top byte is 0F.
//
// THE WAVE SCHEME.  One 64-lane workgroup per item walks the main stream in WINDOWS of 64 x 16 bytes:
//   load    lane l loads the aligned sixteen bytes l of the window into LDS;
//   mark    lane l tests its sixteen bytes against their predecessors in the main stream (the window's first byte against
//           the carried prev) and leaves a 16-bit mask of candidates;
//   decide  lane 0 alone walks the marked positions in order: bit, operand, dest -- written into the window's output image
//           in LDS --, the count of conversions in front of every lane's bytes, and the re-test of the byte behind a
//           conversion, which may ADD a candidate (never remove one: the byte in front of it is E8 / E9 / 8x, not 0F).
//           The rc, call and jump streams are read through sixteen-byte lines (one aligned load per line);
//   place   lane l moves its bytes into the output image, at window position + 4 x conversions in front of it;
//   store   the image goes to the destination: single bytes up to the destination's next 16-byte boundary, aligned
//           16-byte stores built from the image by a byte shift, single bytes for the tail.  Every byte has one writer,
//           nothing outside [dst, dst + out_len) is written.
// prev, the output position and the coder's state carry across windows.  Every stream pointer is a multiple of 16 and its
// allocation reaches the next multiple of 16 behind its length (the output arena's regions and the upload of
// xlz_batch_bcj2 see to that): loads are whole aligned lines, and no byte at or behind a stream's length is ever used.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define XLZ_BCJ2_HD __host__ __device__ inline
#else
#define XLZ_BCJ2_HD inline
#endif

namespace xlzbcj2 {

constexpr uint32_t kLanes = 64;
constexpr uint32_t kLaneBytes = 16;
constexpr uint32_t kWindow = kLanes * kLaneBytes; // main bytes per window
constexpr uint32_t kProbs = 258;
constexpr uint32_t kTop = 1u << 24;
constexpr uint32_t kStreamAlign = 64; // where xlz_batch_bcj2 puts the raw streams it uploads

// What one wave merges per second, in bytes of OUTPUT.  AN ESTIMATE -- the kernel has not been measured on an MI355X yet
// (tools/bcj2_bench.py -> profiles/device_bcj2.txt does it): a window costs five barriers, some twenty LDS round trips
// and, for machine code (the Python binary: forty conversions per KiB of main stream), fifty to sixty decisions of one to
// two hundred cycles each on lane 0 and a dozen line loads from HBM: taken as 10 us per KiB.  The launch-length rule
// (never a launch of more than half a second, as xlz_sha256_plan has it) follows from it: an item longer than
// kMaxDeviceLen is merged on the host.
constexpr double kWaveBytesPerS = 100e6;
constexpr uint64_t kMaxDeviceLen = (uint64_t)(0.5 * kWaveBytesPerS);

constexpr int kStOk = 0, kStResult = -1; // XLZ_OK, XLZ_ERR_RESULT

XLZ_BCJ2_HD bool is_j(uint32_t prev, uint32_t b) { return (b & 0xFE) == 0xE8 || (prev == 0x0F && (b & 0xF0) == 0x80); }
XLZ_BCJ2_HD uint32_t prob_index(uint32_t prev, uint32_t b) { return b == 0xE8 ? prev : b == 0xE9 ? 256u : 257u; }

// ---- the serial twin: what xlz_bcj2_host runs, and what the wave scheme is compared with ----
// -> kStOk / kStResult; *produced (optional) = bytes written to out
inline int host_merge(const uint8_t *main, size_t main_len, const uint8_t *call, size_t call_len, const uint8_t *jump, size_t jump_len,
                      const uint8_t *rc, size_t rc_len, uint8_t *out, size_t out_len, size_t *produced)
{
    if (produced) *produced = 0;
    if (out_len == 0) return kStOk;
    if (rc_len < 5) return kStResult;
    uint16_t p[kProbs];
    for (uint32_t i = 0; i < kProbs; i++) p[i] = 1024;
    uint32_t code = 0, range = 0xFFFFFFFFu, prev = 0;
    size_t rp = 0, mp = 0, cp = 0, jp = 0, op = 0;
    for (; rp < 5; rp++) code = code << 8 | rc[rp];
    int st = kStOk;
    for (;;) {
        uint32_t b = 0;
        bool cand = false;
        while (mp < main_len && op < out_len) {
            b = main[mp++];
            out[op++] = (uint8_t)b;
            if (is_j(prev, b)) {
                cand = true;
                break;
            }
            prev = b;
        }
        if (!cand || op == out_len) break;
        uint16_t &pr = p[prob_index(prev, b)];
        const uint32_t bound = (range >> 11) * pr;
        const bool bit = code >= bound;
        if (!bit)
            range = bound, pr = (uint16_t)(pr + ((2048 - pr) >> 5));
        else
            range -= bound, code -= bound, pr = (uint16_t)(pr - (pr >> 5));
        if (range < kTop) {
            if (rp == rc_len) {
                st = kStResult;
                break;
            }
            range <<= 8, code = code << 8 | rc[rp++];
        }
        if (!bit) {
            prev = b;
            continue;
        }
        const uint8_t *s = b == 0xE8 ? call : jump;
        size_t &sp = b == 0xE8 ? cp : jp;
        if ((b == 0xE8 ? call_len : jump_len) - sp < 4) {
            st = kStResult;
            break;
        }
        const uint32_t src = (uint32_t)s[sp] << 24 | (uint32_t)s[sp + 1] << 16 | (uint32_t)s[sp + 2] << 8 | s[sp + 3];
        sp += 4;
        const uint32_t dest = src - (uint32_t)(op + 4);
        for (uint32_t k = 0; k < 4 && op < out_len; k++) out[op++] = (uint8_t)(dest >> (8 * k));
        if (op == out_len) break;
        prev = dest >> 24;
    }
    if (produced) *produced = op;
    return st == kStOk && op == out_len ? kStOk : kStResult;
}

// ---- the wave scheme ----
struct DevItem {
    const uint8_t *main, *call, *jump, *rc; // multiples of 16 (see the head of this file)
    uint32_t main_len, call_len, jump_len, rc_len;
    uint64_t dst;     // where the item's output goes, from the destination pointer
    uint32_t out_len; // (a folder of 4 GiB and more never gets here)
    uint32_t reserved;
};
struct DevResult {
    uint32_t produced;
    int32_t status; // kStOk / kStResult
};

// a sixteen-byte line of one of the three side streams
struct Line {
    uint32_t q[4];
    uint32_t base; // the line's offset in its stream, ~0u: none yet
};

// what a workgroup keeps in LDS
struct Wave {
    alignas(16) uint8_t win[kWindow];           // the window of the main stream
    alignas(16) uint8_t obuf[5 * kWindow + 16]; // the window's output: every byte may be a converted opcode
    uint16_t cand[kLanes]; // per lane: which of its bytes are candidates
    uint16_t conv[kLanes]; // ... and which were converted
    uint16_t pre[kLanes];  // conversions in front of the lane's first byte
    uint16_t prob[kProbs];
    Line rcl, calll, jumpl;
    uint32_t range, code, rc_pos, call_pos, jump_pos;
    uint32_t prev;     // of the next window's first byte
    uint32_t main_pos; // the next window's first byte
    uint32_t out_pos;  // output bytes so far
    uint32_t wn, win_base, win_out; // of the window just decided: main bytes, first output position, output bytes
    uint32_t done, failed;
};

XLZ_BCJ2_HD void load_line(uint32_t q[4], const uint8_t *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 v = *reinterpret_cast<const uint4 *>(p);
    q[0] = v.x, q[1] = v.y, q[2] = v.z, q[3] = v.w;
#else
    memcpy(q, p, 16);
#endif
}
// byte `pos` of the stream at p (the caller has checked pos < the stream's length)
XLZ_BCJ2_HD uint32_t line_byte(Line &l, const uint8_t *p, uint32_t pos)
{
    const uint32_t a = pos & ~15u;
    if (l.base != a) load_line(l.q, p + a), l.base = a;
    return (l.q[(pos >> 2) & 3] >> (8 * (pos & 3))) & 0xFF;
}
// the big-endian word at `pos`, a multiple of 4 (pos + 4 <= the stream's length)
XLZ_BCJ2_HD uint32_t line_be32(Line &l, const uint8_t *p, uint32_t pos)
{
    const uint32_t a = pos & ~15u;
    if (l.base != a) load_line(l.q, p + a), l.base = a;
    const uint32_t v = l.q[(pos >> 2) & 3];
    return v << 24 | (v & 0xFF00u) << 8 | (v >> 8 & 0xFF00u) | v >> 24;
}

XLZ_BCJ2_HD void wave_init(Wave &w, const DevItem &it, uint32_t lane)
{
    for (uint32_t i = lane; i < kProbs; i += kLanes) w.prob[i] = 1024;
    if (lane != 0) return;
    w.rcl.base = w.calll.base = w.jumpl.base = ~0u;
    w.range = 0xFFFFFFFFu, w.code = 0, w.rc_pos = w.call_pos = w.jump_pos = 0;
    w.prev = 0, w.main_pos = 0, w.out_pos = 0, w.wn = w.win_base = w.win_out = 0;
    w.done = 0, w.failed = 0;
    if (it.out_len == 0) {
        w.done = 1;
    } else if (it.rc_len < 5) {
        w.done = w.failed = 1;
    } else {
        for (; w.rc_pos < 5; w.rc_pos++) w.code = w.code << 8 | line_byte(w.rcl, it.rc, w.rc_pos);
        if (it.main_len == 0) w.done = 1;
    }
}

XLZ_BCJ2_HD uint32_t window_len(const Wave &w, const DevItem &it)
{
    const uint32_t left = it.main_len - w.main_pos;
    return left < kWindow ? left : kWindow;
}

XLZ_BCJ2_HD void wave_load(Wave &w, const DevItem &it, uint32_t lane)
{
    const uint32_t at = kLaneBytes * lane;
    if (at >= window_len(w, it)) return; // (the line that holds the stream's last byte is read whole)
    uint32_t q[4];
    load_line(q, it.main + w.main_pos + at);
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<uint4 *>(w.win + at) = make_uint4(q[0], q[1], q[2], q[3]);
#else
    memcpy(w.win + at, q, 16);
#endif
}

XLZ_BCJ2_HD void wave_mark(Wave &w, const DevItem &it, uint32_t lane)
{
    const uint32_t wn = window_len(w, it), at = kLaneBytes * lane;
    uint32_t m = 0;
    if (at < wn) {
        uint32_t prev = lane ? w.win[at - 1] : w.prev;
        for (uint32_t j = 0; j < kLaneBytes && at + j < wn; j++) {
            const uint32_t b = w.win[at + j];
            if (is_j(prev, b)) m |= 1u << j;
            prev = b;
        }
    }
    w.cand[lane] = (uint16_t)m, w.conv[lane] = 0;
}

// lane 0 alone
XLZ_BCJ2_HD void wave_decide(Wave &w, const DevItem &it)
{
    const uint32_t wn = window_len(w, it), base = w.out_pos;
    uint32_t k = 0;                      // conversions of this window so far
    uint32_t conv_next = ~0u, conv_top = 0; // the position behind the latest conversion, and its dest >> 24
    uint32_t range = w.range, code = w.code;
    bool stop = false, failed = false;
    uint32_t li = 0;
    for (; li < kLanes && !stop; li++) {
        w.pre[li] = (uint16_t)k;
        uint32_t m = w.cand[li];
        while (m) {
            const uint32_t j = (uint32_t)__builtin_ctz(m), p = kLaneBytes * li + j;
            m &= m - 1;
            const uint64_t o = (uint64_t)base + p + 4ull * k; // where the opcode lands in the output
            if (o + 1 >= it.out_len) {                        // not copied any more, or the last output byte: no bit
                stop = true;
                break;
            }
            const uint32_t b = w.win[p];
            const uint32_t prev = p == conv_next ? conv_top : p ? w.win[p - 1] : w.prev;
            uint16_t &pr = w.prob[prob_index(prev, b)];
            const uint32_t bound = (range >> 11) * pr;
            const bool bit = code >= bound;
            if (!bit)
                range = bound, pr = (uint16_t)(pr + ((2048 - pr) >> 5));
            else
                range -= bound, code -= bound, pr = (uint16_t)(pr - (pr >> 5));
            if (range < kTop) {
                if (w.rc_pos >= it.rc_len) {
                    stop = failed = true;
                    break;
                }
                range <<= 8, code = code << 8 | line_byte(w.rcl, it.rc, w.rc_pos);
                w.rc_pos++;
            }
            if (!bit) continue;
            const bool is_call = b == 0xE8;
            uint32_t &sp = is_call ? w.call_pos : w.jump_pos;
            if ((is_call ? it.call_len : it.jump_len) - sp < 4) {
                stop = failed = true;
                break;
            }
            const uint32_t src = line_be32(is_call ? w.calll : w.jumpl, is_call ? it.call : it.jump, sp);
            sp += 4;
            const uint32_t dest = src - (uint32_t)(o + 5);
            uint8_t *q = w.obuf + p + 4 * k + 1;
            q[0] = (uint8_t)dest, q[1] = (uint8_t)(dest >> 8), q[2] = (uint8_t)(dest >> 16), q[3] = (uint8_t)(dest >> 24);
            w.conv[li] = (uint16_t)(w.conv[li] | 1u << j);
            k++;
            conv_next = p + 1, conv_top = dest >> 24;
            if (o + 5 >= it.out_len) { // the operand reaches the end of the output
                stop = true;
                break;
            }
            if (p + 1 < wn && conv_top == 0x0F && (w.win[p + 1] & 0xF0) == 0x80) { // the candidate only the merge sees
                if (j + 1 < kLaneBytes)
                    m |= 1u << (j + 1);
                else
                    w.cand[li + 1] = (uint16_t)(w.cand[li + 1] | 1u);
            }
        }
    }
    for (; li < kLanes; li++) w.pre[li] = (uint16_t)k; // (stopped: what lies behind is cut off by the output's end, or void)
    w.range = range, w.code = code;
    const uint64_t n_out = (uint64_t)wn + 4ull * k, room = it.out_len - base;
    w.wn = wn, w.win_base = base;
    w.win_out = (uint32_t)(n_out < room ? n_out : room);
    w.out_pos = base + w.win_out;
    w.prev = conv_next == wn ? conv_top : w.win[wn - 1];
    w.main_pos += wn;
    if (failed) w.failed = 1;
    if (failed || w.out_pos == it.out_len || w.main_pos == it.main_len) w.done = 1;
}

XLZ_BCJ2_HD void wave_place(Wave &w, uint32_t lane)
{
    const uint32_t at = kLaneBytes * lane, pre = w.pre[lane], cm = w.conv[lane];
    for (uint32_t j = 0; j < kLaneBytes && at + j < w.wn; j++)
        w.obuf[at + j + 4 * (pre + (uint32_t)__builtin_popcount(cm & ((1u << j) - 1)))] = w.win[at + j];
}

XLZ_BCJ2_HD uint32_t obuf_word(const Wave &w, uint32_t a) // a: a multiple of 4
{
    uint32_t v;
    memcpy(&v, __builtin_assume_aligned(w.obuf + a, 4), 4);
    return v;
}

XLZ_BCJ2_HD void wave_store(const Wave &w, const DevItem &it, uint8_t *dst, uint32_t lane)
{
    uint8_t *d = dst + it.dst + w.win_base;
    const uint32_t n = w.win_out;
    uint32_t head = (uint32_t)(0 - (uintptr_t)d) & 15;
    if (head > n) head = n;
    const uint32_t chunks = (n - head) >> 4, tail = n - head - 16 * chunks;
    if (lane < head) d[lane] = w.obuf[lane];
    for (uint32_t c = lane; c < chunks; c += kLanes) {
        const uint32_t off = head + 16 * c, a = off & ~3u, sh = 8 * (off & 3);
        uint32_t x[5], y[4];
        for (uint32_t i = 0; i < 5; i++) x[i] = obuf_word(w, a + 4 * i); // (a + 20 <= sizeof obuf: its sixteen spare bytes)
        for (uint32_t i = 0; i < 4; i++) y[i] = sh ? x[i] >> sh | x[i + 1] << (32 - sh) : x[i];
#if defined(__HIP_DEVICE_COMPILE__)
        *reinterpret_cast<uint4 *>(d + off) = make_uint4(y[0], y[1], y[2], y[3]);
#else
        memcpy(d + off, y, 16);
#endif
    }
    if (lane < tail) d[head + 16 * chunks + lane] = w.obuf[head + 16 * chunks + lane];
}

XLZ_BCJ2_HD DevResult wave_result(const Wave &w, const DevItem &it)
{
    DevResult r;
    r.produced = w.out_pos;
    r.status = !w.failed && w.out_pos == it.out_len ? kStOk : kStResult;
    return r;
}

// the sizes xlz_batch_bcj2 lays a raw stream out by: its place is a multiple of kStreamAlign, the next one behind its
// last line
XLZ_BCJ2_HD uint64_t padded(uint64_t len) { return (len + kStreamAlign - 1) / kStreamAlign * kStreamAlign; }

} // namespace xlzbcj2
