// xlz_pack_dev.h -- the pack of ranges of a batch's output arena into one caller-owned device buffer (xlz_pack_dev.hip),
// in a form that compiles both as device code and as plain C++: a g++ program runs the tile / lane scheme lane by lane on
// the CPU (tests/c/pack_dev_selftest.cpp).  The reference keeps every output in host memory and has nothing of the kind.
//
// The arena keeps every stream in a region of its own (region_bytes: 256-byte aligned, kRegionPad bytes behind the
// stream), so a decoded file is never contiguous there; the destination is, and an item's place in it has no alignment in
// common with its place in the arena.  A launch gets a table of items {src, dst, len}: len > 0, sorted by dst, disjoint
// in the destination; src counts from the arena's first byte, dst from `dst`, a pointer the host rounds DOWN to a
// multiple of 16 (it adds what it took off to every item's dst).
//
// A workgroup of kThreads lanes takes TILES of kTileBytes of the destination (tile t = [t, t + 1) * kTileBytes), finds the
// item its tile starts in by binary search and copies the PORTION the tile holds of that item and of every following one
// that begins inside the tile.  Per portion [d0, d1):
//   * single bytes up to the destination's next 16-byte boundary a0 (lane k copies byte d0 + k),
//   * 16-byte stores at the boundaries a0, a0 + 16, ... < a1 = a0 + ((d1 - a0) & ~15), chunk c by lane c mod kThreads:
//     consecutive lanes store consecutive 16 bytes,
//   * single bytes for the tail [a1, d1).
// The source of a chunk is s = src + (chunk's dst - item's dst).  r = s mod 16 is the same for every chunk of an item:
// r == 0 (source and destination congruent modulo 16) -- one aligned 16-byte load; otherwise the two aligned loads at
// s - r and s - r + 16 and a byte shift (shift16).  No lane depends on another one; nothing outside an item's destination
// bytes is stored.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define XLZ_PACK_HD __host__ __device__ inline
#else
#include <assert.h>
#define XLZ_PACK_HD inline
#endif

namespace xlzpack {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kTileBytes = 16384;
constexpr uint32_t kTileChunks = kTileBytes / 16;
// the output arena's layout (xlz_host.hip lays it out by these): a stream that may produce `cap` bytes owns
// region_bytes(cap) bytes from a multiple of kRegionAlign on, regions back to back from the arena's first byte
constexpr uint64_t kRegionAlign = 256;
constexpr uint64_t kRegionPad = 64;
XLZ_PACK_HD uint64_t region_bytes(uint64_t cap) { return (cap + kRegionPad + kRegionAlign - 1) / kRegionAlign * kRegionAlign; }

struct DevItem {
    uint64_t src; // arena offset of the item's first byte
    uint64_t dst; // where it goes, from the (16-byte aligned) destination pointer
    uint64_t len; // > 0
};

struct Quad {
    uint64_t lo, hi; // bytes 0-7, 8-15 (little-endian)
};

// The aligned sixteen bytes at arena + off (off a multiple of 16).  The chunks of an item [src, src + len) are built
// from loads at multiples of 16 in [src - 15, src + len + 15): up to 15 bytes in front of the item and 15 behind it.
// Such a load never leaves the arena allocation, whichever region the item lies in: the item is part of a stream's
// output, [R, R + cap) of a region that starts at R, a multiple of 256 -- so src rounded down to 16 is >= R, the region's
// own first byte, also for the arena's first region (R = 0) -- and ends at R + region_bytes(cap) >= R + cap + 64, so the
// last load ends at or below src + len rounded up to 16 <= R + cap + 15, inside the region's own pad, also for the
// arena's LAST region (and the arena has a pad of its own behind that).  The bytes read outside the item are never
// stored.  The plain C++ build asserts the bound.
XLZ_PACK_HD Quad load16(const uint8_t *arena, uint64_t arena_bytes, uint64_t off)
{
    Quad q;
#if defined(__HIP_DEVICE_COMPILE__)
    (void)arena_bytes;
    const uint4 v = *reinterpret_cast<const uint4 *>(arena + off);
    q.lo = (uint64_t)v.x | (uint64_t)v.y << 32, q.hi = (uint64_t)v.z | (uint64_t)v.w << 32;
#else
#if !defined(__HIPCC__)
    assert((off & 15) == 0 && off < arena_bytes && arena_bytes - off >= 16);
#endif
    (void)arena_bytes;
    memcpy(&q.lo, arena + off, 8), memcpy(&q.hi, arena + off + 8, 8);
#endif
    return q;
}
XLZ_PACK_HD void store16(uint8_t *dst, uint64_t off, Quad q)
{
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<uint4 *>(dst + off) = make_uint4((uint32_t)q.lo, (uint32_t)(q.lo >> 32), (uint32_t)q.hi, (uint32_t)(q.hi >> 32));
#else
#if !defined(__HIPCC__)
    assert((off & 15) == 0);
#endif
    memcpy(dst + off, &q.lo, 8), memcpy(dst + off + 8, &q.hi, 8);
#endif
}

// bytes r .. r + 15 of the 32 bytes a || b, 0 < r < 16
XLZ_PACK_HD Quad shift16(Quad a, Quad b, uint32_t r)
{
    const bool up = r >= 8;
    const uint64_t x0 = up ? a.hi : a.lo, x1 = up ? b.lo : a.hi, x2 = up ? b.hi : b.lo;
    const uint32_t sh = 8 * (r & 7); // 0 .. 56; (x << 1) << (63 - sh) is x << (64 - sh), and 0 for sh == 0
    Quad q;
    q.lo = (x0 >> sh) | ((x1 << 1) << (63 - sh));
    q.hi = (x1 >> sh) | ((x2 << 1) << (63 - sh));
    return q;
}

// the last item whose dst <= pos (item 0 if none is)
XLZ_PACK_HD uint32_t find_item(const DevItem *items, uint32_t n, uint64_t pos)
{
    uint32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (items[mid].dst <= pos) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// tiles of a launch: from the tile the first item starts in to the one the last item ends in
XLZ_PACK_HD uint64_t first_tile(const DevItem *items) { return items[0].dst / kTileBytes; }
XLZ_PACK_HD uint64_t tile_count(const DevItem *items, uint32_t n)
{
    return (items[n - 1].dst + items[n - 1].len - 1) / kTileBytes - first_tile(items) + 1;
}

// what `lane` of the workgroup that has destination tile `tile` does
XLZ_PACK_HD void tile_lane(const uint8_t *arena, uint64_t arena_bytes, uint8_t *dst, const DevItem *items, uint32_t n, uint64_t tile, uint32_t lane)
{
    const uint64_t t0 = tile * kTileBytes, t1 = t0 + kTileBytes;
    for (uint32_t i = find_item(items, n, t0); i < n; i++) {
        const DevItem it = items[i];
        if (it.dst >= t1) break;
        const uint64_t d0 = it.dst > t0 ? it.dst : t0, end = it.dst + it.len, d1 = end < t1 ? end : t1;
        if (d1 <= d0) continue; // (the item in front of the tile's first byte may end in front of it too)
        const uint64_t s0 = it.src + (d0 - it.dst);
        const uint32_t len = (uint32_t)(d1 - d0);
        uint32_t head = (uint32_t)(0 - d0) & 15;
        if (head > len) head = len;
        const uint32_t chunks = (len - head) >> 4, tail = len - head - 16 * chunks;
        if (lane < head) dst[d0 + lane] = arena[s0 + lane];
        const uint64_t a0 = d0 + head, sa = s0 + head;
        const uint32_t r = (uint32_t)sa & 15;
        // four chunks per lane cover a whole tile: the loads of all four first, then the stores
        Quad q[kTileChunks / kThreads];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint32_t k = 0; k < kTileChunks / kThreads; k++) {
            const uint32_t c = k * kThreads + lane;
            if (c >= chunks) break;
            const uint64_t s = sa + 16ull * c;
            if (r == 0) {
                q[k] = load16(arena, arena_bytes, s);
            } else {
                const Quad a = load16(arena, arena_bytes, s - r), b = load16(arena, arena_bytes, s - r + 16);
                q[k] = shift16(a, b, r);
            }
        }
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint32_t k = 0; k < kTileChunks / kThreads; k++) {
            const uint32_t c = k * kThreads + lane;
            if (c >= chunks) break;
            store16(dst, a0 + 16ull * c, q[k]);
        }
        if (lane < tail) dst[a0 + 16ull * chunks + lane] = arena[sa + 16ull * chunks + lane];
    }
}

// source and destination of an item congruent modulo 16: the kernel's one-load path
XLZ_PACK_HD bool congruent(const DevItem &it) { return ((it.src ^ it.dst) & 15) == 0; }

} // namespace xlzpack
