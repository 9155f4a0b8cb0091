// xlz_xz_cover.h -- what a read of byte ranges of an .xz file (xlz_xz_cover / xlz_xz_read, xlz_xz.hip) decides without a
// device: how a range is clipped to the decoded size, which blocks the ranges touch, whether the destinations are well
// formed, and how every range is cut into pack items over the covering blocks.
// Plain C++ (tests/c/xz_cover_selftest.cpp runs it without a GPU); not part of the C ABI.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/xlz.h"

namespace xlzcover {

// a block of the decoded file: bytes [off, off + len); the blocks of a file lie one behind the other from 0 (off[i + 1] =
// off[i] + len[i]), len may be 0
struct Extent {
    uint64_t off, len;
};

// [off, off + len) clipped to a file of `size` bytes, like pread: -> [lo, hi).  off + len is never formed unless it fits.
inline std::pair<uint64_t, uint64_t> clip(uint64_t size, uint64_t off, uint64_t len)
{
    const uint64_t lo = std::min(off, size);
    return {lo, len > size - lo ? size : lo + len};
}

// the first block that ends behind `pos` (the block that holds byte `pos`, for pos < size; nb otherwise): a binary
// search over the blocks' ends, which never decrease
inline size_t block_of(const Extent *b, size_t nb, uint64_t pos)
{
    size_t lo = 0, hi = nb;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (b[mid].off + b[mid].len > pos)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// the blocks [first, last) that may share a byte with the non-empty [lo, hi): every one of them does, but the empty ones
inline std::pair<size_t, size_t> span(const Extent *b, size_t nb, uint64_t lo, uint64_t hi)
{
    return {block_of(b, nb, lo), block_of(b, nb, hi - 1) + 1};
}

// The ascending, duplicate-free indices of the blocks that ranges[0 .. n) touch (a block is touched where it shares a
// byte with a clipped range; an empty block never is).  O(n log n + n log nb + the blocks between the ends of a range).
inline void cover(const Extent *b, size_t nb, uint64_t size, const xlz_xz_range *ranges, size_t n, std::vector<size_t> &out)
{
    std::vector<std::pair<size_t, size_t>> spans;
    for (size_t i = 0; i < n; i++) {
        const auto c = clip(size, ranges[i].off, ranges[i].len);
        if (c.first < c.second) spans.push_back(span(b, nb, c.first, c.second));
    }
    std::sort(spans.begin(), spans.end());
    out.clear();
    size_t next = 0; // every block in front of it has been looked at
    for (const auto &s : spans)
        for (size_t k = std::max(next, s.first); k < s.second; next = ++k)
            if (b[k].len) out.push_back(k);
}

// What a read does, settled before anything is launched.
struct Plan {
    std::vector<size_t> blocks;       // the cover
    std::vector<uint64_t> lens;       // per range: its clipped length (what the read reports as copied[i])
    std::vector<xlz_pack_item> items; // stream = position in `blocks`, off / len = what range and block share, from the block's start
    uint64_t total = 0;               // the sum of lens
};

// false: a clipped destination [dst_off, dst_off + lens[i]) does not fit in out_cap (no sum is formed unless it fits), or
// two of them share a byte.  A range clipped to nothing declares no byte, wherever its dst_off points.
inline bool plan(const Extent *b, size_t nb, uint64_t size, const xlz_xz_range *ranges, size_t n, uint64_t out_cap, Plan &p)
{
    p = Plan{};
    p.lens.assign(n, 0);
    std::vector<std::pair<uint64_t, uint64_t>> dst;
    for (size_t i = 0; i < n; i++) {
        const auto c = clip(size, ranges[i].off, ranges[i].len);
        const uint64_t len = c.second - c.first;
        if (!len) continue;
        if (ranges[i].dst_off > out_cap || len > out_cap - ranges[i].dst_off) return false;
        p.lens[i] = len, p.total += len; // (no wrap: the destinations are disjoint parts of out_cap once the test below passes)
        dst.emplace_back(ranges[i].dst_off, ranges[i].dst_off + len);
    }
    std::sort(dst.begin(), dst.end());
    for (size_t i = 1; i < dst.size(); i++)
        if (dst[i - 1].second > dst[i].first) return false;
    cover(b, nb, size, ranges, n, p.blocks);
    for (size_t i = 0; i < n; i++) {
        if (!p.lens[i]) continue;
        const uint64_t lo = std::min(ranges[i].off, size), hi = lo + p.lens[i];
        const auto s = span(b, nb, lo, hi);
        size_t at = std::lower_bound(p.blocks.begin(), p.blocks.end(), s.first) - p.blocks.begin();
        for (size_t k = s.first; k < s.second; k++) {
            if (!b[k].len) continue;
            const uint64_t from = std::max(lo, b[k].off), to = std::min(hi, b[k].off + b[k].len);
            p.items.push_back(xlz_pack_item{at++, from - b[k].off, to - from, ranges[i].dst_off + (from - lo)});
        }
    }
    return true;
}

} // namespace xlzcover
