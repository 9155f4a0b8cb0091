// xlz_xz_many.h -- what a decode of many .xz files as one batch (xlz_xz_many_layout / xlz_xz_decode_many /
// xlz_xz_decode_many_device, xlz_xz.hip) decides without a device: whether the files' windows in the destination are well
// formed, how windows are laid out back to back, which stream of the batch a (file, block) is, and how the outcomes of a
// file's blocks and of their checks fold into the file's verdict.
// Plain C++ (tests/c/xz_many_selftest.cpp runs it without a GPU); not part of the C ABI.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/xlz.h"
#include "xlz_windows.h"

namespace xlzmany {

// false: a window [dst_off, dst_off + dst_cap) does not fit in out_cap (no sum is formed unless it fits), or two windows
// share a byte.  A window with dst_cap == 0 declares no byte, wherever its dst_off points.
inline bool windows_ok(const xlz_xz_many_file *f, size_t n, uint64_t out_cap)
{
    std::vector<xlzwin::Window> w;
    for (size_t i = 0; i < n; i++)
        if (f[i].dst_cap) w.emplace_back(f[i].dst_off, f[i].dst_cap);
    return xlzwin::disjoint_within(std::move(w), out_cap);
}

// Windows of sizes[0 .. n) back to back, in order: off[i] = the first multiple of align (>= 1) at or behind the end of
// window i - 1, *total = the end of the last one.  false: an offset or an end does not fit 64 bits (nothing is formed
// unless it fits).
inline bool layout(const uint64_t *sizes, size_t n, uint64_t align, uint64_t *off, uint64_t *total)
{
    return xlzwin::back_to_back(sizes, n, align, off, total);
}

// Which stream of the one batch a (file, block) is: the files that got as far as the batch, in order, each with its
// blocks in file order.  A file that failed before puts nothing into the batch.
constexpr size_t kNotInBatch = ~(size_t)0;
struct Map {
    std::vector<size_t> first;   // per file: the stream of its block 0 (a file without blocks: where it would be); kNotInBatch
    std::vector<size_t> count;   // per file: its blocks in the batch
    std::vector<size_t> file_of; // per stream
    size_t stream(size_t file, size_t block) const { return first[file] + block; }
};
// in_batch[i] != 0: file i goes into the batch with blocks[i] blocks
inline Map map_streams(const uint8_t *in_batch, const size_t *blocks, size_t n)
{
    Map m;
    m.first.assign(n, kNotInBatch), m.count.assign(n, 0);
    for (size_t i = 0; i < n; i++) {
        if (!in_batch[i]) continue;
        m.first[i] = m.file_of.size(), m.count[i] = blocks[i];
        m.file_of.insert(m.file_of.end(), blocks[i], i);
    }
    return m;
}

// What a block's stream says of its file: the stream's own status where that is negative, XLZ_ERR_RESULT where it did
// not produce exactly what the index says or did not use its whole payload.
inline int32_t block_status(int32_t status, uint64_t out_len, uint64_t in_consumed, uint64_t want_out, uint64_t want_in)
{
    if (status < 0) return status;
    return out_len != want_out || in_consumed != want_in ? (int32_t)XLZ_ERR_RESULT : (int32_t)XLZ_OK;
}

// what the comparison of a block's check field said
enum : uint8_t { kCheckGood = 0, kCheckFailed = 1, kCheckUnverified = 2 }; // (unverified: a reserved check type)

struct Verdict {
    int32_t status;
    uint32_t unverified;
};
// A file's verdict from its streams [first, first + count) of block_st[] (block_status) and check[]: the first block in
// file order that failed, then -- verify only -- the first failed check, then XLZ_OK with the count of unverified blocks.
// check[] of a block that failed is not looked at.
inline Verdict fold(const int32_t *block_st, const uint8_t *check, size_t first, size_t count, bool verify)
{
    for (size_t k = 0; k < count; k++)
        if (block_st[first + k] < 0) return {block_st[first + k], 0};
    uint32_t nu = 0;
    for (size_t k = 0; k < count && verify; k++) {
        if (check[first + k] == kCheckFailed) return {XLZ_ERR_RESULT, 0};
        nu += check[first + k] == kCheckUnverified;
    }
    return {XLZ_OK, nu};
}

// a block of the device form must fit a unit's 32-bit counters, payload and output (xlz_batch_create: the streams that
// xlz_decode_batch decodes as sessions, which write host memory only)
constexpr uint64_t kMaxDeviceBlock = 0xFFFF0000ull;

} // namespace xlzmany
