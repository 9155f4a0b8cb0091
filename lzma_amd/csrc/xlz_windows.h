// xlz_windows.h -- the two decisions that every front end makes about windows in one destination: whether the declared
// windows are disjoint and inside its capacity, and where windows of given sizes lie when they are laid back to back.
// Each front end filters what counts as a window (xlz_zip.h, xlz_7z_files.h, xlz_xz_many.h, xlz_post.h, the BCJ2 and
// inflate tables of the batch engine) and asks here.
// Plain C++ over the standard library alone (tests/c/windows_selftest.cpp runs it without a GPU); not part of the C ABI.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace xlzwin {

using Window = std::pair<uint64_t, uint64_t>; // (off, len): the bytes [off, off + len)

// true: every window lies inside cap (no sum is formed unless it fits) and no two windows share a byte.  A window of
// length 0 has to lie inside cap as well -- it may sit at cap -- but holds no byte: it shares none, wherever it is.
inline bool disjoint_within(std::vector<Window> w, uint64_t cap)
{
    size_t k = 0;
    for (const Window &x : w) {
        if (x.first > cap || x.second > cap - x.first) return false;
        if (x.second) w[k++] = x;
    }
    w.resize(k);
    std::sort(w.begin(), w.end());
    for (size_t i = 1; i < k; i++)
        if (w[i - 1].first + w[i - 1].second > w[i].first) return false;
    return true;
}

// Windows of sizes[0 .. n) back to back, in order: off[i] = the first multiple of align (>= 1) at or behind the end of
// window i - 1, *total = the end of the last one.  false: an offset or an end does not fit 64 bits (nothing is formed
// unless it fits); off[] and *total then hold nothing of use.
inline bool back_to_back(const uint64_t *sizes, size_t n, uint64_t align, uint64_t *off, uint64_t *total)
{
    const uint64_t top = ~(uint64_t)0;
    uint64_t at = 0;
    for (size_t i = 0; i < n; i++) {
        const uint64_t over = at % align;
        if (over) {
            if (align - over > top - at) return false;
            at += align - over;
        }
        off[i] = at;
        if (sizes[i] > top - at) return false;
        at += sizes[i];
    }
    *total = at;
    return true;
}

} // namespace xlzwin
