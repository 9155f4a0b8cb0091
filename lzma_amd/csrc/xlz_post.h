// xlz_post.h -- what the post-decode stage of xlz_host.hip (filters, CRC32 / CRC64, SHA-256 behind a collected batch)
// decides without a device: which bytes of a stream or of a device destination a range means and where they lie, how its
// statistics add up, and how its host work is spread over threads.
// Plain C++ (tests/c/post_selftest.cpp runs it without a GPU); not part of the C ABI.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/xlz.h"
#include "xlz_windows.h"

// what xlz_decode_batch runs behind its (sub-)batches: the filter steps, then the digests of `ranges` over the filtered
// bytes.  Exactly one of crc_out (64-bit digests: xlz_decode_batch_checked / _filtered; no XLZ_CHECK_SHA256) and
// digest_out (xlz_decode_batch_digests) is set when n_ranges != 0.  accumulate: add to the context's statistics instead
// of starting them over (the container front-ends, which reset them once per file).
struct PostWork {
    const xlz_filter_step *steps = nullptr;
    size_t n_steps = 0;
    const xlz_check_range *ranges = nullptr;
    size_t n_ranges = 0;
    uint64_t *crc_out = nullptr;
    xlz_digest *digest_out = nullptr;
    bool accumulate = false;
};

namespace xlzpost {

// what a stream left behind: out_len as its result says; `cap` bounds the bytes that exist of a stream in the output
// arena (its reservation there) and of an oversize stream (4 GiB and more: the caller's buffer, where its session wrote);
// a stream outside the arena that is not oversize was settled while parsing, and a range of it lies in the caller's
// buffer if that holds caller_cap bytes (0: there is no buffer to read)
struct StreamOut {
    uint64_t out_len, cap;
    bool in_arena, oversize;
    uint64_t caller_cap;
};
enum class Place { Empty, Arena, Caller, Oversize };
struct Clip {
    uint64_t lo, hi; // the bytes [lo, hi) of the stream
    Place place;     // Empty: none of them exists (hi == lo, or no buffer holds them); Oversize: whether hi == lo or not
};
// [off, off + len) clipped to what the stream produced.  len may be anything up to 2^64 - 1 (a whole-stream range):
// off + len is never formed unless it fits.
inline Clip clip(const StreamOut &s, uint64_t off, uint64_t len)
{
    const uint64_t produced = s.in_arena || s.oversize ? std::min(s.out_len, s.cap) : s.out_len;
    const uint64_t lo = std::min(off, produced), hi = len > produced - lo ? produced : lo + len;
    if (s.oversize) return {lo, hi, Place::Oversize};
    if (hi == lo) return {lo, hi, Place::Empty};
    if (s.in_arena) return {lo, hi, Place::Arena};
    return {lo, hi, hi <= s.caller_cap ? Place::Caller : Place::Empty};
}
constexpr uint64_t kWholeStream = ~(uint64_t)0; // clip(s, 0, kWholeStream): all the stream produced (a filter step)

// xlz_check_range::stream of a range that names no stream but bytes [off, off + len) of the DESTINATION of
// xlz_internal_decode_device (xlz_check_host.h).  Internal: no batch has that many streams, so the public calls refuse it.
constexpr uint64_t kDestStream = ~(uint64_t)0;
// Such a range for the check kernels, which read aligned lines: their base is the destination pointer rounded down to 16,
// `mis` (pointer & 15) bytes in front of it.  -> *at: the range's offset behind that base; false: [off, off + len) does
// not lie inside the destination's `cap` bytes (no sum is formed unless it fits).  An empty range may sit at `cap`.
inline bool dest_resolve(uint64_t off, uint64_t len, uint64_t cap, uint64_t mis, uint64_t *at)
{
    if (mis > 15 || cap > ~(uint64_t)0 - mis || off > cap || len > cap - off) return false;
    *at = off + mis;
    return true;
}

// xlz_check_stats, xlz_sha256_stats and xlz_filter_stats share seven counters; the filters call their ranges steps
template <class T> struct Counts {
    static constexpr uint64_t T::*device = &T::device_ranges, T::*host = &T::host_ranges, T::*empty = &T::empty_ranges;
};
template <> struct Counts<xlz_filter_stats> {
    using T = xlz_filter_stats;
    static constexpr uint64_t T::*device = &T::device_steps, T::*host = &T::host_steps, T::*empty = &T::empty_steps;
};
// t += a over the seven shared counters, between any two of the three
template <class T, class A> void stats_add(T &t, const A &a)
{
    t.*Counts<T>::device += a.*Counts<A>::device, t.*Counts<T>::host += a.*Counts<A>::host, t.*Counts<T>::empty += a.*Counts<A>::empty;
    t.device_bytes += a.device_bytes, t.host_bytes += a.host_bytes, t.kernel_ms += a.kernel_ms, t.launches += a.launches;
}
// ... and xlz_sha256_stats' eighth, which is no sum: the longest range any launch gave the device
struct ThresholdIsMax {};
inline void stats_add(xlz_sha256_stats &t, const xlz_sha256_stats &a, ThresholdIsMax)
{
    stats_add(t, a);
    t.threshold = std::max(t.threshold, a.threshold);
}

// t += a for the pack's and the BCJ2 merge's counters (no two of these share a layout with the seven above)
inline void stats_add(xlz_pack_stats &t, const xlz_pack_stats &a)
{
    t.items += a.items, t.bytes += a.bytes, t.empty_items += a.empty_items, t.congruent_items += a.congruent_items;
    t.kernel_ms += a.kernel_ms, t.launches += a.launches;
}
inline void stats_add(xlz_bcj2_stats &t, const xlz_bcj2_stats &a)
{
    t.device_items += a.device_items, t.device_bytes += a.device_bytes, t.host_items += a.host_items, t.host_bytes += a.host_bytes;
    t.failed_items += a.failed_items, t.kernel_ms += a.kernel_ms, t.launches += a.launches;
}

// min(cap, the machine's hardware threads), at least 1: how many host threads a stage may use
inline unsigned host_thread_cap(unsigned cap)
{
    const unsigned hw = std::thread::hardware_concurrency();
    return std::max(1u, std::min(hw ? hw : 1u, cap));
}
// f(i) for every i in [0, n), each once, on at most k threads of which the caller is one: every thread takes the next i
// that nobody has.  Where a thread cannot be created, those that exist (the caller at least) do the rest.  f must not throw.
template <class F> void parallel_for(size_t n, size_t k, F &&f)
{
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (size_t i; (i = next.fetch_add(1)) < n;) f(i);
    };
    std::vector<std::thread> th;
    try {
        for (size_t t = 1; t < k && t < n; t++) th.emplace_back(work);
    } catch (...) {
    }
    work();
    for (auto &x : th) x.join();
}

// xlz_batch_pack's table as the caller declares it: every item names a stream of the batch, its destination range
// [dst_off, dst_off + len) lies inside dst_cap (the sum is never formed unless it fits) and no two declared ranges share
// a byte -- declared, not clipped: what a stream produced must not decide whether a call is well formed.  An item of
// length 0 declares no byte.
inline bool pack_items_ok(const xlz_pack_item *items, size_t n, size_t n_streams, uint64_t dst_cap)
{
    std::vector<xlzwin::Window> r;
    for (size_t i = 0; i < n; i++) {
        if (items[i].stream >= n_streams) return false;
        r.emplace_back(items[i].dst_off, items[i].len); // (one of length 0 too: its dst_off must lie inside dst_cap)
    }
    return xlzwin::disjoint_within(std::move(r), dst_cap);
}

} // namespace xlzpost
