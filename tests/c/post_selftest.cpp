// What the post-decode stage decides without a device (lzma_amd/csrc/xlz_post.h): which bytes of a stream a range means
// and where they lie -- among them the streams of 4 GiB and more, which no GPU test of a few seconds reaches --, and how
// the statistics add up; where a range of a device destination lies for the check kernels; and the host-thread helper.
// Prints "ok" and exits 0, or says what differs.  "threads" as the only argument: the thread helper alone (the part to
// run under -fsanitize=thread).
#include <cstdio>
#include <cstring>
#include <numeric>

#include "xlz_post.h"

using namespace xlzpost;

static int failures = 0;
static const uint64_t kMax = ~(uint64_t)0;

static const char *name(Place p)
{
    return p == Place::Empty ? "empty" : p == Place::Arena ? "arena" : p == Place::Caller ? "caller" : "oversize";
}

static void want(const char *what, const StreamOut &s, uint64_t off, uint64_t len, uint64_t lo, uint64_t hi, Place place)
{
    const Clip c = clip(s, off, len);
    if (c.lo == lo && c.hi == hi && c.place == place) return;
    printf("%s: [%llu, %llu) %s, expected [%llu, %llu) %s\n", what, (unsigned long long)c.lo, (unsigned long long)c.hi, name(c.place),
           (unsigned long long)lo, (unsigned long long)hi, name(place));
    failures++;
}

static void clips()
{
    // {out_len, cap, in_arena, oversize, caller_cap}
    const StreamOut arena = {1000, 4096, true, false, 0}, caller = {1000, 0, false, false, 1000};
    want("inside", arena, 10, 20, 10, 30, Place::Arena);
    want("longer than the output", arena, 990, 20, 990, 1000, Place::Arena);
    want("off behind what was produced", arena, 1001, 5, 1000, 1000, Place::Empty);
    want("off far behind what was produced", arena, kMax, 5, 1000, 1000, Place::Empty);
    want("off equal to what was produced", arena, 1000, 5, 1000, 1000, Place::Empty);
    want("len 0", arena, 10, 0, 10, 10, Place::Empty);
    want("len 2^64 - 1, off 0", arena, 0, kMax, 0, 1000, Place::Arena);
    want("len 2^64 - 1, off odd", arena, 7, kMax, 7, 1000, Place::Arena);
    want("off + len wraps past 2^64", arena, 999, kMax - 3, 999, 1000, Place::Arena);
    want("off + len wraps to a small sum", arena, 600, kMax - 599 + 100, 600, 1000, Place::Arena);
    want("off + len == 2^64 - 1", arena, 1, kMax - 1, 1, 1000, Place::Arena);
    want("nothing produced", {0, 4096, true, false, 0}, 0, kMax, 0, 0, Place::Empty);
    want("nothing produced, off > 0", {0, 4096, true, false, 0}, 5, 5, 0, 0, Place::Empty);
    want("nothing produced outside the arena", {0, 0, false, false, 100}, 0, kMax, 0, 0, Place::Empty);
    want("out_len above out_cap in the arena: clipped", {5000, 4096, true, false, 0}, 0, kMax, 0, 4096, Place::Arena);
    want("... and a range behind the clip", {5000, 4096, true, false, 0}, 4096, 100, 4096, 4096, Place::Empty);
    want("out_len above out_cap outside the arena: not clipped", {5000, 4096, false, false, 5000}, 0, kMax, 0, 5000, Place::Caller);
    want("outside the arena, inside the caller's buffer", caller, 10, 20, 10, 30, Place::Caller);
    want("outside the arena, the caller's buffer ends at hi", caller, 0, kMax, 0, 1000, Place::Caller);
    want("outside the arena, the caller's buffer is shorter", {1000, 0, false, false, 999}, 0, kMax, 0, 1000, Place::Empty);
    want("... but holds the range", {1000, 0, false, false, 999}, 0, 999, 0, 999, Place::Caller);
    want("outside the arena, no buffer", {1000, 0, false, false, 0}, 0, 1, 0, 1, Place::Empty);
    const uint64_t big = 5ull << 32;
    const StreamOut over = {big, big + 10, false, true, 0};
    want("oversize, whole stream", over, 0, kMax, 0, big, Place::Oversize);
    want("oversize, a range behind 4 GiB", over, (1ull << 32) + 1, 3ull << 32, (1ull << 32) + 1, (4ull << 32) + 1, Place::Oversize);
    want("oversize, off + len wraps", over, big - 1, kMax, big - 1, big, Place::Oversize);
    want("oversize, off behind", over, big + 1, 5, big, big, Place::Oversize);
    want("oversize, clipped to the caller's buffer", {big, big - 3, false, true, 0}, 0, kMax, 0, big - 3, Place::Oversize);
    want("oversize, nothing produced", {0, big, false, true, 0}, 0, kMax, 0, 0, Place::Oversize);
    want("whole stream", arena, 0, kWholeStream, 0, 1000, Place::Arena);
}

#define EQ(a, b) ((a) == (b) ? (void)0 : (void)(printf("line %d: %s != %s\n", __LINE__, #a, #b), failures++))

static void stats()
{
    xlz_check_stats c;
    xlz_sha256_stats s, s2;
    xlz_filter_stats f, f2;
    memset(&c, 0, sizeof c), memset(&s, 0, sizeof s), memset(&s2, 0, sizeof s2), memset(&f, 0, sizeof f), memset(&f2, 0, sizeof f2);
    c.device_ranges = 1, c.device_bytes = 2, c.host_ranges = 3, c.host_bytes = 4, c.empty_ranges = 5, c.kernel_ms = 0.5, c.launches = 6;
    c.reserved = 9;
    s.device_ranges = 10, s.device_bytes = 20, s.host_ranges = 30, s.host_bytes = 40, s.empty_ranges = 50, s.kernel_ms = 0.25, s.launches = 60;
    s.threshold = 4096, s.reserved = 9;
    stats_add(c, s); // the SHA-256 ranges count in xlz_check_stats too
    EQ(c.device_ranges, 11u), EQ(c.device_bytes, 22u), EQ(c.host_ranges, 33u), EQ(c.host_bytes, 44u), EQ(c.empty_ranges, 55u);
    EQ(c.kernel_ms, 0.75), EQ(c.launches, 66u), EQ(c.reserved, 9u);
    stats_add(c, c);
    EQ(c.device_ranges, 22u), EQ(c.launches, 132u), EQ(c.kernel_ms, 1.5);
    // SHA-256 into SHA-256: seven sums, and the threshold is a maximum, whichever side holds it
    s2.device_ranges = 1, s2.device_bytes = 1, s2.host_ranges = 1, s2.host_bytes = 1, s2.empty_ranges = 1, s2.kernel_ms = 1, s2.launches = 1;
    s2.threshold = 100;
    stats_add(s2, s, ThresholdIsMax{});
    EQ(s2.device_ranges, 11u), EQ(s2.device_bytes, 21u), EQ(s2.host_ranges, 31u), EQ(s2.host_bytes, 41u), EQ(s2.empty_ranges, 51u);
    EQ(s2.kernel_ms, 1.25), EQ(s2.launches, 61u), EQ(s2.threshold, 4096u);
    s.threshold = 7;
    stats_add(s2, s, ThresholdIsMax{});
    EQ(s2.threshold, 4096u), EQ(s2.device_ranges, 21u);
    s.threshold = 4097;
    stats_add(s2, s, ThresholdIsMax{});
    EQ(s2.threshold, 4097u), EQ(s2.device_ranges, 31u);
    // the filters' spelling of the same seven
    f.device_steps = 1, f.device_bytes = 2, f.host_steps = 3, f.host_bytes = 4, f.empty_steps = 5, f.kernel_ms = 2, f.launches = 7;
    f2 = f;
    stats_add(f2, f);
    EQ(f2.device_steps, 2u), EQ(f2.device_bytes, 4u), EQ(f2.host_steps, 6u), EQ(f2.host_bytes, 8u), EQ(f2.empty_steps, 10u);
    EQ(f2.kernel_ms, 4.0), EQ(f2.launches, 14u);
}

static void more_stats()
{
    xlz_pack_stats p, p2;
    xlz_bcj2_stats b, b2;
    memset(&p, 0, sizeof p), memset(&b, 0, sizeof b);
    p.items = 1, p.bytes = 2, p.congruent_items = 3, p.empty_items = 4, p.kernel_ms = 0.5, p.launches = 5, p.reserved = 9;
    p2 = p;
    stats_add(p2, p);
    EQ(p2.items, 2u), EQ(p2.bytes, 4u), EQ(p2.congruent_items, 6u), EQ(p2.empty_items, 8u), EQ(p2.kernel_ms, 1.0), EQ(p2.launches, 10u);
    EQ(p2.reserved, 9u);
    b.device_items = 1, b.device_bytes = 2, b.host_items = 3, b.host_bytes = 4, b.failed_items = 5, b.kernel_ms = 0.25, b.launches = 6;
    b.reserved = 9;
    b2 = b;
    stats_add(b2, b);
    stats_add(b2, xlz_bcj2_stats{}); // (a reset front-end that merged nothing)
    EQ(b2.device_items, 2u), EQ(b2.device_bytes, 4u), EQ(b2.host_items, 6u), EQ(b2.host_bytes, 8u), EQ(b2.failed_items, 10u);
    EQ(b2.kernel_ms, 0.5), EQ(b2.launches, 12u), EQ(b2.reserved, 9u);
}

static void dest_ranges()
{
    const uint64_t cap = 1000;
    for (uint64_t mis = 0; mis < 16; mis++) { // all 16 misalignments: the range moves behind the rounded-down base by just that
        uint64_t at = 77;
        EQ(dest_resolve(0, 10, cap, mis, &at), true), EQ(at, mis);
        EQ(dest_resolve(cap - 10, 10, cap, mis, &at), true), EQ(at, cap - 10 + mis); // off == cap - len: the last bytes
        EQ(dest_resolve(cap, 0, cap, mis, &at), true), EQ(at, cap + mis);            // off == cap holds an empty range only
        EQ(dest_resolve(cap, 1, cap, mis, &at), false);
        EQ(dest_resolve(cap - 10, 11, cap, mis, &at), false);
        EQ(dest_resolve(0, 0, cap, mis, &at), true), EQ(at, mis); // len 0
        EQ(dest_resolve(0, cap, cap, mis, &at), true);
        EQ(dest_resolve(0, cap + 1, cap, mis, &at), false);
        EQ(dest_resolve(cap + 1, 0, cap, mis, &at), false);
        // sums that would wrap: off + len, and a destination so large that cap + mis does
        EQ(dest_resolve(1, kMax, cap, mis, &at), false), EQ(dest_resolve(kMax, 1, cap, mis, &at), false);
        EQ(dest_resolve(kMax, kMax, cap, mis, &at), false), EQ(dest_resolve(500, kMax - 499, cap, mis, &at), false);
        EQ(dest_resolve(kMax - 20, 5, kMax, mis, &at), mis == 0);
        EQ(dest_resolve(0, 0, kMax - mis, mis, &at), true), EQ(dest_resolve(kMax - 15, 0, kMax - 15, mis, &at), mis <= 15);
    }
    uint64_t at = 77;
    EQ(dest_resolve(0, 1, cap, 16, &at), false), EQ(at, 77u); // a misalignment is pointer & 15
    EQ(dest_resolve(0, 0, 0, 0, &at), true), EQ(at, 0u);      // an empty destination holds an empty range
    EQ(dest_resolve(0, 1, 0, 0, &at), false);
    EQ(kDestStream, kMax); // no batch has that many streams: the public calls refuse the index
}

// n indices on at most k threads: every index exactly once, whatever n and k; host_thread_cap stays inside [1, cap]
static void threads()
{
    const struct {
        size_t n, k;
    } shapes[] = {{0, 4}, {1, 4}, {1, 0}, {3, 8}, {5, 1}, {5, 0}, {16, 16}, {100000, 7}, {4096, 16}};
    for (const auto &sh : shapes) {
        std::vector<uint32_t> hit(sh.n, 0); // (each index is its own element: no two threads share one)
        std::atomic<size_t> calls{0};
        parallel_for(sh.n, sh.k, [&](size_t i) { hit[i]++, calls.fetch_add(1); });
        size_t once = 0;
        for (uint32_t h : hit) once += h == 1;
        EQ(once, sh.n), EQ(calls.load(), sh.n);
    }
    std::vector<uint64_t> sq(1000);
    parallel_for(sq.size(), host_thread_cap(16), [&](size_t i) { sq[i] = (uint64_t)i * i; });
    EQ(std::accumulate(sq.begin(), sq.end(), (uint64_t)0), (uint64_t)332833500);
    for (unsigned cap : {0u, 1u, 8u, 16u, 1000u}) {
        const unsigned t = host_thread_cap(cap);
        EQ(t >= 1 && (t <= cap || t == 1), true);
    }
}

int main(int argc, char **argv)
{
    if (argc <= 1 || strcmp(argv[1], "threads") != 0) {
        clips();
        stats();
        more_stats();
        dest_ranges();
    }
    threads();
    if (failures) return printf("%d failures\n", failures), 1;
    printf("ok\n");
    return 0;
}
