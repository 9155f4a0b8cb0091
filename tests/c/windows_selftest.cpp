// windows_selftest.cpp -- lzma_amd/csrc/xlz_windows.h without a GPU, against brute-force byte-map models.  The predicate:
// a destination of `cap` bytes in which every window marks its bytes one by one says whether a window leaves it or two
// share a byte.  The layout: the offsets against 128-bit sums, and the windows it makes marked in such a destination.
// A few thousand seeded cases of at most 8 windows in a capacity of at most 64, and the edges by hand: a window of no
// bytes at the capacity, off + len wrapping 64 bits, windows that touch, an alignment that wraps.  Built plain and with
// the host sanitizers (tests/test_windows_cpu.py).
#include <cstdio>
#include <random>

#include "xlz_windows.h"

using xlzwin::Window;

static int fails = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            if (fails++ < 20) printf("%s:%d: %s\n", __FILE__, __LINE__, #c); \
        }                                                          \
    } while (0)

static const uint64_t kTop = ~(uint64_t)0;

// the model: every byte of every window is looked at on its own, 128 bits wide so that nothing wraps
static bool model_disjoint_within(const std::vector<Window> &w, uint64_t cap)
{
    std::vector<uint8_t> hit((size_t)cap, 0); // cap <= 64 here
    for (const Window &x : w) {
        if ((unsigned __int128)x.first + x.second > cap) return false;
        for (uint64_t j = 0; j < x.second; j++)
            if (hit[(size_t)(x.first + j)]++) return false;
    }
    return true;
}

static void predicate_case(std::mt19937_64 &rnd)
{
    const uint64_t cap = rnd() % 65;
    const size_t n = rnd() % 9;
    std::vector<Window> w(n);
    const bool well_formed = rnd() % 2; // half of the cases are laid without a fault, with gaps, then shuffled
    uint64_t at = 0;
    for (size_t i = 0; i < n; i++) {
        if (well_formed) {
            at += rnd() % 3;
            w[i] = {at, rnd() % 3 == 0 ? 0 : rnd() % 12};
            at += w[i].second;
        } else {
            const unsigned kind = (unsigned)(rnd() % 6);
            w[i].first = kind == 0 ? kTop - rnd() % 4 : kind == 1 ? cap : rnd() % (cap + 3);
            w[i].second = kind == 2 ? 0 : kind == 3 ? kTop - rnd() % 4 : rnd() % (cap + 3);
            if (kind == 4 && i) w[i] = w[rnd() % i]; // the same window twice
        }
    }
    for (size_t i = n; i > 1; i--) std::swap(w[i - 1], w[rnd() % i]);
    const uint64_t c = well_formed && at <= 64 ? at : cap; // (a laid set that outgrew 64 bytes is one more faulty case)
    const bool want = model_disjoint_within(w, c);
    CHECK(xlzwin::disjoint_within(w, c) == want);
    if (well_formed && at <= 64) {
        CHECK(want && xlzwin::disjoint_within(w, kTop));
        if (n && at) CHECK(!xlzwin::disjoint_within(w, at - 1)); // (the last window laid ends at `at`, bytes or none)
    }
}

static void layout_case(std::mt19937_64 &rnd)
{
    const size_t n = rnd() % 9;
    const unsigned kind = (unsigned)(rnd() % 8);
    const uint64_t align = kind == 0 ? kTop - rnd() % 3 : kind == 1 ? 1ull << (rnd() % 64) : 1 + rnd() % 9;
    std::vector<uint64_t> sizes(n), off(n, 7);
    for (uint64_t &s : sizes) s = kind == 2 ? kTop / 3 + rnd() % 5 : kind == 3 && rnd() % 3 == 0 ? kTop - rnd() % 70 : rnd() % 3 == 0 ? 0 : rnd() % 9;
    // the model: 128-bit sums
    unsigned __int128 at = 0;
    std::vector<unsigned __int128> want(n);
    bool fits = true;
    for (size_t i = 0; i < n && fits; i++) {
        at = (at + align - 1) / align * align;
        want[i] = at;
        fits = at <= kTop && at + sizes[i] <= kTop;
        at += sizes[i];
    }
    uint64_t total = 5;
    const bool got = xlzwin::back_to_back(sizes.data(), n, align, off.data(), &total);
    CHECK(got == fits);
    if (!got || !fits) return;
    CHECK(total == (uint64_t)at);
    std::vector<Window> w(n);
    for (size_t i = 0; i < n; i++) {
        CHECK(off[i] == (uint64_t)want[i] && off[i] % align == 0);
        w[i] = {off[i], sizes[i]};
    }
    CHECK(xlzwin::disjoint_within(w, total));
    if (total <= 64) CHECK(model_disjoint_within(w, total)); // what it lays is what the predicate's model accepts
}

int main()
{
    std::mt19937_64 rnd(20251021);
    for (int i = 0; i < 6000; i++) predicate_case(rnd);
    for (int i = 0; i < 6000; i++) layout_case(rnd);
    // ---- the edges by hand
    CHECK(xlzwin::disjoint_within({}, 0) && xlzwin::disjoint_within({}, kTop));
    CHECK(xlzwin::disjoint_within({{64, 0}}, 64));             // a window of no bytes may sit at the capacity ...
    CHECK(!xlzwin::disjoint_within({{65, 0}}, 64));            // ... and not behind it
    CHECK(xlzwin::disjoint_within({{0, 0}}, 0) && !xlzwin::disjoint_within({{0, 1}}, 0));
    CHECK(!xlzwin::disjoint_within({{kTop - 1, 2}}, 64));      // off + len wraps to 0
    CHECK(!xlzwin::disjoint_within({{kTop - 1, 2}}, kTop));    // ... also where the capacity is everything
    CHECK(xlzwin::disjoint_within({{kTop - 1, 1}}, kTop) && !xlzwin::disjoint_within({{kTop, 1}}, kTop));
    CHECK(!xlzwin::disjoint_within({{5, kTop - 4}}, 64) && !xlzwin::disjoint_within({{5, kTop}}, kTop));
    CHECK(xlzwin::disjoint_within({{0, 10}, {10, 10}, {20, 44}}, 64));   // windows that touch share nothing
    CHECK(!xlzwin::disjoint_within({{0, 10}, {9, 10}}, 64));             // the last byte of one is the first of the other
    CHECK(!xlzwin::disjoint_within({{8, 4}, {8, 4}}, 64) && !xlzwin::disjoint_within({{0, 64}, {20, 1}}, 64));
    CHECK(xlzwin::disjoint_within({{0, 64}, {20, 0}, {64, 0}, {0, 0}}, 64)); // windows of no bytes share nothing, wherever they are
    CHECK(!xlzwin::disjoint_within({{0, 40}, {10, 0}, {30, 24}}, 64));       // ... and hide no overlap of the others
    CHECK(xlzwin::disjoint_within({{30, 10}, {0, 10}, {10, 20}}, 40));       // in any order
    {
        uint64_t off[4], total = 0;
        const uint64_t sizes[4] = {5, 0, 3, 1};
        CHECK(xlzwin::back_to_back(sizes, 4, 4, off, &total) && off[0] == 0 && off[1] == 8 && off[2] == 8 && off[3] == 12 && total == 13);
        CHECK(xlzwin::back_to_back(sizes, 4, 1, off, &total) && off[1] == 5 && off[2] == 5 && off[3] == 8 && total == 9);
        CHECK(xlzwin::back_to_back(sizes, 0, 4, off, &total) && total == 0);
        const uint64_t big[4] = {1ull << 62, 1ull << 62, 1ull << 62, 1ull << 62};
        CHECK(!xlzwin::back_to_back(big, 4, 1, off, &total));  // the last end is 2^64
        const uint64_t most[4] = {1ull << 62, 1ull << 62, 1ull << 62, (1ull << 62) - 1};
        CHECK(xlzwin::back_to_back(most, 4, 1, off, &total) && total == kTop && off[3] == 3ull << 62);
        const uint64_t odd[2] = {kTop - 2, 1};
        CHECK(xlzwin::back_to_back(odd, 2, 1, off, &total) && total == kTop - 1);
        CHECK(!xlzwin::back_to_back(odd, 2, 4, off, &total));  // rounding the second offset up to 4 wraps
        const uint64_t two[2] = {1, 1};
        CHECK(xlzwin::back_to_back(two, 2, 1ull << 63, off, &total) && off[1] == 1ull << 63 && total == (1ull << 63) + 1);
        const uint64_t three[3] = {1, 1, 1};
        CHECK(!xlzwin::back_to_back(three, 3, 1ull << 63, off, &total)); // the third window would begin at 2^64
        CHECK(!xlzwin::back_to_back(two, 2, kTop, off, &total));         // an alignment of 2^64 - 1: the second offset fits, its end does not
        CHECK(xlzwin::back_to_back(two, 1, kTop, off, &total) && total == 1);
    }
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("ok\n");
    return 0;
}
