// xz_many_selftest.cpp -- lzma_amd/csrc/xlz_xz_many.h without a GPU, against byte-wise models.  The windows of a set of
// files: a destination in which every window marks its bytes says whether two share one or one does not fit.  The layout:
// the offsets against 128-bit sums, and the windows it makes marked in such a destination.  The map from (file, block) to
// the stream of the one batch against a count of everything in front.  The fold of per-block outcomes and check outcomes
// into a file's verdict against a list of every failure event, of which the earliest counts.  Seeded random file sets
// (files that never reach the batch, files without blocks, the same window twice, windows of no bytes anywhere).  Built
// plain and with the host sanitizers (tests/test_xz_many_cpu.py).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <tuple>

#include "xlz_xz_many.h"

static int fails = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            if (fails++ < 20) printf("%s:%d: %s\n", __FILE__, __LINE__, #c); \
        }                                                          \
    } while (0)

static const uint64_t kTop = ~(uint64_t)0;

// ---- windows: every window marks its bytes in a destination of `cap` bytes
static void windows_case(std::mt19937_64 &rnd)
{
    const uint64_t cap = rnd() % 200;
    const size_t n = rnd() % 7;
    std::vector<xlz_xz_many_file> f(n);
    bool well_formed = rnd() % 2; // half of the cases are laid out without a fault, with gaps, in any order
    uint64_t at = 0;
    for (size_t i = 0; i < n; i++) {
        f[i].file = nullptr, f[i].len = 0;
        if (well_formed) {
            at += rnd() % 4;
            f[i].dst_off = at, f[i].dst_cap = rnd() % 3 == 0 ? 0 : rnd() % 40;
            at += f[i].dst_cap;
        } else {
            const unsigned kind = (unsigned)(rnd() % 6);
            f[i].dst_off = kind == 0 ? kTop - rnd() % 4 : kind == 1 ? cap : rnd() % (cap + 3);
            f[i].dst_cap = kind == 2 ? 0 : kind == 3 ? kTop - rnd() % 4 : rnd() % (cap + 3);
            if (kind == 4 && i) f[i] = f[rnd() % i]; // the same window twice
        }
    }
    for (size_t i = n; i > 1; i--) std::swap(f[i - 1], f[rnd() % i]);
    std::vector<uint8_t> hits((size_t)cap, 0);
    bool ok = true;
    for (size_t i = 0; i < n; i++)
        for (uint64_t j = 0; j < f[i].dst_cap && ok; j++) {
            const unsigned __int128 pos = (unsigned __int128)f[i].dst_off + j;
            if (pos >= cap || hits[(size_t)pos]++)
                ok = false; // (the first fault settles it: a window of 2^64 bytes is not walked)
        }
    CHECK(xlzmany::windows_ok(f.data(), n, cap) == ok);
    if (well_formed) {
        CHECK(xlzmany::windows_ok(f.data(), n, at) && xlzmany::windows_ok(f.data(), n, kTop));
        uint64_t end = 0;
        for (size_t i = 0; i < n; i++)
            if (f[i].dst_cap) end = std::max(end, f[i].dst_off + f[i].dst_cap);
        CHECK(xlzmany::windows_ok(f.data(), n, end));
        if (end) CHECK(!xlzmany::windows_ok(f.data(), n, end - 1));
        // two windows that share ONE byte: y starts on x's last or first byte
        std::vector<size_t> full;
        for (size_t i = 0; i < n; i++)
            if (f[i].dst_cap) full.push_back(i);
        if (full.size() >= 2) {
            const size_t x = full[rnd() % full.size()];
            size_t y = full[rnd() % full.size()];
            if (y == x) y = full[0] == x ? full[1] : full[0];
            f[y].dst_off = f[x].dst_off + (rnd() % 2 ? f[x].dst_cap - 1 : 0);
            CHECK(!xlzmany::windows_ok(f.data(), n, kTop));
        }
    }
}

// ---- layout: 128-bit sums beside the header's, and the windows it makes are well formed and touch
static void layout_case(std::mt19937_64 &rnd)
{
    static const uint64_t kAligns[] = {1, 2, 3, 16, 256, 4096, 1ull << 40, 1ull << 63, kTop};
    const uint64_t align = rnd() % 4 == 0 ? 1 + rnd() % 1000 : kAligns[rnd() % (sizeof kAligns / sizeof kAligns[0])];
    const size_t n = rnd() % 8;
    const bool huge = rnd() % 4 == 0;
    std::vector<uint64_t> sizes(n), off(n, 12345);
    for (size_t i = 0; i < n; i++) sizes[i] = rnd() % 3 == 0 ? 0 : huge && rnd() % 2 ? (1ull << 62) - rnd() % 2 : rnd() % 5000;
    unsigned __int128 at = 0;
    bool fits = true;
    std::vector<unsigned __int128> want(n);
    for (size_t i = 0; i < n && fits; i++) {
        at = (at + align - 1) / align * align;
        want[i] = at;
        fits = at <= kTop;
        at += sizes[i];
        fits = fits && at <= kTop;
    }
    uint64_t total = 777;
    const bool got = xlzmany::layout(sizes.data(), n, align, off.data(), &total);
    CHECK(got == fits);
    if (!got || !fits) return;
    CHECK(total == (uint64_t)at);
    std::vector<xlz_xz_many_file> f(n);
    uint64_t prev_end = 0;
    for (size_t i = 0; i < n; i++) {
        CHECK(off[i] == (uint64_t)want[i] && off[i] % align == 0 && off[i] >= prev_end && off[i] - prev_end < align);
        f[i].file = nullptr, f[i].len = 0, f[i].dst_off = off[i], f[i].dst_cap = sizes[i];
        prev_end = off[i] + sizes[i];
    }
    CHECK(prev_end == total);
    CHECK(xlzmany::windows_ok(f.data(), n, total));
    bool any = false;
    for (uint64_t s : sizes) any |= s != 0;
    if (any && total) CHECK(!xlzmany::windows_ok(f.data(), n, total - 1) || sizes[n - 1] == 0);
}

// ---- map and fold
static void fold_case(std::mt19937_64 &rnd)
{
    const size_t n = rnd() % 9;
    std::vector<uint8_t> in_batch(n);
    std::vector<size_t> blocks(n);
    for (size_t i = 0; i < n; i++) in_batch[i] = rnd() % 4 != 0, blocks[i] = rnd() % 3 == 0 ? 0 : rnd() % 6;
    const xlzmany::Map m = xlzmany::map_streams(in_batch.data(), blocks.data(), n);
    // the stream of (file, block): everything in front of it, counted
    size_t streams = 0;
    for (size_t i = 0; i < n; i++) {
        if (!in_batch[i]) {
            CHECK(m.first[i] == xlzmany::kNotInBatch && m.count[i] == 0);
            continue;
        }
        CHECK(m.count[i] == blocks[i] && m.first[i] == streams);
        for (size_t k = 0; k < blocks[i]; k++) {
            size_t in_front = 0;
            for (size_t j = 0; j < i; j++) in_front += in_batch[j] ? blocks[j] : 0;
            CHECK(m.stream(i, k) == in_front + k);
            CHECK(m.stream(i, k) < m.file_of.size() && m.file_of[m.stream(i, k)] == i);
        }
        streams += blocks[i];
    }
    CHECK(m.file_of.size() == streams);
    // per stream: what the block did and what its check says
    static const int32_t kStatus[] = {XLZ_OK, XLZ_OK, XLZ_OK, XLZ_OK_INPUT_EOF, XLZ_ERR_RESULT, XLZ_ERR_UNEXPECTED_EOF, XLZ_ERR_OUT_CAP, XLZ_ERR_PROPS};
    const unsigned damage = (unsigned)(rnd() % 4); // 0: nothing fails; more: more does
    std::vector<int32_t> raw(streams), block_st(streams);
    std::vector<uint64_t> want_out(streams), want_in(streams), out_len(streams), in_used(streams);
    std::vector<uint8_t> check(streams);
    for (size_t s = 0; s < streams; s++) {
        raw[s] = damage && rnd() % (8 / damage) == 0 ? kStatus[rnd() % 8] : XLZ_OK;
        want_out[s] = rnd() % 1000, want_in[s] = 1 + rnd() % 1000;
        out_len[s] = damage && rnd() % (12 / damage) == 0 ? want_out[s] + 1 - 2 * (rnd() % 2) : want_out[s];
        in_used[s] = damage && rnd() % (12 / damage) == 0 ? want_in[s] - 1 : want_in[s];
        check[s] = damage && rnd() % (8 / damage) == 0 ? xlzmany::kCheckFailed : rnd() % 5 == 0 ? xlzmany::kCheckUnverified : xlzmany::kCheckGood;
        block_st[s] = xlzmany::block_status(raw[s], out_len[s], in_used[s], want_out[s], want_in[s]);
        const bool as_announced = out_len[s] == want_out[s] && in_used[s] == want_in[s];
        CHECK(block_st[s] == (raw[s] < 0 ? raw[s] : as_announced ? (int32_t)XLZ_OK : (int32_t)XLZ_ERR_RESULT));
    }
    for (int verify = 0; verify < 2; verify++)
        for (size_t i = 0; i < n; i++) {
            if (!in_batch[i]) continue;
            // every failure event of the file as (phase, block, status): the blocks' own come before any check's
            std::vector<std::tuple<int, size_t, int32_t>> events;
            uint32_t unverified = 0;
            for (size_t k = 0; k < blocks[i]; k++) {
                const size_t s = m.stream(i, k);
                if (raw[s] < 0)
                    events.emplace_back(0, k, raw[s]);
                else if (out_len[s] != want_out[s] || in_used[s] != want_in[s])
                    events.emplace_back(0, k, XLZ_ERR_RESULT);
                if (verify && check[s] == xlzmany::kCheckFailed) events.emplace_back(1, k, XLZ_ERR_RESULT);
                if (verify && check[s] == xlzmany::kCheckUnverified) unverified++;
            }
            std::sort(events.begin(), events.end());
            const xlzmany::Verdict v = xlzmany::fold(block_st.data(), check.data(), m.first[i], m.count[i], verify != 0);
            if (events.empty())
                CHECK(v.status == XLZ_OK && v.unverified == unverified);
            else
                CHECK(v.status == std::get<2>(events[0]) && v.unverified == 0);
        }
}

int main(int argc, char **argv)
{
    const int cases = argc > 1 ? atoi(argv[1]) : 20000;
    std::mt19937_64 rnd(20241019);
    // the layout, on its own
    {
        uint64_t sizes[4] = {5, 0, 7, 1}, off[4], total = 0;
        CHECK(xlzmany::layout(sizes, 4, 4, off, &total) && off[0] == 0 && off[1] == 8 && off[2] == 8 && off[3] == 16 && total == 17);
        CHECK(xlzmany::layout(sizes, 0, 4, off, &total) && total == 0);
        uint64_t big[4] = {1ull << 62, 1ull << 62, 1ull << 62, 1ull << 62};
        CHECK(!xlzmany::layout(big, 4, 1, off, &total));
        big[3] -= 1;
        CHECK(xlzmany::layout(big, 4, 1, off, &total) && total == kTop);
        uint64_t odd[2] = {kTop - 1, 0};
        CHECK(xlzmany::layout(odd, 2, 1, off, &total) && !xlzmany::layout(odd, 2, 4, off, &total));
    }
    for (int c = 0; c < cases; c++) windows_case(rnd), layout_case(rnd), fold_case(rnd);
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("%d cases ok\n", cases);
    return 0;
}
