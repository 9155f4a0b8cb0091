// xz_cover_selftest.cpp -- lzma_amd/csrc/xlz_xz_cover.h without a GPU: the cover of a list of ranges against a scan of
// every (range, block) pair, and the pack items a read is cut into against a byte-wise model that builds the destination by
// indexing the concatenated blocks.  Seeded random files (empty blocks, no blocks) and ranges (empty, at and behind the
// end, off + len past 2^64, on block boundaries, duplicates), destinations in any order with gaps, and destinations that
// overlap or do not fit, which must be refused.  Built plain and with the host sanitizers (tests/test_xz_ranges_cpu.py).
#include <cstdio>
#include <cstdlib>
#include <random>

#include "xlz_xz_cover.h"

using xlzcover::Extent;

static int fails = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            if (fails++ < 20) printf("%s:%d: %s\n", __FILE__, __LINE__, #c); \
        }                                                          \
    } while (0)

static uint8_t byte_of(size_t block, uint64_t j) { return (uint8_t)(block * 131 + j * 7 + (j >> 8)); }

static void one_case(std::mt19937_64 &rnd, bool fixed_file)
{
    // ---- the file
    static const uint64_t kFixed[] = {1, 15, 16, 17, 255, 256, 257, 4096, 16383, 16384, 16385, 70001, 33, 65536};
    std::vector<Extent> b;
    uint64_t size = 0;
    const size_t nb = fixed_file ? sizeof kFixed / sizeof kFixed[0] : rnd() % 13;
    for (size_t k = 0; k < nb; k++) {
        const uint64_t len = fixed_file ? kFixed[k] : rnd() % 4 == 0 ? 0 : 1 + rnd() % (rnd() % 2 ? 40 : 700);
        b.push_back(Extent{size, len});
        size += len;
    }
    std::vector<uint8_t> file; // the decoded file: the blocks one behind the other
    for (size_t k = 0; k < nb; k++)
        for (uint64_t j = 0; j < b[k].len; j++) file.push_back(byte_of(k, j));
    // ---- the ranges
    std::vector<uint64_t> marks = {0, size, size + 1, size + 1000, ~(uint64_t)0};
    for (const Extent &e : b)
        for (uint64_t v : {e.off, e.off + e.len})
            for (uint64_t d : {v - 1, v, v + 1})
                if (d <= size + 1) marks.push_back(d);
    const size_t n = rnd() % 9;
    std::vector<xlz_xz_range> r(n);
    for (size_t i = 0; i < n; i++) {
        const unsigned kind = (unsigned)(rnd() % 8);
        r[i].off = kind < 4 ? marks[rnd() % marks.size()] : size ? rnd() % size : 0;
        r[i].len = kind == 0 ? 0 : kind == 1 ? ~(uint64_t)0 - rnd() % 3 : kind == 2 ? marks[rnd() % marks.size()] - std::min(r[i].off, marks[rnd() % marks.size()]) : rnd() % (size + 2);
        if (kind == 3 && i) r[i] = r[rnd() % i]; // a duplicate (its destination is laid out anew below)
        if (kind == 2 && r[i].len > size + 5) r[i].len = rnd() % 3;
    }
    // ---- cover against the scan of every pair
    std::vector<size_t> brute;
    for (size_t k = 0; k < nb; k++) {
        bool hit = false;
        for (size_t i = 0; i < n; i++) {
            const uint64_t lo = std::min(r[i].off, size), hi = r[i].len > size - lo ? size : lo + r[i].len;
            hit |= std::max(lo, b[k].off) < std::min(hi, b[k].off + b[k].len);
        }
        if (hit) brute.push_back(k);
    }
    std::vector<size_t> got;
    xlzcover::cover(b.data(), nb, size, r.data(), n, got);
    CHECK(got == brute);
    // ---- destinations: one behind the other in a random order, with gaps
    std::vector<uint64_t> want(n);
    std::vector<size_t> order(n);
    for (size_t i = 0; i < n; i++) {
        const uint64_t lo = std::min(r[i].off, size);
        want[i] = r[i].len > size - lo ? size - lo : r[i].len;
        order[i] = i;
    }
    for (size_t i = n; i > 1; i--) std::swap(order[i - 1], order[rnd() % i]);
    uint64_t cap = rnd() % 5;
    for (size_t i : order) {
        r[i].dst_off = want[i] || rnd() % 2 ? cap : ~(uint64_t)0 - rnd() % 7; // (an empty range may point anywhere)
        cap += want[i] + rnd() % 4;
    }
    xlzcover::Plan p;
    CHECK(xlzcover::plan(b.data(), nb, size, r.data(), n, cap, p));
    CHECK(p.blocks == brute && p.lens == want);
    uint64_t total = 0;
    for (uint64_t w : want) total += w;
    CHECK(p.total == total);
    // the byte-wise model: range i's bytes are file[off ...]; 0x100 marks a byte nobody may write
    std::vector<uint16_t> model((size_t)cap, 0x100), dst((size_t)cap, 0x100);
    for (size_t i = 0; i < n; i++)
        for (uint64_t j = 0; j < want[i]; j++) model[(size_t)(r[i].dst_off + j)] = file[(size_t)(r[i].off + j)];
    uint64_t moved = 0;
    for (const xlz_pack_item &it : p.items) {
        CHECK(it.stream < p.blocks.size() && it.len > 0);
        if (it.stream >= p.blocks.size()) continue;
        const size_t k = p.blocks[(size_t)it.stream];
        CHECK(it.off < b[k].len && it.len <= b[k].len - it.off && it.dst_off <= cap && it.len <= cap - it.dst_off);
        if (!(it.off < b[k].len && it.len <= b[k].len - it.off && it.dst_off <= cap && it.len <= cap - it.dst_off)) continue;
        for (uint64_t j = 0; j < it.len; j++) {
            CHECK(dst[(size_t)(it.dst_off + j)] == 0x100); // every byte is written once
            dst[(size_t)(it.dst_off + j)] = byte_of(k, it.off + j);
        }
        moved += it.len;
    }
    CHECK(dst == model && moved == total);
    // ---- what must be refused: a destination one byte short, and two destinations that share a byte
    if (total) {
        uint64_t end = 0;
        for (size_t i = 0; i < n; i++)
            if (want[i]) end = std::max(end, r[i].dst_off + want[i]);
        CHECK(xlzcover::plan(b.data(), nb, size, r.data(), n, end, p));
        CHECK(!xlzcover::plan(b.data(), nb, size, r.data(), n, end - 1, p));
        std::vector<xlz_xz_range> far(r);
        bool wraps = false;
        for (size_t i = 0; i < n; i++)
            if (want[i] >= 2) far[i].dst_off = ~(uint64_t)0 - want[i] + 2, wraps = true; // dst_off + len wraps
        CHECK(!wraps || !xlzcover::plan(b.data(), nb, size, far.data(), n, ~(uint64_t)0, p));
    }
    std::vector<size_t> full;
    for (size_t i = 0; i < n; i++)
        if (want[i]) full.push_back(i);
    if (full.size() >= 2) {
        std::vector<xlz_xz_range> clash(r);
        const size_t x = full[rnd() % full.size()];
        size_t y = full[rnd() % full.size()];
        if (y == x) y = full[0] == x ? full[1] : full[0];
        clash[y].dst_off = clash[x].dst_off + (rnd() % 2 ? want[x] - 1 : 0); // y starts on x's last or first byte
        CHECK(!xlzcover::plan(b.data(), nb, size, clash.data(), n, ~(uint64_t)0, p));
    }
}

int main(int argc, char **argv)
{
    const int cases = argc > 1 ? atoi(argv[1]) : 4000;
    std::mt19937_64 rnd(20240607);
    // clip, on its own
    CHECK(xlzcover::clip(10, 3, 4) == std::make_pair((uint64_t)3, (uint64_t)7));
    CHECK(xlzcover::clip(10, 3, ~(uint64_t)0) == std::make_pair((uint64_t)3, (uint64_t)10));
    CHECK(xlzcover::clip(10, 10, 5) == std::make_pair((uint64_t)10, (uint64_t)10));
    CHECK(xlzcover::clip(10, ~(uint64_t)0, ~(uint64_t)0) == std::make_pair((uint64_t)10, (uint64_t)10));
    CHECK(xlzcover::clip(0, 0, 1) == std::make_pair((uint64_t)0, (uint64_t)0));
    for (int c = 0; c < cases; c++) one_case(rnd, c % 8 == 0);
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("%d cases ok\n", cases);
    return 0;
}
