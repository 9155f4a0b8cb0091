// pack_dev_selftest.cpp -- the tile / lane scheme of lzma_amd/csrc/xlz_pack_dev.h on the CPU, against memcpy per item.
// Plain C++ (g++ -Wall -Werror, no GPU): every tile of a launch, its 256 lanes one by one (ascending for even tiles,
// descending for odd ones: no lane may depend on another), into a destination pre-filled with a sentinel; the whole
// destination is compared, so a byte outside the items that was touched fails too.  The header's load helper asserts
// that every aligned load stays inside the arena, which is laid out as the library lays it out and has NO pad of its own
// behind the last region here.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "xlz_pack_dev.h"
#include "xlz_post.h"

using namespace xlzpack;

namespace {

constexpr uint8_t kSentinel = 0xA5;
uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

struct Arena {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> region; // first byte of each stream's region
    explicit Arena(const std::vector<uint64_t> &caps)
    {
        uint64_t at = 0;
        for (uint64_t c : caps) region.push_back(at), at += region_bytes(c);
        bytes.resize((size_t)at);
        for (auto &b : bytes) b = (uint8_t)rnd();
    }
};

int failures = 0;

// items: any order, empty ones allowed (dropped as the host drops them); dst_bytes: size of the destination
void run(const char *what, const Arena &A, std::vector<DevItem> items, uint64_t dst_bytes)
{
    items.erase(std::remove_if(items.begin(), items.end(), [](const DevItem &i) { return i.len == 0; }), items.end());
    std::sort(items.begin(), items.end(), [](const DevItem &a, const DevItem &b) { return a.dst < b.dst; });
    std::vector<uint8_t> want((size_t)dst_bytes, kSentinel), got((size_t)dst_bytes, kSentinel);
    for (size_t i = 0; i < items.size(); i++) {
        if (items[i].dst + items[i].len > dst_bytes || (i && items[i - 1].dst + items[i - 1].len > items[i].dst)) {
            printf("%s: bad test table\n", what);
            failures++;
            return;
        }
        memcpy(want.data() + items[i].dst, A.bytes.data() + items[i].src, (size_t)items[i].len);
    }
    if (!items.empty()) {
        const uint32_t n = (uint32_t)items.size();
        const uint64_t t0 = first_tile(items.data()), nt = tile_count(items.data(), n);
        for (uint64_t t = 0; t < nt; t++)
            for (uint32_t l = 0; l < kThreads; l++)
                tile_lane(A.bytes.data(), A.bytes.size(), got.data(), items.data(), n, t0 + t, (t & 1) ? kThreads - 1 - l : l);
    }
    if (got != want) {
        size_t at = 0;
        while (got[at] == want[at]) at++;
        printf("%s: byte %zu is %02x, expected %02x\n", what, at, got[at], want[at]);
        failures++;
    }
}

// --pack-list LIST: tables somebody else made (tests/pack_edges.py), as Batch.pack takes them.  LIST holds, per table, a line
// "STREAMS ITEMS DST_CAP MIS", the STREAMS sizes of the streams and ITEMS lines "STREAM OFF LEN DST_OFF".  The arena is laid
// out as the library lays it out; the destination is MIS + DST_CAP bytes and 64 guard bytes from a multiple of 16 on, the
// caller's pointer MIS behind its first byte: every tile of the launch, against memcpy per item, the whole of it compared.
int pack_list(const char *path)
{
    FILE *f = fopen(path, "r");
    if (!f) return 2;
    unsigned long long n_streams, n_items, dst_cap, mis;
    int tables = 0;
    while (fscanf(f, "%llu %llu %llu %llu", &n_streams, &n_items, &dst_cap, &mis) == 4) {
        if (mis > 15) return 2;
        std::vector<uint64_t> caps;
        for (unsigned long long k = 0, c; k < n_streams; k++) {
            if (fscanf(f, "%llu", &c) != 1) return 2;
            caps.push_back(c);
        }
        const Arena A(caps);
        std::vector<DevItem> items;
        for (uint64_t i = 0; i < n_items; i++) {
            unsigned long long s, off, len, dst;
            if (fscanf(f, "%llu %llu %llu %llu", &s, &off, &len, &dst) != 4 || s >= n_streams || off > caps[s] || len > caps[s] - off) return 2;
            items.push_back(DevItem{A.region[s] + off, dst + mis, len});
        }
        char what[48];
        snprintf(what, sizeof what, "table %d (mis %llu)", tables++, mis);
        run(what, A, items, mis + dst_cap + 64);
    }
    fclose(f);
    printf("%d tables, %d failures\n", tables, failures);
    return failures ? 3 : 0;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "--pack-list")) return pack_list(argv[2]);
    // every (source mod 16, destination mod 16) pair x lengths 0-48: each alone, and all of a length in one table
    {
        Arena A({4096});
        for (uint32_t len = 0; len <= 48; len++) {
            std::vector<DevItem> all;
            for (uint32_t s = 0; s < 16; s++)
                for (uint32_t d = 0; d < 16; d++) {
                    const DevItem it = {256 + s + 64 * d, 16384 - 24 + d, len}; // (across a tile boundary for most lengths)
                    run("pair alone", A, {it}, 2 * 16384);
                    all.push_back(DevItem{it.src, (uint64_t)(s * 16 + d) * 80 + d, len});
                }
            run("pairs together", A, all, 256 * 80 + 64);
        }
    }
    // lengths around one and two tiles, at several alignments and places in a tile
    {
        Arena A({70000});
        for (uint64_t base : {16384ull, 32768ull})
            for (int dl = -5; dl <= 5; dl++)
                for (uint32_t s : {0u, 1u, 7u, 8u, 9u, 15u})
                    for (uint64_t d : {0ull, 3ull, 15ull, 16379ull, 16384ull + 8, 5ull * 16384 - 1})
                        run("tile lengths", A, {DevItem{s, d, base + dl}}, 8 * 16384);
    }
    // items that start in the last 1-17 bytes of a tile
    {
        Arena A({40000});
        for (uint32_t k = 1; k <= 17; k++)
            for (uint64_t len : std::vector<uint64_t>{1, k - 1, k, k + 1, 40, 20000})
                for (uint32_t s : {0u, 5u, 11u})
                    run("tile end", A, {DevItem{512 + s, 3 * 16384 - k, len}, DevItem{s, 100, 37}}, 6 * 16384);
    }
    // 40 items of 1-7 bytes inside one tile: back to back, and with gaps
    {
        Arena A({4096});
        for (int gaps = 0; gaps < 2; gaps++)
            for (int rep = 0; rep < 50; rep++) {
                std::vector<DevItem> v;
                uint64_t d = 16384 + rnd() % 4000;
                for (int i = 0; i < 40; i++) {
                    const uint64_t len = 1 + rnd() % 7;
                    v.push_back(DevItem{rnd() % 4000, d, len});
                    d += len + (gaps ? rnd() % 5 : 0);
                }
                std::reverse(v.begin(), v.end());
                run("small items", A, v, 2 * 16384);
            }
    }
    // the arena's first and last region: items from a region's first byte and up to its last one, every destination
    // alignment (the bounds assertion of load16 is what is under test; the arena ends with its last region)
    for (uint64_t cap : {1ull, 15ull, 16ull, 17ull, 33ull, 191ull, 192ull, 193ull, 255ull, 256ull, 257ull, 4097ull, 16384ull + 200}) {
        Arena A({cap, 300, cap});
        for (size_t reg : {(size_t)0, (size_t)2})
            for (uint32_t d = 0; d < 16; d++) {
                run("region whole", A, {DevItem{A.region[reg], 32 + d, cap}}, 3 * 16384);
                for (uint64_t len = 1; len <= 48 && len <= cap; len++) {
                    run("region end", A, {DevItem{A.region[reg] + cap - len, 16384 - 20 + d, len}}, 2 * 16384);
                    run("region start", A, {DevItem{A.region[reg], 7 + d, len}}, 16384);
                }
            }
    }
    // a table of many items of mixed sizes, shuffled
    {
        std::vector<uint64_t> caps;
        for (int i = 0; i < 64; i++) caps.push_back(rnd() % 3 ? rnd() % 300 : rnd() % 50000);
        Arena A(caps);
        std::vector<DevItem> v;
        uint64_t d = 5;
        for (int i = 0; i < 64; i++) {
            const uint64_t off = caps[i] ? rnd() % caps[i] : 0, len = caps[i] - off;
            v.push_back(DevItem{A.region[i] + off, d, len});
            d += len + (rnd() % 4 == 0 ? rnd() % 40 : 0);
        }
        for (size_t i = v.size(); i > 1; i--) std::swap(v[i - 1], v[rnd() % i]);
        run("mixed", A, v, d + 100);
    }
    // what xlz_batch_pack accepts as a table (xlz_post.h: pack_items_ok)
    {
        auto ok = [](std::vector<xlz_pack_item> v, size_t streams, uint64_t cap) { return xlzpost::pack_items_ok(v.data(), v.size(), streams, cap); };
        const uint64_t top = ~(uint64_t)0;
        const bool good = ok({}, 0, 0) && ok({{0, 0, 10, 0}, {1, 5, 10, 10}}, 2, 20) && ok({{0, 0, 10, 10}, {0, 0, 10, 0}}, 1, 20) &&
                          ok({{0, 0, 0, 20}, {0, 0, 20, 0}, {0, 7, 0, 5}}, 1, 20) && ok({{0, top, top, 0}}, 1, top);
        const bool bad = ok({{2, 0, 1, 0}}, 2, 20) || ok({{0, 0, 11, 10}}, 1, 20) || ok({{0, 0, 1, 21}}, 1, 20) || ok({{0, 0, top, 2}}, 1, top) ||
                         ok({{0, 0, 10, 0}, {0, 0, 10, 9}}, 1, 20) || ok({{0, 0, 4, 8}, {0, 0, 20, 0}}, 1, 20) || ok({{0, 0, 0, 21}}, 1, 20);
        if (!good || bad) {
            printf("pack_items_ok: good %d bad %d\n", (int)good, (int)bad);
            failures++;
        }
    }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
