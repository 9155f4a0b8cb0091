// The device checks' 64-lane scheme (lzma_amd/csrc/xlz_check_dev.h) run lane by lane on the CPU against a bit-by-bit
// CRC: what the kernels of xlz_check_dev.hip compute, without a GPU.  Prints "ok" and exits 0, or says what differs.
//   check_dev_selftest                        the built-in sweep
//   check_dev_selftest --list LIST ARENA OUT  the scheme over the ranges LIST names in the bytes of ARENA (list_mode below):
//                                             tests/test_digest_edges_cpu.py judges the digests in OUT
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "xlz_check_dev.h"

using namespace xlzchk;

template <int W> static uint64_t bitwise(const uint8_t *p, size_t n)
{
    uint64_t c = Crc<W>::ones;
    for (size_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (Crc<W>::poly & (0ull - (c & 1)));
    }
    return (c ^ Crc<W>::ones) & Crc<W>::ones;
}

template <int W> struct Scheme {
    Consts<W> c;
    std::vector<typename Crc<W>::tab_t> T;
    Scheme() : T(kTabEntries)
    {
        build_consts<W>(c);
        build_tables<W>(c, T.data());
    }
    // what the segment kernel and the fold kernel do for one range
    uint64_t range(const uint8_t *arena, uint64_t off, uint64_t len) const
    {
        const uint64_t m = range_segments(off, len);
        std::vector<uint64_t> v(m);
        for (uint64_t s = 0; s < m; s++) {
            const SegGeom g = seg_geom(off, len, s);
            uint64_t x = 0;
            for (uint32_t lane = 0; lane < kLanes; lane++)
                x ^= lane_finish<W>(c, seg_lane<W>(arena, g, off, off + len, lane, T.data()), lane);
            v[s] = seg_finish<W>(c, x, g.pad);
        }
        uint64_t F = 0;
        for (uint32_t t = 0; t < kFoldThreads; t++) F ^= fold_thread<W>(c, v.data(), m, t);
        return range_finish<W>(c, F, v.data(), m, off, len);
    }
};

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint8_t rnd8()
{
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return (uint8_t)(rng_state >> 32);
}

template <int W> static int run()
{
    static const Scheme<W> S;
    int bad = 0;
    // the published check values of "123456789"
    const uint8_t nine[] = "123456789";
    const uint64_t want9 = W == 32 ? 0xCBF43926ull : 0x995DC9BBDF1939FAull;
    std::vector<uint8_t> a(4096 + 16, 0xAA);
    memcpy(a.data() + 1024 + 5, nine, 9);
    if (S.range(a.data(), 1024 + 5, 9) != want9) bad++, printf("crc%d: check value of 123456789 differs\n", W);

    const size_t cap = (size_t)kSegBytes * (kFoldThreads + 4) + 4096;
    std::vector<uint8_t> arena(cap), other(cap);
    for (size_t i = 0; i < cap; i++) arena[i] = rnd8();
    auto one = [&](uint64_t off, uint64_t len, bool twice) {
        const uint64_t got = S.range(arena.data(), off, len), want = bitwise<W>(arena.data() + off, (size_t)len);
        if (got != want) {
            if (bad++ < 10) printf("crc%d: off %llu len %llu: %016llx, bit by bit %016llx\n", W, (unsigned long long)off,
                                   (unsigned long long)len, (unsigned long long)got, (unsigned long long)want);
            return;
        }
        if (twice) { // other bytes around the range: the digest must not see them
            for (size_t i = 0; i < cap; i++) other[i] = (i >= off && i < off + len) ? arena[i] : (uint8_t)~arena[i];
            if (S.range(other.data(), off, len) != want) {
                if (bad++ < 10) printf("crc%d: off %llu len %llu: bytes outside the range change the digest\n", W,
                                       (unsigned long long)off, (unsigned long long)len);
            }
        }
    };
    for (uint64_t align = 0; align < 16; align++)
        for (uint64_t len = 0; len <= 300; len++) one(256 + align, len, false);
    for (uint64_t align = 0; align < 16; align++) {
        const uint64_t off = 1024 + 112 + align; // (also: the last sixteen bytes of a 128-byte line)
        for (uint64_t len : {kRowBytes - 17, kRowBytes - 16, kRowBytes - 1, kRowBytes, kRowBytes + 1, kRowBytes + 16, 2 * kRowBytes,
                             4 * kRowBytes + 3, 5 * kRowBytes, kSegBytes - kRowBytes, kSegBytes - 129, kSegBytes - 128, kSegBytes - 1, kSegBytes,
                             kSegBytes + 1, kSegBytes + 127, kSegBytes + 128, 2 * kSegBytes - 1, 2 * kSegBytes, 2 * kSegBytes + 1,
                             3 * kSegBytes + 777})
            one(off, len, align % 5 == 0);
    }
    // a range that ends exactly where a segment does, and many segments: around one round of the fold's threads
    one(128, kSegBytes - 128 + kSegBytes, true);
    one(7, (uint64_t)kSegBytes * 7 + 12345, true);
    for (uint64_t segs : {kFoldThreads - 1, kFoldThreads, kFoldThreads + 1, kFoldThreads + 2, kFoldThreads + 3})
        one(3, (uint64_t)kSegBytes * segs - 3 + (segs % 2 ? 1 : 0) * 555, false);
    // the exported fold
    for (size_t n : {(size_t)0, (size_t)1, (size_t)1000, (size_t)70001})
        for (size_t cut : {(size_t)0, (size_t)1, n / 3, n}) {
            if (cut > n) continue;
            const uint64_t got = combine<W>(S.c, bitwise<W>(arena.data(), cut), bitwise<W>(arena.data() + cut, n - cut), n - cut);
            if (got != bitwise<W>(arena.data(), n)) bad++, printf("crc%d: combine at %zu of %zu differs\n", W, cut, n);
        }
    return bad;
}

// --list: one range per line of LIST, "KIND OFF LEN" (KIND 1 = CRC32, 4 = CRC64; OFF + LEN inside ARENA), through
// Scheme::range; OUT receives eight bytes per line, the digest zero-extended, little-endian
static int list_mode(const char *list_path, const char *arena_path, const char *out_path)
{
    std::vector<uint8_t> arena;
    FILE *f = fopen(arena_path, "rb");
    if (!f) return 2;
    if (fseek(f, 0, SEEK_END) != 0) return 2;
    const long size = ftell(f);
    if (size < 0 || fseek(f, 0, SEEK_SET) != 0) return 2;
    arena.resize((size_t)size);
    if (size && fread(arena.data(), 1, arena.size(), f) != arena.size()) return 2;
    fclose(f);
    FILE *list = fopen(list_path, "r"), *out = fopen(out_path, "wb");
    if (!list || !out) return 2;
    static const Scheme<32> S32;
    static const Scheme<64> S64;
    unsigned long kind;
    unsigned long long off, len;
    while (fscanf(list, "%lu %llu %llu", &kind, &off, &len) == 3) {
        if ((kind != 1 && kind != 4) || off > arena.size() || len > arena.size() - off) return 2;
        const uint64_t d = kind == 1 ? S32.range(arena.data(), off, len) : S64.range(arena.data(), off, len);
        uint8_t b[8];
        for (int k = 0; k < 8; k++) b[k] = (uint8_t)(d >> (8 * k));
        if (fwrite(b, 1, 8, out) != 8) return 2;
    }
    const bool all_read = feof(list) != 0;
    fclose(list);
    return fclose(out) == 0 && all_read ? 0 : 2;
}

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "--list")) return list_mode(argv[2], argv[3], argv[4]);
    if (argc != 1) {
        printf("usage: check_dev_selftest [--list LIST ARENA OUT]\n");
        return 2;
    }
    const int bad = run<32>() + run<64>();
    if (bad) {
        printf("%d differences\n", bad);
        return 1;
    }
    printf("ok\n");
    return 0;
}
