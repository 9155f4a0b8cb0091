// The device Adler-32's 64-lane scheme (lzma_amd/csrc/xlz_adler_dev.h) run lane by lane on the CPU: what the kernels of
// xlz_adler_dev.hip compute, without a GPU.  Prints "ok" and exits 0, or says what differs.
//   adler_dev_selftest                        the built-in sweep, against a byte-by-byte Adler-32 with a modulo per byte
//   adler_dev_selftest --list LIST ARENA OUT  the scheme over the ranges LIST names ("off len" per line) in the bytes of
//                                             ARENA; one digest per line, in hex, goes to OUT (tests/test_adler_dev.py
//                                             judges them with zlib.adler32).  Every range is ALSO run over a heap copy
//                                             of exactly its bytes, so that a sanitizer build sees a load outside a range.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "xlz_adler_dev.h"

using namespace xlzadl;

static uint32_t bytewise(const uint8_t *p, size_t n)
{
    uint32_t a = 1, b = 0;
    for (size_t i = 0; i < n; i++) a = (a + p[i]) % kMod, b = (b + a) % kMod;
    return b << 16 | a;
}

// what the segment kernel and the fold kernel do for one range of `buf`
static uint32_t scheme(const uint8_t *buf, uint64_t off, uint64_t len)
{
    if (!len) return 1; // (the host settles an empty range: it never reaches the kernels)
    const uint64_t m = range_segments(off, len);
    std::vector<uint32_t> v(m);
    for (uint64_t s = 0; s < m; s++) {
        const SegGeom g = seg_geom(off, len, s);
        uint32_t s_sum = 0, b_sum = 0;
        for (uint32_t lane = 0; lane < kLanes; lane++) {
            const LanePart p = lane_finish(seg_lane(buf, g, off, off + len, lane), lane);
            s_sum += p.s, b_sum += p.b;
        }
        v[s] = seg_finish(s_sum, b_sum, (uint32_t)(seg_end(off, len, s, m) - seg_begin(off, s)), g.pad);
    }
    uint32_t a = 0, b = 0;
    for (uint32_t t = 0; t < kFoldThreads; t++) {
        const FoldPart p = fold_thread(v.data(), m, off, len, t);
        a += p.a, b += p.b;
    }
    return range_finish(a, b);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint8_t rnd8()
{
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return (uint8_t)(rng_state >> 32);
}

static bool read_file(const char *path, std::vector<uint8_t> &out)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint8_t tmp[1 << 16];
    for (size_t k; (k = fread(tmp, 1, sizeof tmp, f)) > 0;) out.insert(out.end(), tmp, tmp + k);
    fclose(f);
    return true;
}

static int list_mode(const char *list, const char *arena_path, const char *out_path)
{
    std::vector<uint8_t> arena;
    FILE *l = fopen(list, "r"), *o = fopen(out_path, "w");
    if (!l || !o || !read_file(arena_path, arena)) return printf("cannot open the files\n"), 2;
    unsigned long long off, len;
    int bad = 0;
    while (fscanf(l, "%llu %llu", &off, &len) == 2) {
        if (off > arena.size() || len > arena.size() - off) return printf("range %llu + %llu leaves the arena\n", off, len), 2;
        const uint32_t got = scheme(arena.data(), off, len);
        // the same range where nothing else may be touched: a heap block of exactly its bytes, its first byte at an address
        // congruent to `off` modulo 128 as far as the scheme can tell (it only forms offsets)
        uint8_t *exact = static_cast<uint8_t *>(malloc(len ? (size_t)len : 1));
        if (len) memcpy(exact, arena.data() + off, (size_t)len);
        const uint64_t shift = off % 128;
        const uint32_t again = scheme(reinterpret_cast<const uint8_t *>((uintptr_t)exact - (uintptr_t)shift), shift, len);
        free(exact);
        if (again != got) bad++, printf("range %llu + %llu: %08x in the arena, %08x alone\n", off, len, got, again);
        fprintf(o, "%08x\n", got);
    }
    fclose(l), fclose(o);
    if (bad) return 1;
    printf("ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "--list")) return list_mode(argv[2], argv[3], argv[4]);
    int bad = 0;
    const size_t cap = (size_t)kSegBytes * 4 + 4096;
    std::vector<uint8_t> arena(cap);
    for (size_t i = 0; i < cap; i++) arena[i] = rnd8();
    auto one = [&](const std::vector<uint8_t> &a, uint64_t off, uint64_t len) {
        const uint32_t got = scheme(a.data(), off, len), want = bytewise(a.data() + off, (size_t)len);
        if (got != want && bad++ < 10) printf("off %llu len %llu: %08x, byte by byte %08x\n", (unsigned long long)off, (unsigned long long)len, got, want);
    };
    const uint64_t lens[] = {0, 1, 2, 15, 16, 17, 31, 127, 128, 129, 1023, 1024, 1025, 5552, kSegBytes - 1, kSegBytes, kSegBytes + 1, 3 * kSegBytes + 1};
    for (uint64_t len : lens)
        for (uint64_t off = 0; off < 130; off += (off < 17 || off > 125) ? 1 : 13) one(arena, off, len);
    std::vector<uint8_t> ff(cap, 0xFF), zero(cap, 0);
    for (uint64_t len : lens) one(ff, 3, len), one(zero, 5, len), one(ff, 0, len);
    // "Wikipedia" -> 0x11E60398 (the example everybody quotes)
    const uint8_t w[] = "Wikipedia";
    memcpy(arena.data() + 1000, w, 9);
    if (scheme(arena.data(), 1000, 9) != 0x11E60398u) bad++, printf("the digest of \"Wikipedia\" differs\n");
    // the host's serial digest and the combine rule
    for (int k = 0; k < 200; k++) {
        const size_t n = (size_t)rnd8() * 97 + rnd8(), cut = n ? ((size_t)rnd8() * 131) % (n + 1) : 0;
        const uint32_t whole = host_update(1, arena.data(), n), x = host_update(1, arena.data(), cut), y = host_update(1, arena.data() + cut, n - cut);
        if (whole != bytewise(arena.data(), n) || combine(x, y, n - cut) != whole || host_update(x, arena.data() + cut, n - cut) != whole)
            if (bad++ < 10) printf("host: n %zu cut %zu differs\n", n, cut);
    }
    if (bad) return printf("%d failures\n", bad), 1;
    printf("ok\n");
    return 0;
}
