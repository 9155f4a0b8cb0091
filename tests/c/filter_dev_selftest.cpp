// filter_dev_selftest.cpp -- runs the device scheme of the filters (lzma_amd/csrc/xlz_filter_dev.h) on the CPU, lane by
// lane, window by window and chunk by chunk, the way the kernels of xlz_filter_dev.hip drive it, and compares every result
// with the serial twin host_apply() (which tests/test_filter_dev.py compares with liblzma).
//
//   filter_dev_selftest            seeded buffers: text, random, zeros, dense opcodes, adversarial x86; lengths 0-40 and
//                                  around every tile / window / chunk size; all start offsets and distances
//   filter_dev_selftest FILE ...   the same filters over the bytes of the given files (machine code)
//   filter_dev_selftest --apply ID PARAM IN OUT   the lane scheme of one step over a file, written to OUT
//   filter_dev_selftest --apply-list LIST IN OUT  the same for many buffers laid end to end in IN: LIST holds a line
//                                  "ID PARAM LENGTH" per buffer, OUT receives the results end to end
// Both --apply forms run a fixed-width BCJ step three times: lanes last to first on the bytes as they stand, and with
// every lane's loads taken BEFORE any lane's store (what lanes that run at the same time see), stores first to last and
// last to first.  The three must agree (exit status 3 if not).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "xlz_filter_dev.h"

using namespace xlzflt;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

// ---- the kernels, one "lane" at a time.  Lanes run in an order the device never promises: last to first. ----
static void dev_bcj(uint32_t id, uint32_t param, std::vector<uint8_t> &v)
{
    uint8_t *buf = v.data();
    const uint64_t len = v.size(), chunks = (len + 15) / 16;
    for (uint64_t c = chunks; c-- > 0;) {
        const uint64_t pos = c * 16, left = len - pos;
        const uint32_t whole = left < 16 ? (uint32_t)left : 16u;
        uint32_t w[4] = {0, 0, 0, 0};
        memcpy(w, buf + pos, whole);
        uint32_t flags = 0, next_out = 0;
        if (id == kARMThumb) {
            const uint32_t prev_h = pos ? ((uint32_t)buf[pos - 2] | (uint32_t)buf[pos - 1] << 8) : 0u;
            const uint32_t next_h = left >= 18 ? ((uint32_t)buf[pos + 16] | (uint32_t)buf[pos + 17] << 8) : 0u;
            flags = thumb_chunk16(param + (uint32_t)pos, w, left >= 18 ? 18u : whole, prev_h, next_h, &next_out);
        } else {
            bcj_chunk16(id, param + (uint32_t)pos, w, whole);
        }
        const uint32_t lo = (flags & 1) ? 2u : 0u;
        if (whole > lo) memcpy(buf + pos + lo, (const uint8_t *)w + lo, whole - lo);
        if (flags & 2) buf[pos + 16] = (uint8_t)next_out, buf[pos + 17] = (uint8_t)(next_out >> 8);
    }
}
// the same in ascending order: both orders must agree
static void dev_bcj_forward(uint32_t id, uint32_t param, std::vector<uint8_t> &v)
{
    uint8_t *buf = v.data();
    const uint64_t len = v.size(), chunks = (len + 15) / 16;
    for (uint64_t c = 0; c < chunks; c++) {
        const uint64_t pos = c * 16, left = len - pos;
        const uint32_t whole = left < 16 ? (uint32_t)left : 16u;
        uint32_t w[4] = {0, 0, 0, 0};
        memcpy(w, buf + pos, whole);
        uint32_t flags = 0, next_out = 0;
        if (id == kARMThumb) {
            const uint32_t prev_h = pos ? ((uint32_t)buf[pos - 2] | (uint32_t)buf[pos - 1] << 8) : 0u;
            const uint32_t next_h = left >= 18 ? ((uint32_t)buf[pos + 16] | (uint32_t)buf[pos + 17] << 8) : 0u;
            flags = thumb_chunk16(param + (uint32_t)pos, w, left >= 18 ? 18u : whole, prev_h, next_h, &next_out);
        } else {
            bcj_chunk16(id, param + (uint32_t)pos, w, whole);
        }
        const uint32_t lo = (flags & 1) ? 2u : 0u;
        if (whole > lo) memcpy(buf + pos + lo, (const uint8_t *)w + lo, whole - lo);
        if (flags & 2) buf[pos + 16] = (uint8_t)next_out, buf[pos + 17] = (uint8_t)(next_out >> 8);
    }
}
// every lane loads (its chunk and the halfwords beside it) before any lane stores; stores in ascending or descending order
static void dev_bcj_snapshot(uint32_t id, uint32_t param, std::vector<uint8_t> &v, bool ascending)
{
    const std::vector<uint8_t> orig = v;
    const uint8_t *src = orig.data();
    uint8_t *buf = v.data();
    const uint64_t len = v.size(), chunks = (len + 15) / 16;
    for (uint64_t q = 0; q < chunks; q++) {
        const uint64_t c = ascending ? q : chunks - 1 - q;
        const uint64_t pos = c * 16, left = len - pos;
        const uint32_t whole = left < 16 ? (uint32_t)left : 16u;
        uint32_t w[4] = {0, 0, 0, 0};
        memcpy(w, src + pos, whole);
        uint32_t flags = 0, next_out = 0;
        if (id == kARMThumb) {
            const uint32_t prev_h = pos ? ((uint32_t)src[pos - 2] | (uint32_t)src[pos - 1] << 8) : 0u;
            const uint32_t next_h = left >= 18 ? ((uint32_t)src[pos + 16] | (uint32_t)src[pos + 17] << 8) : 0u;
            flags = thumb_chunk16(param + (uint32_t)pos, w, left >= 18 ? 18u : whole, prev_h, next_h, &next_out);
        } else {
            bcj_chunk16(id, param + (uint32_t)pos, w, whole);
        }
        const uint32_t lo = (flags & 1) ? 2u : 0u;
        if (whole > lo) memcpy(buf + pos + lo, (const uint8_t *)w + lo, whole - lo);
        if (flags & 2) buf[pos + 16] = (uint8_t)next_out, buf[pos + 17] = (uint8_t)(next_out >> 8);
    }
}
static void dev_x86(uint32_t param, std::vector<uint8_t> &v)
{
    const uint64_t len = v.size(), n_win = x86_windows(len);
    std::vector<uint16_t> sync(n_win + 1);
    for (uint64_t j = 0; j < n_win; j++) sync[j] = x86_first_sync(v.data(), len, j); // first launch: on the original bytes
    for (uint64_t j = n_win; j-- > 0;) x86_lane(v.data(), len, param, sync.data(), n_win, j);
}
static void dev_delta(uint32_t d, std::vector<uint8_t> &v)
{
    const uint64_t len = v.size(), chunks = delta_chunks(len);
    std::vector<uint8_t> sums(chunks * kDeltaMaxDist + 1, 0xA5);
    std::vector<uint32_t> x(kDeltaWords), nx(kDeltaWords);
    // first launch: the column sums of every chunk but the last
    for (uint64_t c = 0; c + 1 < chunks; c++) {
        const uint64_t P = c * kDeltaChunk;
        memcpy(x.data(), v.data() + P, kDeltaChunk);
        uint32_t n = kDeltaChunk;
        while (n > d) {
            const uint32_t h = delta_fold_at(n, d), words = (n - h + 3) / 4;
            for (uint32_t j = 0; j < words; j++) nx[j] = delta_fold_word(x.data(), n, h, j);
            for (uint32_t j = 0; j < words; j++) x[j] = nx[j];
            n = h;
        }
        for (uint32_t k = 0; k < d; k++) sums[c * kDeltaMaxDist + (uint32_t)((P + k) % d)] = (uint8_t)(x[k >> 2] >> (8 * (k & 3)));
    }
    // second launch, two levels: inside groups of chunks (groups in descending order), then over the groups' totals
    const uint64_t groups = delta_groups(chunks);
    std::vector<uint8_t> gsums(groups * kDeltaMaxDist + 1, 0x5A);
    for (uint64_t g = groups; g-- > 0;)
        for (uint32_t r = 0; r < d; r++) delta_group_scan(sums.data(), gsums.data() + g * kDeltaMaxDist, (uint32_t)chunks, (uint32_t)g, r);
    for (uint32_t r = 0; r < d; r++) delta_groups_scan(gsums.data(), (uint32_t)groups, r);
    // third launch: chunks in descending order
    for (uint64_t c = chunks; c-- > 0;) {
        const uint64_t P = c * kDeltaChunk;
        const uint32_t n = len - P < kDeltaChunk ? (uint32_t)(len - P) : kDeltaChunk;
        std::fill(x.begin(), x.end(), 0u);
        memcpy(x.data(), v.data() + P, n);
        if (c)
            for (uint32_t t = 0; 4 * t < d; t++) {
                uint32_t carry = 0;
                for (uint32_t b = 0; b < 4; b++) {
                    const uint32_t k = 4 * t + b;
                    if (k < d) carry |= (delta_carry(sums.data(), gsums.data(), (uint32_t)c, (uint32_t)((P + k) % d)) & 0xFF) << (8 * b);
                }
                x[t] = add_bytes(x[t], carry);
            }
        for (uint32_t s = d; s < n; s *= 2) {
            for (uint32_t j = 0; j < kDeltaWords; j++) nx[j] = delta_scan_word(x.data(), s, j);
            x = nx;
        }
        memcpy(v.data() + P, x.data(), n);
    }
}
static void dev_apply(uint32_t id, uint32_t param, std::vector<uint8_t> &v)
{
    if (id == kDelta) dev_delta(param, v);
    else if (id == kX86) dev_x86(param, v);
    else dev_bcj(id, param, v);
}

// --apply: the scheme in every order it is restated in; false when the orders disagree
static bool dev_apply_all_orders(uint32_t id, uint32_t param, std::vector<uint8_t> &v)
{
    if (id == kDelta || id == kX86) {
        dev_apply(id, param, v);
        return true;
    }
    std::vector<uint8_t> up = v, down = v;
    dev_bcj(id, param, v);
    dev_bcj_snapshot(id, param, up, true);
    dev_bcj_snapshot(id, param, down, false);
    if (up == v && down == v) return true;
    v = up != v ? up : down; // (the caller's judge sees the bytes that differ)
    return false;
}
static bool read_file(const char *path, std::vector<uint8_t> &v)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint8_t tmp[65536];
    size_t got;
    while ((got = fread(tmp, 1, sizeof tmp, f)) > 0) v.insert(v.end(), tmp, tmp + got);
    fclose(f);
    return true;
}

static long n_cases = 0, n_changed = 0;
static bool check(uint32_t id, uint32_t param, const std::vector<uint8_t> &in, const char *what)
{
    std::vector<uint8_t> a = in, b = in;
    host_apply(id, param, a.data(), a.size());
    dev_apply(id, param, b);
    n_cases++;
    n_changed += a != in;
    bool ok = a == b;
    if (ok && id != kDelta && id != kX86) {
        std::vector<uint8_t> c = in;
        dev_bcj_forward(id, param, c);
        ok = a == c;
    }
    if (!ok) {
        size_t at = 0;
        while (at < a.size() && a[at] == b[at]) at++;
        printf("MISMATCH %s: filter %u param %u len %zu, first at %zu\n", what, id, param, in.size(), at);
    }
    return ok;
}

static const uint32_t kOffsets[3] = {0, 4096, 0xFFFFFFF0u};
static const uint32_t kDists[8] = {1, 2, 3, 4, 7, 16, 255, 256};

static bool all_filters(const std::vector<uint8_t> &in, const char *what)
{
    bool ok = true;
    for (uint32_t id = kDelta; id <= kSPARC; id++)
        for (uint32_t p = 0; p < (id == kDelta ? 8u : 3u); p++) ok &= check(id, id == kDelta ? kDists[p] : kOffsets[p], in, what);
    return ok;
}

// bytes in which every filter finds work: opcodes of all seven at random places
static std::vector<uint8_t> opcode_soup(size_t n, uint32_t density)
{
    std::vector<uint8_t> v(n);
    for (auto &b : v) b = (uint8_t)rnd();
    for (size_t i = 0; i + 16 <= n; i += 4) {
        if (rnd() % 100 >= density) continue;
        switch (rnd() % 8) {
        case 0: v[i + 3] = 0xEB; break;
        case 1: v[i] = 0x48 | (v[i] & 3), v[i + 3] = (v[i + 3] & ~3) | 1; break;
        case 2: v[i] = 0x40, v[i + 1] &= 0x3F; break;
        case 3: v[i] = 0x7F, v[i + 1] |= 0xC0; break;
        case 4: v[i + 1] = 0xF0 | (v[i + 1] & 7), v[i + 3] = 0xF8 | (v[i + 3] & 7); break;
        case 5: v[i + 3] = 0xF0 | (v[i + 3] & 7), v[i + 5] = 0xF8 | (v[i + 5] & 7); break; // a pair at 2 mod 4
        case 6: v[i] = (rnd() & 1) ? 0xE8 : 0xE9, v[i + 4] = (rnd() & 1) ? 0x00 : 0xFF; break;
        default: {
            const size_t bnd = i & ~(size_t)15;
            static const uint8_t t[10] = {16, 17, 18, 19, 22, 23, 24, 25, 28, 29};
            uint8_t raw[16];
            memcpy(raw, &v[bnd], 16);
            unsigned __int128 x;
            memcpy(&x, raw, 16);
            x = (x & ~(unsigned __int128)0x1F) | t[rnd() % 10];
            for (int slot = 0; slot < 3; slot++) {
                const int at = 5 + 41 * slot;
                x &= ~(((unsigned __int128)0xF << 37 | (unsigned __int128)0x7 << 9) << at);
                x |= ((unsigned __int128)0x5 << 37) << at;
            }
            memcpy(&v[bnd], &x, 16);
        }
        }
    }
    return v;
}
static std::vector<uint8_t> x86_adversarial(size_t n, uint32_t density_percent, bool runs)
{
    std::vector<uint8_t> v(n);
    for (size_t i = 0; i < n; i++) {
        const uint32_t r = rnd();
        if (r % 100 < density_percent) v[i] = (r & 0x100) ? 0xE8 : 0xE9;
        else v[i] = (r & 0x600) == 0 ? 0x00 : (r & 0x600) == 0x200 ? 0xFF : (uint8_t)(r >> 11);
    }
    if (runs)
        for (size_t i = 0; i + 700 < n; i += 1500) memset(&v[i], (i / 1500) & 1 ? 0xE9 : 0xE8, 300 + (rnd() % 400));
    return v;
}
static std::vector<uint8_t> text(size_t n)
{
    static const char *words[] = {"the ", "decoder ", "wave ", "arena ", "filter ", "branch ", "offset ", "\n", "call ", "0x"};
    std::string s;
    while (s.size() < n) s += words[rnd() % 10];
    return std::vector<uint8_t>(s.begin(), s.begin() + n);
}

int main(int argc, char **argv)
{
    if (argc == 6 && !strcmp(argv[1], "--apply")) {
        const uint32_t id = (uint32_t)strtoul(argv[2], nullptr, 0), param = (uint32_t)strtoul(argv[3], nullptr, 0);
        if (bad_step(id, param)) return 2;
        std::vector<uint8_t> v;
        if (!read_file(argv[4], v)) return 2;
        const bool agree = dev_apply_all_orders(id, param, v);
        FILE *f = fopen(argv[5], "wb");
        if (!f || (!v.empty() && fwrite(v.data(), 1, v.size(), f) != v.size())) return 2;
        fclose(f);
        return agree ? 0 : 3;
    }
    if (argc == 5 && !strcmp(argv[1], "--apply-list")) {
        std::vector<uint8_t> in;
        FILE *list = fopen(argv[2], "r");
        if (!list || !read_file(argv[3], in)) return 2;
        FILE *f = fopen(argv[4], "wb");
        if (!f) return 2;
        unsigned long id, param;
        unsigned long long n;
        size_t at = 0;
        bool agree = true;
        while (fscanf(list, "%lu %lu %llu", &id, &param, &n) == 3) {
            if (bad_step((uint32_t)id, (uint32_t)param) || n > in.size() - at) return 2;
            std::vector<uint8_t> v(in.begin() + at, in.begin() + at + n);
            at += n;
            agree &= dev_apply_all_orders((uint32_t)id, (uint32_t)param, v);
            if (!v.empty() && fwrite(v.data(), 1, v.size(), f) != v.size()) return 2;
        }
        fclose(list);
        fclose(f);
        return at != in.size() ? 2 : agree ? 0 : 3;
    }
    bool ok = true;
    if (argc > 1) {
        for (int a = 1; a < argc; a++) {
            FILE *f = fopen(argv[a], "rb");
            if (!f) {
                printf("cannot read %s\n", argv[a]);
                return 2;
            }
            std::vector<uint8_t> v;
            uint8_t tmp[65536];
            size_t got;
            while ((got = fread(tmp, 1, sizeof tmp, f)) > 0 && v.size() < (4u << 20)) v.insert(v.end(), tmp, tmp + got);
            fclose(f);
            ok &= all_filters(v, argv[a]);
        }
    } else {
        // lengths 0 - 40 and around every size the schemes are cut at, +- 5
        std::vector<size_t> lens;
        for (size_t n = 0; n <= 40; n++) lens.push_back(n);
        const size_t marks[] = {kX86Window, 2 * kX86Window, kX86Window * kX86TileWindows, kBcjTileBytes, kDeltaChunk, 2 * kDeltaChunk, 3 * kDeltaChunk, 4096, 512};
        for (size_t m : marks)
            for (int d = -5; d <= 5; d++) lens.push_back(m + d);
        const std::vector<uint8_t> soup = opcode_soup(4 * kDeltaChunk, 30), zeros(4 * kDeltaChunk, 0), txt = text(4 * kDeltaChunk);
        std::vector<uint8_t> rnd_bytes(4 * kDeltaChunk);
        for (auto &b : rnd_bytes) b = (uint8_t)rnd();
        for (size_t n : lens) {
            ok &= all_filters(std::vector<uint8_t>(soup.begin(), soup.begin() + n), "soup");
            ok &= all_filters(std::vector<uint8_t>(soup.end() - n, soup.end()), "soup tail");
            ok &= all_filters(std::vector<uint8_t>(rnd_bytes.begin(), rnd_bytes.begin() + n), "random");
        }
        ok &= all_filters(zeros, "zeros");
        ok &= all_filters(txt, "text");
        ok &= all_filters(opcode_soup(300000, 10), "soup 300000");
        {   // Delta over more chunks than one group of the second pass holds, and over exactly two and three groups
            const std::vector<uint8_t> big = opcode_soup((size_t)(3 * kDeltaGroup + 2) * kDeltaChunk + 77, 3);
            for (size_t n : {(size_t)kDeltaGroup * kDeltaChunk, (size_t)kDeltaGroup * kDeltaChunk + 1, (size_t)2 * kDeltaGroup * kDeltaChunk + 5, big.size()})
                for (uint32_t p = 0; p < 8; p++) ok &= check(kDelta, kDists[p], std::vector<uint8_t>(big.begin(), big.begin() + n), "delta groups");
        }
        ok &= all_filters(opcode_soup(100001, 90), "soup dense");
        // x86: every density, runs of E8 / E9 (windows without a sync point), opcodes in the last eight bytes
        const uint32_t dens[] = {1, 5, 10, 15, 20, 25, 30, 60, 100};
        for (uint32_t dp : dens)
            for (int runs = 0; runs < 2; runs++)
                for (size_t n : {(size_t)600, (size_t)5000, (size_t)70001}) {
                    std::vector<uint8_t> v = x86_adversarial(n, dp, runs != 0);
                    for (uint32_t p = 0; p < 3; p++) ok &= check(kX86, kOffsets[p], v, "x86 adversarial");
                    for (size_t k = 1; k <= 8; k++) {
                        std::vector<uint8_t> w = v;
                        w[n - k] = 0xE8;
                        if (k > 4) w[n - k + 4] = 0x00;
                        ok &= check(kX86, 0, w, "x86 opcode near the end");
                    }
                }
        // Thumb: chains of halfwords that alternate first / second halves across every lane boundary
        for (int phase = 0; phase < 4; phase++) {
            std::vector<uint8_t> v(1000 + phase);
            for (size_t i = 0; i + 1 < v.size(); i += 2) {
                const uint32_t r = rnd();
                const uint32_t kind = ((i / 2 + phase) & 1) ? 0xF8 : 0xF0;
                v[i] = (uint8_t)r, v[i + 1] = (uint8_t)((r % 5 == 0 ? (r >> 8) & 0xF8 : kind) | ((r >> 16) & 7));
            }
            for (uint32_t p = 0; p < 3; p++) ok &= check(kARMThumb, kOffsets[p] & ~1u, v, "thumb chain");
        }
    }
    printf("%ld cases, %ld changed by their filter\n", n_cases, n_changed);
    if (!ok || (argc == 1 && n_changed < n_cases / 4)) {
        printf("FAILED\n");
        return 1;
    }
    printf("ok\n");
    return 0;
}
