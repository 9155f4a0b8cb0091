// bcj2_dev_selftest.cpp -- the BCJ2 merge of lzma_amd/csrc/xlz_bcj2_dev.h without a GPU.  A plain C++ program: it encodes
// inputs with an encoder of its own (written from the description, as tests/bcj2_ref.py is), checks that host_merge()
// gives the input back, and runs the WAVE SCHEME phase by phase with the lanes in descending order -- so nothing may depend
// on lane 0 going first -- into a guarded destination at every alignment, against host_merge: same status, same bytes,
// guards untouched.  Every stream lies in a heap block of exactly its length rounded up to 16, so an address sanitizer sees
// any load the header's alignment rule does not cover.
//   g++ -O2 -std=c++17 -I lzma_amd/csrc tests/c/bcj2_dev_selftest.cpp -o t && ./t [file of machine code]
//   ./t --merge-list LIST IN OUT   the wave scheme on items somebody else made (tests/bcj2_edges.py): LIST holds a line
//                                  "MAIN CALL JUMP RC OUT_LEN RESIDUE KEEP" per item -- the lengths of its four streams,
//                                  which lie end to end in IN, its out_len, the residue modulo 16 of its destination, and
//                                  KEEP = 1 for an item that finds the Wave as the item before it left it (what a
//                                  workgroup's second item finds; 0: filled with A5).  OUT receives per item a status byte
//                                  (0 OK, 1 XLZ_ERR_RESULT) and, for status 0, the out_len bytes.  Exit status 3: the
//                                  wave and host_merge disagree, or a guard byte was written.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "xlz_bcj2_dev.h"

using namespace xlzbcj2;
using Bytes = std::vector<uint8_t>;

static int g_fail = 0;
static long g_cases = 0;
#define CHECK(c, ...)                                                                                                  \
    do {                                                                                                               \
        if (!(c)) {                                                                                                    \
            if (g_fail++ < 20) printf("FAIL %s:%d: ", __FILE__, __LINE__), printf(__VA_ARGS__), printf("\n");          \
        }                                                                                                              \
    } while (0)

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_seed ^= g_seed << 13, g_seed ^= g_seed >> 7, g_seed ^= g_seed << 17;
    return (uint32_t)(g_seed >> 16);
}

// ---- the encoder ----
struct RangeEnc {
    uint64_t low = 0;
    uint32_t range = 0xFFFFFFFFu;
    uint8_t cache = 0;
    uint64_t cache_size = 1;
    Bytes out;
    void shift_low()
    {
        if (low < 0xFF000000ull || low >= (1ull << 32)) {
            const uint8_t carry = (uint8_t)(low >> 32);
            uint8_t c = cache;
            do {
                out.push_back((uint8_t)(c + carry));
                c = 0xFF;
            } while (--cache_size);
            cache = (uint8_t)(low >> 24);
        }
        cache_size++;
        low = (low & 0x00FFFFFFull) << 8;
    }
    void bit(uint16_t &p, bool b)
    {
        const uint32_t bound = (range >> 11) * p;
        if (!b)
            range = bound, p = (uint16_t)(p + ((2048 - p) >> 5));
        else
            low += bound, range -= bound, p = (uint16_t)(p - (p >> 5));
        while (range < kTop) range <<= 8, shift_low();
    }
    void finish()
    {
        for (int i = 0; i < 5; i++) shift_low();
    }
};

struct Enc {
    Bytes main, call, jump, rc;
};
// policy: 0 near branches (top byte 00 / FF), 1 those and top byte 0F (the prev trap), 2 every candidate, 3 none
static Enc encode(const Bytes &d, int policy)
{
    Enc e;
    RangeEnc rc;
    uint16_t probs[kProbs];
    for (auto &p : probs) p = 1024;
    uint32_t prev = 0;
    size_t i = 0;
    const size_t n = d.size();
    while (i < n) {
        const uint32_t b = d[i++];
        e.main.push_back((uint8_t)b);
        if (!is_j(prev, b)) {
            prev = b;
            continue;
        }
        if (i == n) break;
        uint16_t &p = probs[prob_index(prev, b)];
        if (n - i >= 4) {
            const uint32_t rel = (uint32_t)d[i] | (uint32_t)d[i + 1] << 8 | (uint32_t)d[i + 2] << 16 | (uint32_t)d[i + 3] << 24;
            const uint32_t top = rel >> 24;
            const bool take = policy == 2 || (policy != 3 && (top == 0 || top == 0xFF || (policy == 1 && top == 0x0F)));
            if (take) {
                rc.bit(p, true);
                const uint32_t abs = rel + (uint32_t)(i + 4);
                Bytes &s = b == 0xE8 ? e.call : e.jump;
                s.push_back((uint8_t)(abs >> 24)), s.push_back((uint8_t)(abs >> 16)), s.push_back((uint8_t)(abs >> 8)), s.push_back((uint8_t)abs);
                i += 4;
                prev = top;
                continue;
            }
        }
        rc.bit(p, false);
        prev = b;
    }
    rc.finish();
    e.rc = rc.out;
    return e;
}

// ---- the wave, lane by lane ----
// a copy of v in a block of exactly its length rounded up to 16 (malloc aligns to 16)
struct Block {
    uint8_t *p;
    explicit Block(const Bytes &v) : p((uint8_t *)malloc(((v.size() + 15) & ~(size_t)15) + (v.empty() ? 16 : 0)))
    {
        if (!v.empty()) memcpy(p, v.data(), v.size());
    }
    ~Block() { free(p); }
};

static DevResult wave_run(const DevItem &it, uint8_t *dst, bool keep = false)
{
    static Wave w;
    if (!keep) memset(&w, 0xA5, sizeof w);
    for (int l = kLanes - 1; l >= 0; l--) wave_init(w, it, (uint32_t)l);
    while (!w.done) {
        for (int l = kLanes - 1; l >= 0; l--) wave_load(w, it, (uint32_t)l);
        for (int l = kLanes - 1; l >= 0; l--) wave_mark(w, it, (uint32_t)l);
        wave_decide(w, it);
        for (int l = kLanes - 1; l >= 0; l--) wave_place(w, (uint32_t)l);
        for (int l = kLanes - 1; l >= 0; l--) wave_store(w, it, dst, (uint32_t)l);
    }
    return wave_result(w, it);
}

// host_merge and the wave on the same four streams and out_len, the wave at destination offset dst_off (any alignment)
static void compare(const char *what, const Enc &e, size_t out_len, const Bytes *expect, int expect_status, uint32_t dst_off, bool keep = false,
                    FILE *report = nullptr)
{
    g_cases++;
    Bytes ho(out_len + 1, 0xCC);
    size_t hp = 0;
    const int hs = host_merge(e.main.data(), e.main.size(), e.call.data(), e.call.size(), e.jump.data(), e.jump.size(), e.rc.data(), e.rc.size(),
                              ho.data(), out_len, &hp);
    CHECK(ho[out_len] == 0xCC, "%s: host_merge wrote behind out_len", what);
    if (expect_status != 1) CHECK(hs == expect_status, "%s: host_merge status %d, expected %d", what, hs, expect_status);
    if (expect && hs == kStOk) CHECK(hp == out_len && (!out_len || !memcmp(ho.data(), expect->data(), out_len)), "%s: host_merge bytes differ (len %zu)", what, out_len);
    constexpr size_t kGuard = 64;
    const Block bm(e.main), bc(e.call), bj(e.jump), br(e.rc);
    uint8_t *raw = (uint8_t *)malloc(kGuard + 16 + dst_off + out_len + kGuard);
    uint8_t *base = raw + ((0 - (uintptr_t)raw) & 15); // a multiple of 16: the item's place is base + kGuard + dst_off
    const size_t span = kGuard + dst_off + out_len + kGuard;
    memset(base, 0x5A, span);
    DevItem it;
    memset(&it, 0, sizeof it);
    it.main = bm.p, it.call = bc.p, it.jump = bj.p, it.rc = br.p;
    it.main_len = (uint32_t)e.main.size(), it.call_len = (uint32_t)e.call.size(), it.jump_len = (uint32_t)e.jump.size(), it.rc_len = (uint32_t)e.rc.size();
    it.dst = kGuard + dst_off, it.out_len = (uint32_t)out_len;
    const DevResult r = wave_run(it, base, keep);
    CHECK(r.status == hs, "%s: wave status %d, host_merge %d (out_len %zu, dst_off %u)", what, r.status, hs, out_len, dst_off);
    if (hs == kStOk && r.status == kStOk) // (how far a failed merge came is not part of the contract)
        CHECK(r.produced == hp && !memcmp(base + it.dst, ho.data(), out_len), "%s: wave bytes differ (out_len %zu, dst_off %u)", what, out_len, dst_off);
    bool guards = true;
    for (size_t i = 0; i < it.dst; i++) guards = guards && base[i] == 0x5A;
    for (size_t i = it.dst + out_len; i < span; i++) guards = guards && base[i] == 0x5A;
    CHECK(guards, "%s: wave wrote outside its range (out_len %zu, dst_off %u)", what, out_len, dst_off);
    if (report) {
        fputc(r.status == kStOk ? 0 : 1, report);
        if (r.status == kStOk && out_len) fwrite(base + it.dst, 1, out_len, report);
    }
    free(raw);
}

// everything one input goes through
static void run_input(const char *what, const Bytes &d, int policy, bool thorough)
{
    const Enc e = encode(d, policy);
    static const uint32_t offs[4] = {0, 1, 7, 13};
    for (uint32_t k = 0; k < (thorough ? 4u : 1u); k++) compare(what, e, d.size(), &d, kStOk, offs[(k + d.size()) & 3]);
    if (!thorough) return;
    // less room than the streams fill: a cut operand, a candidate as the last byte, ...: OK with a prefix of the input
    for (size_t cut = 1; cut <= 9 && cut <= d.size(); cut++) compare(what, e, d.size() - cut, &d, kStOk, (uint32_t)cut);
    // more room than they fill, and damaged streams: XLZ_ERR_RESULT
    compare(what, e, d.size() + 1, nullptr, kStResult, 3);
    Enc t = e;
    if (!t.main.empty()) {
        t.main.pop_back();
        compare(what, t, d.size(), nullptr, kStResult, 5);
    }
    if (e.call.size() >= 4) {
        t = e, t.call.resize(e.call.size() - 1);
        compare(what, t, d.size(), nullptr, kStResult, 2);
        t = e, t.call.resize(e.call.size() / 8 * 4);
        compare(what, t, d.size(), nullptr, kStResult, 2);
    }
    if (e.jump.size() >= 4) {
        t = e, t.jump.resize(e.jump.size() - 4);
        compare(what, t, d.size(), nullptr, kStResult, 9);
    }
    if (!d.empty()) {
        t = e, t.rc.resize(4);
        compare(what, t, d.size(), nullptr, kStResult, 0);
    }
    if (e.rc.size() > 6) { // (status 1: whatever it is -- the cut may fall behind the last byte the decoder reads)
        t = e, t.rc.resize(e.rc.size() / 2 > 5 ? e.rc.size() / 2 : 5);
        compare(what, t, d.size(), nullptr, 1, 11);
    }
}

static Bytes soup(size_t n, uint32_t density)
{
    Bytes v(n);
    for (auto &b : v) b = (uint8_t)rnd();
    for (size_t i = 0; i + 6 < n; i++) {
        if (rnd() % 100 >= density) continue;
        const uint32_t r = rnd() % 4;
        if (r == 3)
            v[i] = 0x0F, v[i + 1] = (uint8_t)(0x80 | (rnd() & 15)), i++;
        else
            v[i] = r == 0 ? 0xE9 : 0xE8;
        const uint32_t t = rnd() % 4;
        v[i + 4] = t == 0 ? 0x00 : t == 1 ? 0xFF : t == 2 ? 0x0F : (uint8_t)rnd();
    }
    return v;
}
static Bytes plain(size_t n)
{
    Bytes v(n);
    for (size_t i = 0; i < n; i++) v[i] = (uint8_t)((7 * i + 1) % 0xE0); // no E8 / E9, no 0F 8x
    return v;
}

// --merge-list: see the head of this file
static int merge_list(const char *list_path, const char *in_path, const char *out_path)
{
    FILE *list = fopen(list_path, "r"), *in = fopen(in_path, "rb"), *out = fopen(out_path, "wb");
    if (!list || !in || !out) return 2;
    unsigned long len[4], out_len, res, keep;
    char what[32];
    while (fscanf(list, "%lu %lu %lu %lu %lu %lu %lu", &len[0], &len[1], &len[2], &len[3], &out_len, &res, &keep) == 7) {
        if (res > 15 || keep > 1) return 2;
        Enc e;
        Bytes *s[4] = {&e.main, &e.call, &e.jump, &e.rc};
        for (int k = 0; k < 4; k++) {
            s[k]->resize(len[k]);
            if (len[k] && fread(s[k]->data(), 1, len[k], in) != len[k]) return 2;
        }
        snprintf(what, sizeof what, "item %ld", g_cases);
        compare(what, e, out_len, nullptr, 1, (uint32_t)res, keep != 0, out);
    }
    const bool rest = fgetc(in) != EOF;
    fclose(list), fclose(in);
    if (fclose(out) != 0 || rest) return 2;
    printf("%ld items, %d failures\n", g_cases, g_fail);
    return g_fail ? 3 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "--merge-list")) return merge_list(argv[2], argv[3], argv[4]);
    static const size_t lens[] = {0, 1, 4, 5, 6, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049, 5000, 65539};
    for (size_t n : lens)
        for (int policy = 0; policy < 4; policy++)
            for (uint32_t density : {0u, 3u, 30u}) run_input("soup", soup(n, density), policy, true);
    for (size_t n : {(size_t)1, (size_t)5, (size_t)1024, (size_t)4096, (size_t)5121})
        for (int policy : {2, 3, 0}) {
            run_input("E8 run", Bytes(n, 0xE8), policy, true);
            Bytes v(n);
            for (size_t i = 0; i < n; i++) v[i] = i & 1 ? (uint8_t)(0x80 | ((i >> 1) & 15)) : 0x0F;
            run_input("0F 8x run", v, policy, true);
        }
    // a candidate as the last byte, and with one to three bytes behind it
    for (size_t lead : {(size_t)0, (size_t)3, (size_t)1019, (size_t)1023, (size_t)1024})
        for (size_t behind = 0; behind <= 5; behind++)
            for (uint8_t op : {(uint8_t)0xE8, (uint8_t)0xE9}) {
                Bytes v = plain(lead);
                v.push_back(op);
                for (size_t k = 0; k < behind; k++) v.push_back(0);
                run_input("candidate near the end", v, 0, true);
            }
    // window boundaries of the MAIN stream (no candidate in the lead: main position = input position): the opcode as a
    // window's last byte with its operand in the next; the prev trap -- E8, operand with top byte 0F, then 80 -- with the
    // 80 as the next window's first byte, and inside a window, and across a lane's sixteen bytes
    bool trap_seen = false;
    for (size_t lead : {(size_t)0, (size_t)14, (size_t)15, (size_t)100, (size_t)1022, (size_t)1023, (size_t)1024, (size_t)2047, (size_t)3071}) {
        Bytes v = plain(lead);
        const uint8_t body[] = {0xE8, 0x11, 0x22, 0x33, 0x0F, 0x80, 0x44, 0x55, 0x66, 0x00};
        v.insert(v.end(), body, body + sizeof body);
        const Bytes tail = plain(40);
        v.insert(v.end(), tail.begin(), tail.end());
        const Enc e = encode(v, 1);
        // the trap is there: the main stream has E8 80 side by side, and both were converted
        if (e.main.size() == v.size() - 8 && e.main[lead] == 0xE8 && e.main[lead + 1] == 0x80 && e.call.size() == 4 && e.jump.size() == 4) trap_seen = true;
        else CHECK(false, "the prev trap is not in the input (lead %zu)", lead);
        run_input("prev trap", v, 1, true);
    }
    CHECK(trap_seen, "no trap input");
    // a window without candidates between two with, a window of 1024 candidates taken / not taken, a conversion that ends
    // exactly at out_len
    {
        Bytes v = soup(1024, 30), p = plain(1024), s = soup(700, 30);
        v.insert(v.end(), p.begin(), p.end()), v.insert(v.end(), s.begin(), s.end());
        for (int policy = 0; policy < 4; policy++) run_input("quiet window", v, policy, true);
        Bytes c = plain(2000);
        const uint8_t last[] = {0xE8, 0x10, 0x00, 0x00, 0x00};
        c.insert(c.end(), last, last + 5);
        run_input("conversion at the end", c, 0, true);
    }
    for (int k = 0; k < 300; k++) run_input("random", soup(1 + rnd() % 9000, rnd() % 60), (int)(rnd() % 4), false);
    // real machine code: the file named on the command line, else this program
    {
        const char *path = argc > 1 ? argv[1] : argv[0];
        FILE *f = fopen(path, "rb");
        Bytes v;
        if (f) {
            v.resize(400000);
            v.resize(fread(v.data(), 1, v.size(), f));
            fclose(f);
        }
        CHECK(!v.empty(), "cannot read %s", path);
        const Enc e = encode(v, 0);
        CHECK(e.call.size() + e.jump.size() > 0 || v.size() < 4096, "no conversion in the machine code");
        run_input("machine code", v, 0, true);
    }
    printf("%ld comparisons, %d failures\n", g_cases, g_fail);
    puts(g_fail ? "FAILED" : "ok");
    return g_fail ? 1 : 0;
}
