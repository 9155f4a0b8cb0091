// inflate_dev_selftest.cpp -- the raw-deflate decoder of lzma_amd/csrc/xlz_inflate_dev.h without a GPU.  A plain C++
// program: it runs the WAVE SCHEME lane by lane (every piece the lanes run is a loop over the 64 of them here) and the
// serial twin host_inflate, and compares the two; what is right is decided by the caller (tests/test_inflate_edges_cpu.py
// judges with Python's zlib).
//   g++ -O2 -std=c++17 -I lzma_amd/csrc tests/c/inflate_dev_selftest.cpp -o t && ./t
//   ./t --inflate-list LIST IN OUT    LIST: one line "in_len out_cap residue" per item, IN: the inputs back to back;
//                                     OUT: per item one byte 0 OK / 1 RESULT / 2 EOF / 3 OUT_CAP, and for OK four bytes
//                                     of consumed input (little-endian) and the bytes produced
// Every input lies in a heap block of exactly its length rounded up to 16 and every destination in one of exactly
// residue + out_cap bytes, so that AddressSanitizer sees a byte too many in either; the bytes between an input's end and
// its block's are 0xFF in one run and 0x00 in a second one, which must agree; the bytes in front of the destination are
// compared.  One Wave serves all items and is never cleared, as a workgroup's LDS is not.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "xlz_inflate_dev.h"

using namespace xlzinf;

static int g_fail = 0;
static long g_cases = 0;
#define CHECK(c, ...)                                                                                                  \
    do {                                                                                                               \
        if (!(c)) {                                                                                                    \
            if (g_fail++ < 20) printf("FAIL %s:%d: ", __FILE__, __LINE__), printf(__VA_ARGS__), printf("\n");          \
        }                                                                                                              \
    } while (0)

static Wave g_wave;

struct Outcome {
    int status;
    uint32_t produced, consumed;
    std::vector<uint8_t> bytes;
};

static Outcome run_wave(const uint8_t *in, uint32_t in_len, uint32_t out_cap, uint32_t residue, uint8_t pad, const char *what)
{
    const size_t in_block = (size_t)padded(in_len);
    uint8_t *src = static_cast<uint8_t *>(aligned_alloc(16, in_block ? in_block : 16));
    memset(src, pad, in_block ? in_block : 16);
    if (in_len) memcpy(src, in, in_len);
    // (malloc's blocks are multiples of 16: the destination lies at `residue` modulo 16)
    uint8_t *exact = static_cast<uint8_t *>(malloc((size_t)residue + out_cap ? (size_t)residue + out_cap : 1));
    memset(exact, 0xA5, (size_t)residue + out_cap);
    DevItem it;
    it.in = src, it.in_len = in_len, it.out_cap = out_cap, it.dst = residue;
    const DevResult r = wave_inflate(g_wave, it, exact);
    Outcome o;
    o.status = r.status, o.produced = r.produced, o.consumed = r.consumed;
    for (uint32_t i = 0; i < residue; i++) CHECK(exact[i] == 0xA5, "%s: byte %u in front of the destination was written", what, i);
    if (r.status == kStOk) {
        CHECK(r.produced <= out_cap, "%s: produced %u of %u", what, r.produced, out_cap);
        o.bytes.assign(exact + residue, exact + residue + r.produced);
        for (uint32_t i = r.produced; i < out_cap; i++)
            if (exact[residue + i] != 0xA5) {
                CHECK(false, "%s: byte %u behind the output was written", what, i);
                break;
            }
    } else {
        CHECK(r.produced == 0 && r.consumed == 0, "%s: a failed item reports bytes", what);
    }
    free(exact), free(src);
    return o;
}

static Outcome run_host(const uint8_t *in, uint32_t in_len, uint32_t out_cap)
{
    uint8_t *src = static_cast<uint8_t *>(malloc(in_len ? in_len : 1)), *dst = static_cast<uint8_t *>(malloc(out_cap ? out_cap : 1));
    if (in_len) memcpy(src, in, in_len);
    size_t produced = 7, consumed = 7;
    Outcome o;
    o.status = host_inflate(src, in_len, dst, out_cap, &produced, &consumed);
    o.produced = (uint32_t)produced, o.consumed = (uint32_t)consumed;
    if (o.status == kStOk) o.bytes.assign(dst, dst + produced);
    free(src), free(dst);
    return o;
}

static bool same(const Outcome &a, const Outcome &b)
{
    return a.status == b.status && a.produced == b.produced && a.consumed == b.consumed && a.bytes == b.bytes;
}

static Outcome run_all(const uint8_t *in, uint32_t in_len, uint32_t out_cap, uint32_t residue, const char *what)
{
    const Outcome a = run_wave(in, in_len, out_cap, residue, 0xFF, what), b = run_wave(in, in_len, out_cap, residue, 0x00, what);
    const Outcome h = run_host(in, in_len, out_cap);
    CHECK(same(a, b), "%s: the bytes behind the input's end changed the result (%d / %d)", what, a.status, b.status);
    CHECK(same(a, h), "%s: wave %d (%u, %u) and host %d (%u, %u) differ", what, a.status, a.produced, a.consumed, h.status, h.produced,
          h.consumed);
    g_cases++;
    return a;
}

static int inflate_list(const char *list_path, const char *in_path, const char *out_path)
{
    FILE *list = fopen(list_path, "r"), *in = fopen(in_path, "rb"), *out = fopen(out_path, "wb");
    if (!list || !in || !out) return 2;
    memset(&g_wave, 0xEE, sizeof g_wave);
    unsigned long in_len, out_cap, residue;
    std::vector<uint8_t> s;
    while (fscanf(list, "%lu %lu %lu", &in_len, &out_cap, &residue) == 3) {
        s.resize(in_len);
        if (in_len && fread(s.data(), 1, in_len, in) != in_len) return 2;
        char what[64];
        snprintf(what, sizeof what, "item %ld", g_cases);
        const Outcome o = run_all(s.data(), (uint32_t)in_len, (uint32_t)out_cap, (uint32_t)residue, what);
        const uint8_t cls = o.status == kStOk ? 0 : o.status == kStResult ? 1 : o.status == kStEof ? 2 : o.status == kStOutCap ? 3 : 9;
        fputc(cls, out);
        if (cls == 0) {
            const uint8_t c4[4] = {(uint8_t)o.consumed, (uint8_t)(o.consumed >> 8), (uint8_t)(o.consumed >> 16), (uint8_t)(o.consumed >> 24)};
            fwrite(c4, 1, 4, out);
            if (!o.bytes.empty()) fwrite(o.bytes.data(), 1, o.bytes.size(), out);
        }
    }
    fclose(list), fclose(in), fclose(out);
    printf("%ld items, %d failures\n", g_cases, g_fail);
    return g_fail ? 1 : 0;
}

// a few streams written out by hand, so that the program says something without its caller
static void builtin()
{
    memset(&g_wave, 0xEE, sizeof g_wave);
    { // a final stored block of five bytes
        const uint8_t s[] = {0x01, 0x05, 0x00, 0xFA, 0xFF, 'h', 'e', 'l', 'l', 'o'};
        for (uint32_t res = 0; res < 16; res++) {
            const Outcome o = run_all(s, sizeof s, 5, res, "stored");
            CHECK(o.status == kStOk && o.bytes.size() == 5 && !memcmp(o.bytes.data(), "hello", 5) && o.consumed == sizeof s, "stored");
        }
        CHECK(run_all(s, sizeof s, 4, 0, "stored, short of room").status == kStOutCap, "stored, short of room");
        CHECK(run_all(s, sizeof s - 1, 5, 0, "stored, cut").status == kStEof, "stored, cut");
    }
    { // fixed codes: 'a', then a match of length 9 at distance 1, end of block
        // bits: 1 (final) 01 (fixed) | 'a' = 0x30 + 0x61 = 10010001 (8) | length 9 = symbol 263: 0000111 (7) | distance 1 = 00000 | 256: 0000000
        const uint8_t s[] = {0x4B, 0x84, 0x03, 0x00, 0x00};
        const Outcome o = run_all(s, sizeof s, 10, 3, "fixed");
        CHECK(o.status == kStOk && o.bytes.size() == 10 && o.bytes == std::vector<uint8_t>(10, 'a'), "fixed: status %d, %zu bytes", o.status,
              o.bytes.size());
        CHECK(run_all(s, sizeof s, 9, 0, "fixed, short of room").status == kStOutCap, "fixed, short of room");
    }
    { // block type 3
        const uint8_t s[] = {0x07};
        CHECK(run_all(s, 1, 10, 0, "type 3").status == kStResult, "type 3");
        CHECK(run_all(s, 0, 10, 0, "empty").status == kStEof, "empty");
    }
}

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "--inflate-list")) return inflate_list(argv[2], argv[3], argv[4]);
    builtin();
    printf("%ld comparisons, %d failures\n", g_cases, g_fail);
    return g_fail ? 1 : 0;
}
