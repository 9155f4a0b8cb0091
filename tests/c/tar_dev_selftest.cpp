// tar_dev_selftest.cpp -- the lane scheme of lzma_amd/csrc/xlz_tar_dev.h on the CPU, against a serial classifier written
// here.  Plain C++ (g++ -Wall -Werror, no GPU): every pair of blocks of an image through wave_pair -- the 64 lanes of a wave
// in turn, the xor-shuffles and the ballot spelled out --, pairs in descending order for odd runs (no pair may depend on
// another), into a flag array pre-filled with a sentinel and one byte longer than the image has blocks.  The header's
// load helper asserts that no load leaves the complete blocks of the image, and every image is a heap block of exactly
// len bytes, so a sanitizer build sees a stray load too.  Gather: index lists into a sentinel-filled staging buffer.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "xlz_tar_dev.h"

using namespace xlztar;

namespace {

constexpr uint8_t kSentinel = 0xA5;
uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

int failures = 0;
int runs = 0;

// the judge: one block, byte by byte
uint8_t serial_flag(const uint8_t *b)
{
    long u = 0, s = 0;
    bool zero = true;
    for (int i = 0; i < 512; i++) {
        const int c = (i >= 148 && i < 156) ? 0x20 : b[i];
        u += c, s += c >= 0x80 ? c - 256 : c;
        if (b[i]) zero = false;
    }
    if (zero) return 2;
    int i = 148, digits = 0;
    long v = 0;
    while (i < 156 && b[i] == ' ') i++;
    while (i < 156 && b[i] >= '0' && b[i] <= '7') v = v * 8 + (b[i++] - '0'), digits++;
    if (digits < 1 || digits > 7) return 0;
    while (i < 156)
        if (b[i] != 0 && b[i] != ' ') return 0;
        else i++;
    return v == u || v == s ? 1 : 0;
}

struct Image { // exactly len bytes on the heap
    uint8_t *p;
    uint64_t len;
    explicit Image(uint64_t n) : p(static_cast<uint8_t *>(malloc(n ? (size_t)n : 1))), len(n) { memset(p, 0, n ? (size_t)n : 1); }
    ~Image() { free(p); }
    Image(const Image &) = delete;
    Image &operator=(const Image &) = delete;
};

void check(const char *what, const Image &im)
{
    const uint64_t nb = im.len >> 9, np = pair_count(im.len);
    std::vector<uint8_t> got((size_t)nb + 1, kSentinel);
    if (runs++ & 1)
        for (uint64_t p = np; p-- > 0;) wave_pair(im.p, im.len, p, got.data());
    else
        for (uint64_t p = 0; p < np; p++) wave_pair(im.p, im.len, p, got.data());
    for (uint64_t b = 0; b < nb; b++) {
        const uint8_t want = serial_flag(im.p + 512 * b);
        if (got[(size_t)b] != want) {
            printf("%s: block %llu of %llu: flag %u, the serial classifier says %u\n", what, (unsigned long long)b, (unsigned long long)nb,
                   got[(size_t)b], want);
            failures++;
            return;
        }
    }
    if (got[(size_t)nb] != kSentinel) printf("%s: a flag was written behind the last complete block\n", what), failures++;
}

// a header-like block: random printable bytes in the name, some fields, then the field written in `form` over `value`
enum Form { kSevenDigitsNul, kSixDigitsNulSpace, kLeadingSpaces, kSevenDigitsNoEnd, kAllSpaces, kAllNul, kDigitEight, kJunkBehindEnd, kEightDigits };
void put_field(uint8_t *b, Form form, long value)
{
    char f[16];
    memset(f, 0, sizeof f);
    switch (form) {
    case kSevenDigitsNul: snprintf(f, sizeof f, "%07lo", value); break;                      // "0012345\0"
    case kSixDigitsNulSpace: snprintf(f, sizeof f, "%06lo", value), f[7] = ' '; break;       // "012345\0 "
    case kLeadingSpaces: snprintf(f, sizeof f, "%6lo", value), f[6] = ' ', f[7] = 0; break;  // "  2345 \0"
    case kSevenDigitsNoEnd: snprintf(f, sizeof f, " %07lo", value); break;                   // " 0012345"
    case kAllSpaces: memset(f, ' ', 8); break;
    case kAllNul: break;
    case kDigitEight: snprintf(f, sizeof f, "%07lo", value), f[3] = '8'; break;
    case kJunkBehindEnd: snprintf(f, sizeof f, "%06lo", value), f[7] = 'x'; break;
    case kEightDigits: snprintf(f, sizeof f, "%08lo", value); break;
    }
    memcpy(b + 148, f, 8);
}
long sum_of(const uint8_t *b, bool as_signed)
{
    long s = 256;
    for (int i = 0; i < 512; i++)
        if (i < 148 || i >= 156) s += as_signed && b[i] >= 0x80 ? b[i] - 256 : b[i];
    return s;
}
void header_block(uint8_t *b, Form form, bool high_bytes, bool as_signed, long off_by = 0)
{
    memset(b, 0, 512);
    for (int i = 0; i < 60; i++) b[i] = (uint8_t)('a' + rnd() % 26);
    if (high_bytes)
        for (int i = 60; i < 90; i++) b[i] = (uint8_t)(0x80 + rnd() % 128);
    memcpy(b + 100, "0000644", 7), memcpy(b + 124, "00000001000", 11), b[156] = '0', memcpy(b + 257, "ustar", 5);
    put_field(b, form, sum_of(b, as_signed) + off_by);
}

void fill_mixed(Image &im)
{
    const uint64_t nb = im.len >> 9;
    for (uint64_t i = 0; i < im.len; i++) im.p[i] = (uint8_t)rnd();
    for (uint64_t b = 0; b < nb; b++) {
        uint8_t *p = im.p + 512 * b;
        switch (rnd() % 6) {
        case 0: memset(p, 0, 512); break;
        case 1: header_block(p, (Form)(rnd() % 9), rnd() & 1, rnd() & 1); break;
        case 2: header_block(p, kSixDigitsNulSpace, rnd() & 1, rnd() & 1, (rnd() & 1) ? 1 : -1); break;
        case 3: memset(p, 0, 512), p[rnd() % 512] = (uint8_t)(1 + rnd() % 255); break; // one non-zero byte, any lane
        default: break; // random bytes
        }
    }
}

void classify_tests()
{
    for (uint64_t nb : {0, 1, 2, 63, 64, 65, 127, 128, 129})
        for (int rep = 0; rep < 3; rep++) {
            Image im(512 * nb);
            fill_mixed(im);
            check("block counts", im);
        }
    for (uint64_t len : {511, 512, 513, 1023, 1024, 1025}) {
        Image im(len);
        fill_mixed(im);
        if (len >= 512) header_block(im.p, kSixDigitsNulSpace, false, false);
        check("lengths", im);
    }
    for (int form = kSevenDigitsNul; form <= kEightDigits; form++)
        for (int high = 0; high < 2; high++)
            for (int as_signed = 0; as_signed < 2; as_signed++) {
                Image im(512 * 3); // the block under test in each half of a pair, and alone in the last pair
                for (int k = 0; k < 3; k++) header_block(im.p + 512 * k, (Form)form, high, as_signed);
                check("field forms", im);
                const uint8_t want = form == kAllSpaces || form == kAllNul || form == kDigitEight || form == kJunkBehindEnd || form == kEightDigits ? 0 : 1;
                if (serial_flag(im.p) != want) printf("field form %d: the serial classifier says %u\n", form, serial_flag(im.p)), failures++;
            }
    { // signed and unsigned sums differ; each stored in turn is a candidate, the mean of the two is none
        Image im(512 * 3);
        header_block(im.p, kSixDigitsNulSpace, true, false);
        header_block(im.p + 512, kSixDigitsNulSpace, true, true);
        header_block(im.p + 1024, kSixDigitsNulSpace, true, true);
        put_field(im.p + 1024, kSixDigitsNulSpace, (sum_of(im.p + 1024, false) + sum_of(im.p + 1024, true)) / 2);
        check("signed and unsigned", im);
        if (sum_of(im.p, false) == sum_of(im.p, true) || serial_flag(im.p) != 1 || serial_flag(im.p + 512) != 1 || serial_flag(im.p + 1024) != 0)
            printf("signed and unsigned: bad test blocks\n"), failures++;
    }
    { // only the field is non-zero: the sum is 256 = 0400
        Image im(512 * 2);
        memcpy(im.p + 148, "0000400", 8);
        memcpy(im.p + 512 + 148, "0000401", 8);
        check("field alone", im);
        if (serial_flag(im.p) != 1 || serial_flag(im.p + 512) != 0) printf("field alone: bad test blocks\n"), failures++;
    }
    for (long off_by : {-1, 1}) {
        Image im(512 * 2);
        header_block(im.p, kSevenDigitsNul, false, false, off_by);
        header_block(im.p + 512, kSevenDigitsNul, true, true, off_by);
        check("off by one", im);
        if (serial_flag(im.p) != 0 || serial_flag(im.p + 512) != 0) printf("off by one: bad test blocks\n"), failures++;
    }
    { // every byte 0xFF: the largest sums the packed word must hold
        Image im(512 * 2);
        memset(im.p, 0xFF, 1024);
        put_field(im.p, kSixDigitsNulSpace, sum_of(im.p, false));
        put_field(im.p + 512, kSevenDigitsNul, 504 * 255 + 256 - 1);
        check("all ones", im);
        if (serial_flag(im.p) != 1) printf("all ones: bad test block\n"), failures++;
    }
}

void gather_run(const char *what, const Image &im, const std::vector<uint64_t> &idx)
{
    std::vector<uint8_t> got(idx.size() * 512 + 16, kSentinel), want(idx.size() * 512 + 16, kSentinel);
    for (size_t k = 0; k < idx.size(); k++) memcpy(want.data() + 512 * k, im.p + 512 * idx[k], 512);
    const uint64_t chunks = idx.size() * kBlockLanes;
    if (runs++ & 1)
        for (uint64_t c = chunks; c-- > 0;) gather_chunk(im.p, im.len, idx.data(), got.data(), c);
    else
        for (uint64_t c = 0; c < chunks; c++) gather_chunk(im.p, im.len, idx.data(), got.data(), c);
    if (got != want) printf("gather %s: the staging buffer differs\n", what), failures++;
}

void gather_tests()
{
    Image im(512 * 130 + 77);
    for (uint64_t i = 0; i < im.len; i++) im.p[i] = (uint8_t)rnd();
    gather_run("empty", im, {});
    gather_run("one", im, {129});
    gather_run("first", im, {0});
    std::vector<uint64_t> many;
    for (int k = 0; k < 65; k++) many.push_back(rnd() % 130);
    gather_run("65", im, many);
    gather_run("repeated and descending", im, {129, 129, 64, 64, 63, 2, 1, 1, 0, 0});
}

} // namespace

int main()
{
    classify_tests();
    gather_tests();
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("tar_dev_selftest: %d runs ok\n", runs);
    return 0;
}
