// One lane of the device's SHA-256 (lzma_amd/csrc/xlz_sha256_dev.h) run on the CPU against the FIPS 180-4 known answers
// and the host's xlzcheck::sha256: what xlz_check_sha256_kernel computes per range, without a GPU.  Prints "ok" and exits
// 0, or says what differs.
//   sha256_dev_selftest                        the built-in sweep
//   sha256_dev_selftest --list LIST ARENA OUT  the lane's code over the ranges LIST names in the bytes of ARENA (list_mode
//                                              below): tests/test_digest_edges_cpu.py judges the digests in OUT
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "xlz_check.h"
#include "xlz_sha256_dev.h"

using namespace xlzsha;

static int failures = 0;

// what the kernel stores for one range: the digest's bytes in FIPS order
static void lane(const uint8_t *arena, uint64_t arena_bytes, uint64_t off, uint64_t len, uint8_t out[32])
{
    uint32_t h[8];
    lane_digest(arena, arena_bytes, off, len, h);
    for (int k = 0; k < 8; k++) {
        const uint32_t v = digest_word(h[k]);
        memcpy(out + 4 * k, &v, 4);
    }
}

static void hex(const uint8_t d[32], char s[65])
{
    for (int i = 0; i < 32; i++) snprintf(s + 2 * i, 3, "%02x", d[i]);
}

static void known(const char *name, const std::vector<uint8_t> &msg, const char *want)
{
    // at every start alignment, in an arena that ends with the message and in one with room behind it
    for (uint64_t off = 0; off < 16; off++)
        for (uint64_t slack : {0ull, 200ull}) {
            std::vector<uint8_t> arena(off + msg.size() + slack, 0xA5);
            if (!msg.empty()) memcpy(arena.data() + off, msg.data(), msg.size());
            uint8_t d[32];
            char s[65];
            lane(arena.data(), arena.size(), off, msg.size(), d);
            hex(d, s);
            if (strcmp(s, want) != 0) {
                printf("known answer %s at offset %llu (slack %llu): %s, want %s\n", name, (unsigned long long)off,
                       (unsigned long long)slack, s, want);
                failures++;
            }
        }
}

static void against_host(const std::vector<uint8_t> &arena, uint64_t arena_bytes, uint64_t off, uint64_t len, const char *what)
{
    uint8_t d[32], ref[32];
    lane(arena.data(), arena_bytes, off, len, d);
    xlzcheck::sha256(arena.data() + off, (size_t)len, ref);
    if (memcmp(d, ref, 32) != 0) {
        printf("%s: offset %llu length %llu in an arena of %llu differs from xlzcheck::sha256\n", what, (unsigned long long)off,
               (unsigned long long)len, (unsigned long long)arena_bytes);
        failures++;
    }
}

// --list: one range per line of LIST, "KIND OFF LEN" (KIND 10 = SHA-256; OFF + LEN inside ARENA), through lane_digest and
// digest_word with the file's size as arena_bytes; OUT receives the 32 bytes the kernel would store per line
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
    unsigned long kind;
    unsigned long long off, len;
    while (fscanf(list, "%lu %llu %llu", &kind, &off, &len) == 3) {
        if (kind != 10 || off > arena.size() || len > arena.size() - off) return 2;
        uint8_t d[32];
        lane(arena.data(), arena.size(), off, len, d);
        if (fwrite(d, 1, 32, out) != 32) return 2;
    }
    const bool all_read = feof(list) != 0;
    fclose(list);
    return fclose(out) == 0 && all_read ? 0 : 2;
}

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "--list")) return list_mode(argv[2], argv[3], argv[4]);
    if (argc != 1) {
        printf("usage: sha256_dev_selftest [--list LIST ARENA OUT]\n");
        return 2;
    }
    known("empty", {}, "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855");
    known("abc", {'a', 'b', 'c'}, "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad");
    {
        const char *m = "abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq";
        known("56 bytes", std::vector<uint8_t>(m, m + 56), "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1");
    }
    known("a million a", std::vector<uint8_t>(1000000, 'a'), "cdc76e5c9914fb9281a1c7e284d73e67f1809a48a497200e046d39ccc7112cd0");

    std::vector<uint8_t> arena(1 << 16);
    uint32_t x = 12345;
    for (uint8_t &b : arena) b = (uint8_t)((x = x * 1664525u + 1013904223u) >> 24);
    // every length 0-300 at every start alignment 0-15 (behind a 64-byte lead, so that bytes lie in front of the range),
    // in the big arena and in one that ends where the range ends (the byte-wise blocks at the arena's end)
    for (uint64_t a = 0; a < 16; a++)
        for (uint64_t len = 0; len <= 300; len++) {
            against_host(arena, arena.size(), 64 + a, len, "sweep");
            against_host(arena, 64 + a + len, 64 + a, len, "sweep, arena ends with the range");
            against_host(arena, 64 + a + len + 3, 64 + a, len, "sweep, three bytes behind the range");
        }
    // the padding's corners, with many blocks in front
    for (uint64_t blocks : {0ull, 1ull, 2ull, 37ull})
        for (uint64_t r : {0ull, 1ull, 54ull, 55ull, 56ull, 57ull, 62ull, 63ull, 64ull, 65ull, 118ull, 119ull, 120ull, 121ull, 127ull, 128ull})
            for (uint64_t a : {0ull, 1ull, 2ull, 3ull, 5ull, 15ull}) {
                against_host(arena, arena.size(), a, 64 * blocks + r, "padding corners");
                against_host(arena, a + 64 * blocks + r, a, 64 * blocks + r, "padding corners, arena ends with the range");
            }
    // poison on both sides of a range must not change its digest
    for (uint64_t a = 0; a < 16; a++)
        for (uint64_t len : {0ull, 1ull, 3ull, 4ull, 63ull, 64ull, 65ull, 127ull, 128ull, 129ull, 1000ull, 4096ull, 4099ull}) {
            const uint64_t off = 256 + a;
            uint8_t before[32], after[32];
            lane(arena.data(), arena.size(), off, len, before);
            std::vector<uint8_t> poisoned(arena);
            for (uint64_t i = 0; i < off; i++) poisoned[i] ^= 0xFF;
            for (uint64_t i = off + len; i < poisoned.size(); i++) poisoned[i] ^= 0xFF;
            lane(poisoned.data(), poisoned.size(), off, len, after);
            if (memcmp(before, after, 32) != 0) {
                printf("bytes outside offset %llu length %llu reached its digest\n", (unsigned long long)off, (unsigned long long)len);
                failures++;
            }
        }
    // the byte permute that does the big-endian load: every shift
    for (uint32_t s = 0; s < 4; s++) {
        const uint32_t lo = 0x03020100u, hi = 0x07060504u, want = (s << 24) | ((s + 1) << 16) | ((s + 2) << 8) | (s + 3);
        if (perm(hi, lo, be_selector(s)) != want) {
            printf("perm with shift %u: %08x, want %08x\n", s, perm(hi, lo, be_selector(s)), want);
            failures++;
        }
    }
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
