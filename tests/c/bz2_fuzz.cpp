// bz2_fuzz.cpp -- a stand-alone program over lzma_amd/csrc/xlz_bz2.h and the serial twin of xlz_bz2_dev.h: seeded
// mutations, cuts and splices of the files it is given, each decoded into a window with guard bytes behind it.  Built with
// -fsanitize=address,undefined by tests/test_bz2_cpu.py; what it checks itself: the guards, the result's invariants, that a
// second run gives the same result, and that the scan finds every chain block.
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -I include tests/c/bz2_fuzz.cpp -o f
//   ./f ROUNDS FILE...
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../lzma_amd/csrc/xlz_bz2.h"

using namespace xlzbz2;

static uint32_t rng_state = 2463534242u;
static uint32_t rng()
{
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 17, rng_state ^= rng_state << 5;
    return rng_state;
}

static int check(const std::vector<uint8_t> &f, size_t cap)
{
    std::vector<uint8_t> out(cap + 32, 0xA5), again(cap + 32, 0xA5);
    xlz_bz2_result r = {}, r2 = {};
    decode_host(f.data(), f.size(), out.data(), cap, true, &r);
    decode_host(f.data(), f.size(), again.data(), cap, true, &r2);
    for (size_t i = cap; i < out.size(); i++)
        if (out[i] != 0xA5) return 1;
    if (memcmp(&r, &r2, sizeof r)) return 2;
    if (r.status == XLZ_OK && (r.out_len > cap || r.in_consumed > f.size() || memcmp(out.data(), again.data(), r.out_len))) return 3;
    if (r.status != XLZ_OK && r.status != XLZ_ERR_OUT_CAP && (r.out_len || r.in_consumed)) return 4;
    if (r.status == XLZ_ERR_OUT_CAP && r.out_len <= cap) return 5;
    // every block of the chain is a candidate of the scan
    Chain c;
    chain_open(c, f.data(), f.size(), true);
    std::vector<Magic> m = scan(f.data(), f.size());
    HostBlockBuffers buf;
    while (chain_step(c)) {
        bool found = false;
        for (const Magic &x : m) found = found || (!x.end && x.bit == c.bit);
        if (!found) return 6;
        buf.room(c.level * kLevelBytes);
        BlockInfo bi;
        host_block(f.data(), f.size(), c.bit, c.level * kLevelBytes, buf.ll.data(), buf.tt.data(), buf.pre.data(), &bi);
        chain_block(c, bi.status, bi.end_bit, bi.nblock, bi.out_len, bi.crc);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const long rounds = atol(argv[1]);
    std::vector<std::vector<uint8_t>> files;
    for (int i = 2; i < argc; i++) {
        FILE *fp = fopen(argv[i], "rb");
        if (!fp) return 2;
        std::vector<uint8_t> f;
        uint8_t tmp[4096];
        for (size_t n; (n = fread(tmp, 1, sizeof tmp, fp)) > 0;) f.insert(f.end(), tmp, tmp + n);
        fclose(fp);
        files.push_back(f);
    }
    for (long k = 0; k < rounds; k++) {
        std::vector<uint8_t> f = files[rng() % files.size()];
        switch (f.empty() ? 3 : rng() % 5) {
        case 0: f[rng() % f.size()] ^= (uint8_t)(1u << (rng() % 8)); break;
        case 1: f[rng() % f.size()] = (uint8_t)rng(); break;
        case 2: f.resize(rng() % (f.size() + 1)); break;
        case 3: { // a splice: another file's tail behind this one's head
            const std::vector<uint8_t> &g = files[rng() % files.size()];
            f.resize(f.empty() ? 0 : rng() % f.size());
            if (!g.empty()) f.insert(f.end(), g.begin() + rng() % g.size(), g.end());
            break;
        }
        default: // a few bytes of noise
            for (int j = 0; j < 4; j++) f[rng() % f.size()] = (uint8_t)rng();
        }
        const size_t cap = rng() % 3 ? 70000 : rng() % 2000;
        const int rc = check(f, cap);
        if (rc) {
            printf("round %ld: check %d\n", k, rc);
            return 1;
        }
    }
    puts("ok");
    return 0;
}
