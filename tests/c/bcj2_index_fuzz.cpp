// bcj2_index_fuzz.cpp -- a seeded mutation loop over the headers of .7z archives with BCJ2 folders, through
// xlz_7z_index_bcj2 (and the two older index calls), as a stand-alone program: the parser of lzma_amd/csrc/xlz_7z.hip is
// host-only code and is compiled INTO this program, what it calls of the rest of the library is stubbed (an index call with
// ctx == NULL on a plain header never gets there).  Meant to be built with -fsanitize=address,undefined: every mutated header
// is parsed twice (count, then fill into arrays of exactly the counted sizes), the header's CRCs mended so that the
// mutation reaches the parser.
//   g++ -O1 -g -std=c++17 -x c++ -fsanitize=address,undefined -I include tests/c/bcj2_index_fuzz.cpp -o f && ./f ROUNDS a.7z b.7z ...
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../lzma_amd/csrc/xlz_7z.hip"

// ---- what xlz_7z.hip calls of xlz_host.hip ----
extern "C" uint32_t xlz_decode_dict_size2(uint8_t e) { return e >= 40 ? 0xFFFFFFFFu : (uint32_t)(2 | (e & 1)) << (e / 2 + 11); }
extern "C" int xlz_ctx_check_mode(const xlz_ctx *) { return 0; }
extern "C" int xlz_ctx_filter_mode(const xlz_ctx *) { return 0; }
extern "C" int xlz_ctx_bcj2_mode(const xlz_ctx *) { return 0; }
extern "C" int xlz_decode_batch(xlz_ctx *, const xlz_stream_desc *, size_t, xlz_result *) { return XLZ_ERR_DEVICE; }
extern "C" int xlz_decode_batch_multi(xlz_ctx *const *, size_t, const xlz_stream_desc *, size_t, xlz_result *) { return XLZ_ERR_DEVICE; }
void xlz_internal_check_stats_reset(xlz_ctx *) {}
void xlz_internal_check_stats_host(xlz_ctx *, uint64_t, uint64_t) {}
void xlz_internal_filter_stats_reset(xlz_ctx *) {}
void xlz_internal_bcj2_stats_reset(xlz_ctx *) {}
int xlz_internal_decode_batch(xlz_ctx *, const xlz_stream_desc *, size_t, xlz_result *, const PostWork &) { return XLZ_ERR_DEVICE; }
int xlz_internal_decode_device(xlz_ctx *, const xlz_stream_desc *, size_t, xlz_result *, const PostWork &, const DeviceDest &) { return XLZ_ERR_DEVICE; }
int xlz_internal_device_block(xlz_ctx *, size_t, void **) { return XLZ_ERR_DEVICE; }
int xlz_internal_device_block_download(xlz_ctx *, const void *, uint8_t *, size_t) { return XLZ_ERR_DEVICE; }
void xlz_internal_device_block_release(xlz_ctx *, void *) {}

static uint64_t g_seed = 1;
static uint32_t rnd()
{
    g_seed ^= g_seed << 13, g_seed ^= g_seed >> 7, g_seed ^= g_seed << 17;
    return (uint32_t)(g_seed >> 11);
}

static void put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8), p[2] = (uint8_t)(v >> 16), p[3] = (uint8_t)(v >> 24); }

static long g_ok = 0, g_bcj2 = 0;
static void index_all(const std::vector<uint8_t> &a)
{
    size_t nf = 0, ns = 0, nst = 0, nb = 0;
    uint64_t total = 0;
    int st = xlz_7z_index_bcj2(nullptr, a.data(), a.size(), nullptr, 0, &nf, nullptr, 0, &ns, nullptr, 0, &nst, nullptr, 0, &nb, &total);
    if (st == XLZ_OK) {
        // arrays of exactly the counted sizes (heap: a write past them is seen)
        std::vector<xlz_7z_folder> fo(nf);
        std::vector<xlz_7z_substream> su(ns);
        std::vector<xlz_filter_step> fs(nst);
        std::vector<xlz_7z_bcj2> br(nb);
        size_t nf2 = 0, ns2 = 0, nst2 = 0, nb2 = 0;
        st = xlz_7z_index_bcj2(nullptr, a.data(), a.size(), fo.data(), nf, &nf2, su.data(), ns, &ns2, fs.data(), nst, &nst2, br.data(), nb, &nb2, &total);
        if (st != XLZ_OK || nf2 != nf || ns2 != ns || nst2 != nst || nb2 != nb) {
            printf("FAIL: the second pass disagrees with the first (%d)\n", st);
            exit(1);
        }
        for (const xlz_7z_bcj2 &r : br) { // every record names a BCJ2 folder and places its streams inside the file
            const xlz_7z_bcj2_sub *sub[3] = {&r.main_s, &r.call_s, &r.jump_s};
            bool ok = r.folder < nf && fo[(size_t)r.folder].method == XLZ_7Z_BCJ2 && r.rc_off <= a.size() && r.rc_len <= a.size() - r.rc_off;
            for (const xlz_7z_bcj2_sub *s : sub) ok = ok && s->pack_off <= a.size() && s->pack_len <= a.size() - s->pack_off;
            if (!ok) {
                printf("FAIL: a record reaches outside the file\n");
                exit(1);
            }
        }
        g_ok++, g_bcj2 += (long)nb;
    }
    size_t n1 = 0, n2 = 0, n3 = 0;
    (void)xlz_7z_index(nullptr, a.data(), a.size(), nullptr, 0, &n1, nullptr, 0, &n2, &total);
    (void)xlz_7z_index_chains(nullptr, a.data(), a.size(), nullptr, 0, &n1, nullptr, 0, &n2, nullptr, 0, &n3, &total);
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const long rounds = atol(argv[1]);
    long cases = 0;
    for (int k = 2; k < argc; k++) {
        FILE *f = fopen(argv[k], "rb");
        if (!f) return 2;
        std::vector<uint8_t> seed;
        uint8_t buf[65536];
        for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) seed.insert(seed.end(), buf, buf + n);
        fclose(f);
        if (seed.size() < 32) return 2;
        const uint64_t hoff = le64(seed.data() + 12), hlen = le64(seed.data() + 20);
        if (hoff > seed.size() - 32 || hlen > seed.size() - 32 - hoff || hlen == 0) return 2;
        index_all(seed);
        g_seed = 0x1234567 + (uint64_t)k;
        for (long r = 0; r < rounds; r++, cases++) {
            std::vector<uint8_t> a = seed;
            uint8_t *h = a.data() + 32 + hoff;
            const uint32_t n_mut = 1 + rnd() % 4;
            for (uint32_t m = 0; m < n_mut; m++) {
                const size_t at = rnd() % hlen;
                switch (rnd() % 4) {
                case 0: h[at] = (uint8_t)rnd(); break;
                case 1: h[at] ^= (uint8_t)(1u << (rnd() % 8)); break;
                case 2: h[at] = (uint8_t)(h[at] + 1); break;
                default: h[at] = (uint8_t)(rnd() % 8); break; // (small numbers: coder counts, stream indices)
                }
            }
            size_t len = hlen;
            if (rnd() % 16 == 0) len = rnd() % hlen + 1; // a header cut short
            a.resize(32 + hoff + len);
            put32(a.data() + 20 + 0, (uint32_t)len), put32(a.data() + 24, 0);
            put32(a.data() + 28, xlzcheck::crc32(a.data() + 32 + hoff, len));
            put32(a.data() + 8, xlzcheck::crc32(a.data() + 12, 20));
            index_all(a);
        }
    }
    printf("%ld mutated headers, %ld indexed, %ld BCJ2 records among them\nok\n", cases, g_ok, g_bcj2);
    return 0;
}
