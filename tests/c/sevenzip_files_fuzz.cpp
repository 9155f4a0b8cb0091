// sevenzip_files_fuzz.cpp -- a seeded mutation loop over the headers of .7z archives with a FilesInfo section, through
// xlz_7z_open(NULL, ...), as a stand-alone program: the parser of lzma_amd/csrc/xlz_7z.hip (with xlz_7z_files.h) is
// host-only code and is compiled INTO this program, what it calls of the rest of the library is stubbed (an open with
// ctx == NULL on a plain header never gets there).  Meant to be built with -fsanitize=address,undefined: the header's CRCs
// are mended so that the mutation reaches the parser, and every archive that opens has its table fetched into arrays of
// exactly the counted sizes and walked -- names inside the pool and terminated, entries inside their folders.
//   g++ -O1 -g -std=c++17 -x c++ -fsanitize=address,undefined -I include tests/c/sevenzip_files_fuzz.cpp -o f && ./f ROUNDS a.7z b.7z ...
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

static void fail(const char *what)
{
    printf("FAIL: %s\n", what);
    exit(1);
}

static long g_opened = 0, g_refused = 0, g_entries = 0;
static void open_all(const std::vector<uint8_t> &a)
{
    xlz_7z_archive *h = nullptr;
    const int st = xlz_7z_open(nullptr, a.data(), a.size(), &h);
    size_t nf0 = 0, ns0 = 0, nst0 = 0, nb0 = 0;
    uint64_t total0 = 0;
    const int st_index = xlz_7z_index_bcj2(nullptr, a.data(), a.size(), nullptr, 0, &nf0, nullptr, 0, &ns0, nullptr, 0, &nst0, nullptr, 0, &nb0, &total0);
    if (st != XLZ_OK) {
        if (h) fail("a handle behind a refused open");
        g_refused++;
        return;
    }
    if (st_index != XLZ_OK) fail("the archive opens, but does not index"); // (FilesInfo is all that may refuse more)
    size_t ne = 0, nf = 0, nb = 0;
    uint64_t total = 0;
    if (xlz_7z_archive_info(h, &ne, &nf, &nb, &total) != XLZ_OK || nf != nf0) fail("archive_info");
    // arrays of exactly the counted sizes (heap: a write past them is seen)
    std::vector<xlz_7z_entry> e(ne);
    std::vector<char> names(nb);
    std::vector<xlz_7z_folder> fo(nf);
    if (xlz_7z_archive_entries(h, e.data(), ne, names.data(), nb) != XLZ_OK) fail("archive_entries");
    if (xlz_7z_archive_folders(h, fo.data(), nf) != XLZ_OK) fail("archive_folders");
    if (ne && xlz_7z_archive_entries(h, e.data(), ne - 1, names.data(), nb) != XLZ_ERR_OUT_CAP) fail("a short entry array is not reported");
    uint64_t sum = 0;
    size_t with_stream = 0;
    for (const xlz_7z_entry &x : e) {
        if (x.name_off > nb || x.name_len > nb - x.name_off) fail("a name leaves the pool");
        if (nb && (x.name_off + x.name_len >= nb || names[x.name_off + x.name_len] != 0)) fail("a name is not terminated");
        if (x.flags & XLZ_7Z_ENTRY_HAS_STREAM) {
            if (x.folder >= nf || x.size > fo[x.folder].unpack_len || x.folder_off > fo[x.folder].unpack_len - x.size) fail("an entry leaves its folder");
            with_stream++;
        } else if (x.folder != XLZ_7Z_NO_FOLDER || x.size) {
            fail("an entry without a stream has bytes");
        }
        sum += x.size;
    }
    if (sum != total || (ne && with_stream != ns0)) fail("sizes or counts disagree");
    g_opened++, g_entries += (long)ne;
    xlz_7z_close(h);
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
        open_all(seed);
        g_seed = 0x7654321 + (uint64_t)k;
        for (long r = 0; r < rounds; r++, cases++) {
            std::vector<uint8_t> a = seed;
            uint8_t *h = a.data() + 32 + hoff;
            const uint32_t n_mut = 1 + rnd() % 4;
            for (uint32_t m = 0; m < n_mut; m++) {
                // (half of the mutations in the last third of the header, where FilesInfo lies)
                const size_t at = rnd() % 2 ? rnd() % hlen : hlen - 1 - rnd() % (hlen / 3 + 1);
                switch (rnd() % 5) {
                case 0: h[at] = (uint8_t)rnd(); break;
                case 1: h[at] ^= (uint8_t)(1u << (rnd() % 8)); break;
                case 2: h[at] = (uint8_t)(h[at] + 1); break;
                case 3: h[at] = (uint8_t)(0x0E + rnd() % 12); break; // (property ids)
                default: h[at] = (uint8_t)(rnd() % 8); break;        // (small numbers: counts, sizes)
                }
            }
            size_t len = hlen;
            if (rnd() % 16 == 0) len = rnd() % hlen + 1; // a header cut short
            a.resize(32 + hoff + len);
            put32(a.data() + 20 + 0, (uint32_t)len), put32(a.data() + 24, 0);
            put32(a.data() + 28, xlzcheck::crc32(a.data() + 32 + hoff, len));
            put32(a.data() + 8, xlzcheck::crc32(a.data() + 12, 20));
            open_all(a);
        }
    }
    printf("%ld mutated headers, %ld opened, %ld refused, %ld entries in all\nok\n", cases, g_opened, g_refused, g_entries);
    return 0;
}
