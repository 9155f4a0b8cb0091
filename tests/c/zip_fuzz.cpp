// zip_fuzz.cpp -- a seeded mutation loop over .zip archives through xlz_zip_open, the entries and the layout, as a
// stand-alone program: lzma_amd/csrc/xlz_zip.hip (with xlz_zip.h) is host-only code and is compiled INTO this program;
// what it calls of the rest of the library is stubbed (nothing here extracts).  Meant to be built with
// -fsanitize=address,undefined.  Most mutations fall into the central directory and the end records, some into the
// local headers; some archives are cut.  Every archive that opens has its table fetched into arrays of exactly the
// counted sizes and walked: names inside the pool and terminated, the payload of every entry that is not bad inside the
// file and READ from end to end, the layout and the plan of all entries formed, every stream and span of the plan read.
//   g++ -O1 -g -std=c++17 -x c++ -fsanitize=address,undefined -I include tests/c/zip_fuzz.cpp -o f && ./f ROUNDS a.zip b.zip ...
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../lzma_amd/csrc/xlz_zip.hip"

// ---- what xlz_zip.hip calls of xlz_host.hip ----
void xlz_internal_check_stats_reset(xlz_ctx *) {}
void xlz_internal_pack_stats_reset(xlz_ctx *) {}
void xlz_internal_zip_extract_stats_set(xlz_ctx *, const xlz_zip_extract_stats &) {}
int xlz_internal_device_dst_ok(xlz_ctx *, const void *, size_t) { return XLZ_ERR_DEVICE; }
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

static void fail(const char *what)
{
    printf("FAIL: %s\n", what);
    exit(1);
}

static long g_opened = 0, g_refused = 0, g_entries = 0, g_bad = 0;
static volatile uint32_t g_sink = 0;
static void touch(const uint8_t *p, size_t n)
{
    uint32_t s = 0;
    for (size_t k = 0; k < n; k++) s += p[k];
    g_sink = g_sink + s;
}

static void open_all(const uint8_t *file, size_t len)
{
    xlz_zip_archive *h = nullptr;
    const int st = xlz_zip_open(file, len, &h);
    if (st != XLZ_OK) {
        if (h) fail("a handle behind a refused open");
        if (st != XLZ_ERR_RESULT && st != XLZ_ERR_UNEXPECTED_EOF && st != XLZ_ERR_UNSUPPORTED) fail("open refuses with a status it does not document");
        g_refused++;
        return;
    }
    size_t ne = 0, nb = 0;
    uint64_t total = 0, shift = 0;
    if (xlz_zip_archive_info(h, &ne, &nb, &total, &shift) != XLZ_OK || shift > len) fail("archive_info");
    std::vector<xlz_zip_entry> e(ne); // arrays of exactly the counted sizes (heap: a write past them is seen)
    std::vector<char> names(nb);
    if (xlz_zip_archive_entries(h, e.data(), ne, names.data(), nb) != XLZ_OK) fail("archive_entries");
    if (ne && xlz_zip_archive_entries(h, e.data(), ne - 1, names.data(), nb) != XLZ_ERR_OUT_CAP) fail("a short entry array is not reported");
    std::vector<xlz_zip_want> w(ne);
    for (size_t i = 0; i < ne; i++) {
        const xlz_zip_entry &x = e[i];
        if (x.name_off > nb || x.name_len >= nb - x.name_off || names[x.name_off + x.name_len] != 0) fail("a name leaves the pool or is not terminated");
        const bool bad = x.flags & XLZ_ZIP_ENTRY_BAD, ok = x.flags & XLZ_ZIP_ENTRY_SUPPORTED;
        if (bad && ok) fail("an entry is supported and bad");
        if (!bad) {
            if (x.data_off > len || x.comp_size > len - x.data_off || x.header_off > x.data_off) fail("a payload leaves the file");
            touch(file + x.header_off, 30), touch(file + x.data_off, (size_t)x.comp_size);
            if (ok && x.method == 14 && (x.comp_size < 9 || x.props >= 225)) fail("a malformed LZMA header is supported");
        }
        g_bad += bad;
        w[i] = xlz_zip_want{i, 0, 0};
    }
    uint64_t laid = 0;
    const int ls = xlz_zip_extract_layout(h, w.data(), ne, 1 + rnd() % 64, &laid);
    if (ls != XLZ_OK && ls != XLZ_ERR_OUT_CAP) fail("layout");
    if (ls == XLZ_OK) {
        if (laid < total) fail("the layout is shorter than the entries");
        std::vector<uint64_t> dst(ne);
        for (size_t i = 0; i < ne; i++) dst[i] = w[i].dst_off;
        xlzzip::Plan p;
        xlzzip::plan(file, e.data(), w.data(), dst.data(), ne, p);
        for (const xlz_stream_desc &d : p.streams) touch(d.in, d.in_len);
        for (const xlzzip::Span &s : p.spans) touch(file + s.src_off, (size_t)s.len);
        // (the argument tests of an extraction, which end at the missing context)
        std::vector<xlz_zip_file_result> res(ne);
        uint8_t out[1];
        if (ne && xlz_zip_extract(nullptr, h, w.data(), ne, out, (size_t)laid, 1, res.data()) != XLZ_ERR_BAD_ARG) fail("an extraction without a context");
    }
    g_opened++, g_entries += (long)ne;
    xlz_zip_close(h);
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
        size_t end_pos;
        if (!xlzzip::find_end(seed.data(), seed.size(), &end_pos)) return 2;
        xlzzip::End e;
        if (xlzzip::read_end(seed.data(), seed.size(), e) != XLZ_OK) return 2;
        const size_t cd = (size_t)e.cd_pos, tail = seed.size() - cd;
        open_all(seed.data(), seed.size());
        g_seed = 0x2468ACE1 + (uint64_t)k;
        for (long r = 0; r < rounds; r++, cases++) {
            // (a heap copy of exactly the archive's size: a read past its end is seen)
            std::vector<uint8_t> a = seed;
            const uint32_t n_mut = 1 + rnd() % 4;
            for (uint32_t m = 0; m < n_mut; m++) {
                const uint32_t where = rnd() % 8;
                const size_t at = where < 5 ? cd + rnd() % tail : where < 7 ? seed.size() - 1 - rnd() % std::min<size_t>(seed.size(), 98) : rnd() % seed.size();
                switch (rnd() % 6) {
                case 0: a[at] = (uint8_t)rnd(); break;
                case 1: a[at] ^= (uint8_t)(1u << (rnd() % 8)); break;
                case 2: a[at] = (uint8_t)(a[at] + 1); break;
                case 3: a[at] = 0xFF; break;                 // (all-ones fields: the ZIP64 paths)
                case 4: a[at] = 0; break;
                default: a[at] = (uint8_t)(rnd() % 16); break; // (small numbers: counts, lengths, methods)
                }
            }
            if (rnd() % 16 == 0) {
                a.resize(rnd() % a.size() + 1); // an archive cut short
                a.shrink_to_fit();
            }
            std::vector<uint8_t> exact(a.begin(), a.end());
            open_all(exact.data(), exact.size());
        }
    }
    printf("%ld mutated archives, %ld opened, %ld refused, %ld entries in all, %ld bad\nok\n", cases, g_opened, g_refused, g_entries, g_bad);
    return 0;
}
