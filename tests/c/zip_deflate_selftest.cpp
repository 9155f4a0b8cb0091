// zip_deflate_selftest.cpp -- what lzma_amd/csrc/xlz_zip.h decides about deflate (method 8) entries, without a GPU and
// without the library.  A plain C++ program over one archive (tests/golden/infozip.zip: Info-ZIP wrote two deflate entries
// into it):
//   g++ -O2 -std=c++17 -I lzma_amd/csrc tests/c/zip_deflate_selftest.cpp -o t && ./t tests/golden/infozip.zip
// The classes of open stay as they were and XLZ_ZIP_ENTRY_DEFLATE stands beside them; plan() in deflate mode 0 -- also
// when the mode is not passed at all -- is the plan of old: a deflate entry is settled as unsupported and nothing is
// inflated; in mode 1 and 2 it becomes an inflate item INTO the file, with a CRC32 range over the destination; and
// inflate_status folds an item's outcome into the entry's.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "xlz_zip.h"

using namespace xlzzip;

static int g_fail = 0;
static long g_cases = 0;
#define CHECK(c, ...)                                                                                                  \
    do {                                                                                                               \
        g_cases++;                                                                                                     \
        if (!(c)) {                                                                                                    \
            if (g_fail++ < 20) printf("FAIL %s:%d: ", __FILE__, __LINE__), printf(__VA_ARGS__), printf("\n");          \
        }                                                                                                              \
    } while (0)

static bool same_plan(const Plan &a, const Plan &b)
{
    if (a.pre != b.pre || a.stream_want != b.stream_want || a.span_want != b.span_want || a.inflate_want != b.inflate_want) return false;
    if (a.streams.size() != b.streams.size() || a.spans.size() != b.spans.size() || a.items.size() != b.items.size()) return false;
    for (size_t k = 0; k < a.streams.size(); k++)
        if (a.streams[k].in != b.streams[k].in || a.streams[k].in_len != b.streams[k].in_len || a.streams[k].out_cap != b.streams[k].out_cap) return false;
    for (size_t k = 0; k < a.spans.size(); k++)
        if (a.spans[k].dst != b.spans[k].dst || a.spans[k].src_off != b.spans[k].src_off || a.spans[k].len != b.spans[k].len) return false;
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> file(1 << 20);
    file.resize(fread(file.data(), 1, file.size(), f));
    fclose(f);
    Table t;
    CHECK(parse(file.data(), file.size(), t) == XLZ_OK, "the archive does not open");
    size_t n_deflate = 0;
    for (const xlz_zip_entry &x : t.entries) {
        const bool deflate = (x.flags & XLZ_ZIP_ENTRY_DEFLATE) != 0;
        CHECK(deflate == (x.method == kDeflate), "the deflate bit and method %u", x.method);
        CHECK(!deflate || !(x.flags & (XLZ_ZIP_ENTRY_SUPPORTED | XLZ_ZIP_ENTRY_BAD)), "a deflate entry has a class bit");
        CHECK(!deflate || unsupported(x), "a deflate entry is not unsupported any more");
        CHECK(deflate || is_dir(x) || (x.flags & XLZ_ZIP_ENTRY_SUPPORTED), "a stored entry lost its class");
        n_deflate += deflate;
    }
    CHECK(n_deflate == 2, "%zu deflate entries", n_deflate);
    // every entry wanted once, windows of the sizes back to back
    std::vector<xlz_zip_want> w(t.entries.size());
    for (size_t i = 0; i < w.size(); i++) w[i].entry = i;
    uint64_t total = 0;
    CHECK(layout(t.entries.data(), w.data(), w.size(), 16, &total), "layout");
    std::vector<uint64_t> dst(w.size());
    for (size_t i = 0; i < w.size(); i++) dst[i] = w[i].dst_off;
    Plan old_form, mode0, mode1, mode2;
    plan(file.data(), t.entries.data(), w.data(), dst.data(), w.size(), old_form);
    plan(file.data(), t.entries.data(), w.data(), dst.data(), w.size(), mode0, 0);
    plan(file.data(), t.entries.data(), w.data(), dst.data(), w.size(), mode1, 1);
    plan(file.data(), t.entries.data(), w.data(), dst.data(), w.size(), mode2, 2);
    CHECK(same_plan(old_form, mode0), "mode 0 is not the plan without a mode");
    CHECK(mode0.inflate.empty() && mode0.inflate_want.empty(), "mode 0 inflates");
    CHECK(mode1.inflate.size() == 2 && same_plan(mode1, mode2), "mode 1 / 2: %zu items", mode1.inflate.size());
    CHECK(mode1.spans.size() == mode0.spans.size() && mode1.streams.size() == mode0.streams.size(), "the other entries changed");
    for (size_t i = 0; i < w.size(); i++) {
        const xlz_zip_entry &x = t.entries[i];
        const bool deflate = (x.flags & XLZ_ZIP_ENTRY_DEFLATE) != 0;
        CHECK(mode0.pre[i] == (deflate && has_bytes(x) ? (int32_t)XLZ_ERR_UNSUPPORTED : (int32_t)XLZ_OK), "mode 0, entry %zu: %d", i, mode0.pre[i]);
        CHECK(mode1.pre[i] == XLZ_OK, "mode 1, entry %zu: %d", i, mode1.pre[i]);
    }
    for (size_t k = 0; k < mode1.inflate.size(); k++) {
        const size_t i = mode1.inflate_want[k];
        const xlz_zip_entry &x = t.entries[w[i].entry];
        const xlz_inflate_item &it = mode1.inflate[k];
        CHECK(it.in == file.data() + x.data_off && it.in_len == x.comp_size && it.dst_off == dst[i] && it.dst_cap == x.size, "item %zu", k);
    }
    std::vector<xlz_check_range> cr;
    std::vector<size_t> range_of;
    check_ranges(mode1, w.size(), cr, range_of);
    for (size_t k = 0; k < mode1.inflate.size(); k++) {
        const size_t q = range_of[mode1.inflate_want[k]];
        CHECK(q != kNone && cr[q].stream == kDestStream && cr[q].off == mode1.inflate[k].dst_off && cr[q].len == mode1.inflate[k].dst_cap &&
                  cr[q].kind == XLZ_CHECK_CRC32,
              "range of item %zu", k);
    }
    check_ranges(mode0, w.size(), cr, range_of);
    for (size_t i = 0; i < w.size(); i++)
        CHECK(!(t.entries[i].flags & XLZ_ZIP_ENTRY_DEFLATE) || range_of[i] == kNone, "mode 0 checks a deflate entry");
    // a window one byte short settles a deflate entry before the batch, in every mode
    {
        std::vector<xlz_zip_want> s = w;
        const size_t i = mode1.inflate_want[0];
        s[i].dst_cap--;
        Plan p;
        plan(file.data(), t.entries.data(), s.data(), dst.data(), s.size(), p, 1);
        CHECK(p.pre[i] == XLZ_ERR_OUT_CAP && p.inflate.size() == 1, "a short window: %d", p.pre[i]);
    }
    // the verdict of an item
    xlz_zip_entry x = t.entries[w[mode1.inflate_want[0]].entry];
    CHECK(inflate_status(x, XLZ_OK, x.size) == XLZ_OK, "good");
    CHECK(inflate_status(x, XLZ_OK, x.size - 1) == XLZ_ERR_RESULT, "short");
    CHECK(inflate_status(x, XLZ_ERR_OUT_CAP, 0) == XLZ_ERR_RESULT, "out_cap");
    CHECK(inflate_status(x, XLZ_ERR_UNEXPECTED_EOF, 0) == XLZ_ERR_UNEXPECTED_EOF, "eof");
    CHECK(inflate_status(x, XLZ_ERR_RESULT, 0) == XLZ_ERR_RESULT, "result");
    // what does NOT get the bit
    for (int kind = 0; kind < 4; kind++) {
        std::vector<uint8_t> g = file;
        Table u;
        // the first deflate entry's central record: its method (offset 10) or flags (offset 8)
        uint64_t pos = t.end.cd_pos;
        size_t idx = 0;
        for (; idx < t.entries.size() && t.entries[idx].method != kDeflate; idx++) pos += kCentralLen + le16(g.data() + pos + 28) + le16(g.data() + pos + 30) + le16(g.data() + pos + 32);
        if (kind == 0) g[pos + 10] = 9;       // Deflate64
        if (kind == 1) g[pos + 8] |= 1;       // encrypted
        if (kind == 2) g[pos + 8] |= 1u << 5; // patched data
        if (kind == 3) g[pos + 42] = 0xFF, g[pos + 43] = 0xFF, g[pos + 44] = 0x7F; // a local header out of the file
        CHECK(parse(g.data(), g.size(), u) == XLZ_OK, "kind %d does not open", kind);
        CHECK(!(u.entries[idx].flags & XLZ_ZIP_ENTRY_DEFLATE), "kind %d keeps the deflate bit", kind);
        CHECK(((u.entries[idx].flags & XLZ_ZIP_ENTRY_BAD) != 0) == (kind == 3), "kind %d: bad", kind);
    }
    printf("%ld checks, %d failures\n", g_cases, g_fail);
    return g_fail ? 1 : 0;
}
