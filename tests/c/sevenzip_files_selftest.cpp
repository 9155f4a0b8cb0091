// sevenzip_files_selftest.cpp -- lzma_amd/csrc/xlz_7z_files.h without a GPU, against brute-force models.  Seeded random
// folder / entry layouts (solid folders, entries without bytes, every method, chains, hand-made unit tables): the reach of
// a want list and the cover against a destination-free byte marking; the cut of a folder -- by capacity, at a unit
// boundary, never -- against a walk over the units; the layout against 128-bit sums; the windows against a destination in
// which every window marks its bytes; the pack items against a copy per want over folders whose bytes name themselves;
// the outcome a cut stream must end in and the verdict fold for every combination of stream outcome x digest outcome; the
// name pool for surrogate pairs and unpaired surrogates.  Built plain and with the host sanitizers
// (tests/test_sevenzip_files_cpu.py).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "xlz_7z_files.h"

using namespace xlz7zf;

static int fails = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            if (fails++ < 20) printf("%s:%d: %s\n", __FILE__, __LINE__, #c); \
        }                                                          \
    } while (0)

static const uint64_t kTop = ~(uint64_t)0;

struct Archive {
    std::vector<FolderShape> fs;
    std::vector<std::vector<xlz_lzma2_unit>> units;
    std::vector<xlz_7z_entry> e;
};

// a unit table of `nu` units over (pack_len, unpack_len), back to back; `broken`: one that must not be trusted
static std::vector<xlz_lzma2_unit> make_units(std::mt19937_64 &rnd, size_t nu, uint64_t pack_len, uint64_t unpack_len, bool broken)
{
    std::vector<xlz_lzma2_unit> u(nu);
    uint64_t in_at = 0, out_at = 0;
    for (size_t k = 0; k < nu; k++) {
        memset(&u[k], 0, sizeof u[k]);
        const uint64_t in_left = pack_len - in_at, out_left = unpack_len - out_at;
        u[k].in_off = in_at, u[k].out_off = out_at;
        u[k].in_len = k + 1 == nu ? in_left : rnd() % (in_left + 1);
        u[k].out_len = k + 1 == nu ? out_left : rnd() % (out_left + 1);
        in_at += u[k].in_len, out_at += u[k].out_len;
    }
    if (broken && nu >= 2) {
        switch (rnd() % 3) {
        case 0: u[nu - 1].out_len += 1; break;                 // does not add up
        case 1: u[1].out_off += 1; break;                      // a gap
        default: u[nu - 1].in_len = pack_len + 1; break;       // leaves the payload
        }
    }
    return u;
}

static Archive make_archive(std::mt19937_64 &rnd)
{
    Archive a;
    const size_t nf = rnd() % 5;
    const uint32_t methods[] = {XLZ_7Z_LZMA, XLZ_7Z_LZMA2, XLZ_7Z_LZMA2, XLZ_7Z_COPY, XLZ_7Z_BCJ2, XLZ_7Z_UNSUPPORTED};
    a.units.resize(nf);
    for (size_t k = 0; k < nf; k++) {
        const size_t files = rnd() % 5;
        uint64_t off = 0;
        for (size_t j = 0; j < files; j++) {
            xlz_7z_entry x;
            memset(&x, 0, sizeof x);
            x.flags = XLZ_7Z_ENTRY_HAS_STREAM | (rnd() % 4 ? XLZ_7Z_ENTRY_HAS_CRC : 0);
            x.size = rnd() % 4 == 0 ? 0 : rnd() % 30, x.folder = k, x.folder_off = off, x.substream = a.e.size();
            off += x.size;
            a.e.push_back(x);
            if (rnd() % 4 == 0) { // an entry without a stream in between
                xlz_7z_entry d;
                memset(&d, 0, sizeof d);
                d.folder = d.substream = XLZ_7Z_NO_FOLDER, d.flags = XLZ_7Z_ENTRY_IS_DIR;
                a.e.push_back(d);
            }
        }
        FolderShape f;
        f.method = methods[rnd() % 6];
        f.steps = (f.method == XLZ_7Z_LZMA || f.method == XLZ_7Z_LZMA2) && rnd() % 4 == 0;
        f.usable = !f.steps || rnd() % 2;
        f.unpack_len = off, f.pack_len = 1 + rnd() % 40;
        if (f.method == XLZ_7Z_LZMA2 && rnd() % 5) a.units[k] = make_units(rnd, 1 + rnd() % 4, f.pack_len, f.unpack_len, rnd() % 6 == 0);
        a.fs.push_back(f);
    }
    for (size_t k = 0; k < nf; k++) a.fs[k].units = a.units[k].data(), a.fs[k].n_units = a.units[k].size();
    if (a.e.empty() || rnd() % 3 == 0) {
        xlz_7z_entry d;
        memset(&d, 0, sizeof d);
        d.folder = d.substream = XLZ_7Z_NO_FOLDER;
        a.e.push_back(d);
    }
    return a;
}

// the model of cut_folder: the units walked one by one
static Cut model_cut(const FolderShape &f, uint64_t P)
{
    const Cut whole = {f.unpack_len, f.pack_len, kWhole};
    if (f.steps || (f.method != XLZ_7Z_LZMA && f.method != XLZ_7Z_LZMA2) || P >= f.unpack_len) return whole;
    if (f.method == XLZ_7Z_LZMA) return Cut{P, f.pack_len, kCapCut};
    if (f.n_units == 0) return whole;
    if (f.n_units == 1) return Cut{P, f.pack_len, kCapCut};
    unsigned __int128 in_sum = 0, out_sum = 0;
    for (size_t k = 0; k < f.n_units; k++) {
        if (f.units[k].in_off != in_sum || f.units[k].out_off != out_sum) return whole;
        in_sum += f.units[k].in_len, out_sum += f.units[k].out_len;
        if (in_sum > f.pack_len || out_sum > f.unpack_len) return whole;
    }
    if (out_sum != f.unpack_len) return whole;
    for (size_t k = 0; k < f.n_units; k++) // the unit that holds byte P - 1
        if (f.units[k].out_off <= P - 1 && P - 1 < f.units[k].out_off + f.units[k].out_len) {
            if (k + 1 == f.n_units || f.units[k].out_off + f.units[k].out_len == f.unpack_len) return whole; // (nothing behind it)
            // (empty units behind it belong to the cut: the input ends where the next unit WITH bytes behind P begins --
            //  any boundary between the two is an end of unit k's bytes; the header takes the first)
            return Cut{f.units[k].out_off + f.units[k].out_len, f.units[k].in_off + f.units[k].in_len, kUnitCut};
        }
    return whole;
}

static void plan_case(std::mt19937_64 &rnd)
{
    const Archive a = make_archive(rnd);
    const size_t nf = a.fs.size(), n = rnd() % 8;
    std::vector<xlz_7z_want> w(n);
    std::vector<uint64_t> dst(n), wanted(n);
    uint64_t at = 0;
    for (size_t i = 0; i < n; i++) {
        w[i].entry = rnd() % a.e.size(), wanted[i] = w[i].entry;
        const uint64_t size = a.e[(size_t)w[i].entry].size;
        w[i].dst_cap = rnd() % 5 == 0 && size ? size - 1 : size + rnd() % 3; // now and then a short window
        at += rnd() % 3;
        w[i].dst_off = dst[i] = at, at += w[i].dst_cap;
    }
    const uint64_t cap = at;
    CHECK(wants_ok(a.e.data(), a.e.size(), w.data(), n, cap));
    // ---- reach and cover over ALL wanted entries (xlz_7z_cover): the bytes marked folder by folder
    std::vector<uint64_t> P;
    reach(a.e.data(), wanted.data(), nullptr, n, nf, P);
    for (size_t k = 0; k < nf; k++) {
        std::vector<uint8_t> mark((size_t)a.fs[k].unpack_len, 0);
        for (size_t i = 0; i < n; i++) {
            const xlz_7z_entry &x = a.e[(size_t)wanted[i]];
            if ((x.flags & XLZ_7Z_ENTRY_HAS_STREAM) && x.folder == k)
                for (uint64_t j = 0; j < x.size; j++) mark[(size_t)(x.folder_off + j)] = 1;
        }
        uint64_t last = 0;
        for (size_t j = 0; j < mark.size(); j++)
            if (mark[j]) last = j + 1;
        CHECK(P[k] == last);
        if (!last) continue;
        const Cut c = cut_folder(a.fs[k].method, a.fs[k].steps, a.fs[k].unpack_len, a.fs[k].pack_len, a.fs[k].units, a.fs[k].n_units, last);
        const Cut m = model_cut(a.fs[k], last);
        CHECK(c.kind == m.kind && c.decode_len == m.decode_len);
        CHECK(c.decode_len >= last && c.decode_len <= a.fs[k].unpack_len && c.in_len <= a.fs[k].pack_len);
        if (c.kind == kUnitCut) { // a boundary of the table, behind the model's unit and in front of the next unit with bytes
            bool boundary = false;
            for (size_t q = 0; q < a.fs[k].n_units; q++) boundary |= a.fs[k].units[q].out_off == c.decode_len && a.fs[k].units[q].in_off == c.in_len;
            CHECK(boundary && c.in_len >= m.in_len);
        } else {
            CHECK(c.in_len == a.fs[k].pack_len);
        }
        if (c.kind != kWhole) CHECK(c.decode_len < a.fs[k].unpack_len);
    }
    // ---- the plan: what settles a want, the cover of the rest, the streams, the items
    Plan p;
    plan(a.e.data(), a.fs.data(), nf, w.data(), dst.data(), n, p);
    CHECK(p.pre.size() == n);
    std::vector<uint8_t> left(n, 0);
    for (size_t i = 0; i < n; i++) {
        const xlz_7z_entry &x = a.e[(size_t)w[i].entry];
        int32_t want = XLZ_OK;
        if ((x.flags & XLZ_7Z_ENTRY_HAS_STREAM) && x.size) {
            const FolderShape &f = a.fs[(size_t)x.folder];
            if (w[i].dst_cap < x.size)
                want = XLZ_ERR_OUT_CAP;
            else if (f.method == XLZ_7Z_BCJ2 || f.method == XLZ_7Z_UNSUPPORTED || (f.steps && !f.usable))
                want = XLZ_ERR_UNSUPPORTED;
            else
                left[i] = 1;
        }
        CHECK(p.pre[i] == want);
    }
    std::vector<size_t> folders; // ascending, duplicate-free, the folders of the wants that are left
    for (size_t k = 0; k < nf; k++) {
        bool any = false;
        for (size_t i = 0; i < n; i++) any |= left[i] && a.e[(size_t)w[i].entry].folder == k;
        if (any) folders.push_back(k);
    }
    CHECK(p.folders == folders && p.cuts.size() == folders.size());
    size_t streams = 0;
    for (size_t q = 0; q < folders.size() && q < p.cuts.size(); q++) {
        const size_t k = folders[q];
        uint64_t last = 0;
        for (size_t i = 0; i < n; i++)
            if (left[i] && a.e[(size_t)w[i].entry].folder == k) last = std::max(last, a.e[(size_t)w[i].entry].folder_off + a.e[(size_t)w[i].entry].size);
        const Cut m = model_cut(a.fs[k], last);
        CHECK(p.cuts[q].kind == m.kind && p.cuts[q].decode_len == m.decode_len);
        if (a.fs[k].method == XLZ_7Z_COPY) {
            CHECK(p.stream_of[k] == kNoStream && p.cuts[q].kind == kWhole);
        } else {
            CHECK(p.stream_of[k] == streams && p.stream_folder[streams] == k);
            streams++;
        }
    }
    CHECK(p.stream_folder.size() == streams);
    // the items, run over folders whose bytes name themselves, against a copy per want; bytes outside stay untouched; every
    // item lies inside what its stream is asked to decode
    auto byte_of = [](size_t folder, uint64_t off) { return (uint8_t)(1 + (folder * 37 + off * 11) % 250); };
    std::vector<uint8_t> got((size_t)cap, 0), want((size_t)cap, 0);
    CHECK(p.items.size() == p.item_want.size());
    for (size_t j = 0; j < p.items.size(); j++) {
        const xlz_pack_item &it = p.items[j];
        CHECK(it.stream < streams && it.len > 0);
        if (it.stream >= streams) continue;
        const size_t k = p.stream_folder[(size_t)it.stream];
        size_t q = 0;
        while (p.folders[q] != k) q++;
        CHECK(it.off + it.len <= p.cuts[q].decode_len);
        for (uint64_t b = 0; b < it.len; b++) {
            CHECK(it.dst_off + b < cap && got[(size_t)(it.dst_off + b)] == 0);
            if (it.dst_off + b < cap) got[(size_t)(it.dst_off + b)] = byte_of(k, it.off + b);
        }
    }
    for (size_t i : p.copy_wants) {
        const xlz_7z_entry &x = a.e[(size_t)w[i].entry];
        CHECK(left[i] && a.fs[(size_t)x.folder].method == XLZ_7Z_COPY);
        for (uint64_t b = 0; b < x.size; b++) got[(size_t)(dst[i] + b)] = byte_of((size_t)x.folder, x.folder_off + b);
    }
    for (size_t i = 0; i < n; i++) {
        const xlz_7z_entry &x = a.e[(size_t)w[i].entry];
        for (uint64_t b = 0; b < x.size && left[i]; b++) want[(size_t)(dst[i] + b)] = byte_of((size_t)x.folder, x.folder_off + b);
    }
    CHECK(got == want);
}

// ---- windows: every window of an entry with bytes marks its bytes in a destination of `cap` bytes
static void windows_case(std::mt19937_64 &rnd)
{
    const Archive a = make_archive(rnd);
    const uint64_t cap = rnd() % 120;
    const size_t n = rnd() % 6;
    std::vector<xlz_7z_want> w(n);
    bool index_ok = true;
    for (size_t i = 0; i < n; i++) {
        const unsigned kind = (unsigned)(rnd() % 8);
        w[i].entry = kind == 0 ? a.e.size() + rnd() % 2 : kind == 1 ? kTop : rnd() % a.e.size();
        w[i].dst_off = kind == 2 ? kTop - rnd() % 4 : kind == 3 ? cap : rnd() % (cap + 3);
        w[i].dst_cap = kind == 4 ? 0 : kind == 5 ? kTop - rnd() % 4 : rnd() % (cap + 3);
        if (kind == 6 && i) w[i] = w[rnd() % i];
        index_ok = index_ok && w[i].entry < a.e.size();
    }
    bool ok = index_ok;
    std::vector<uint8_t> hits((size_t)cap, 0);
    for (size_t i = 0; i < n && index_ok; i++) {
        const xlz_7z_entry &x = a.e[(size_t)w[i].entry];
        if (!((x.flags & XLZ_7Z_ENTRY_HAS_STREAM) && x.size)) continue; // declares nothing
        for (uint64_t j = 0; j < w[i].dst_cap && ok; j++) {
            const unsigned __int128 at = (unsigned __int128)w[i].dst_off + j;
            if (at >= cap || hits[(size_t)at]++) ok = false;
            if (j > 400) ok = false; // (longer than any destination here)
        }
    }
    CHECK(wants_ok(a.e.data(), a.e.size(), w.data(), n, cap) == ok);
}

// ---- layout: against 128-bit sums
static void layout_case(std::mt19937_64 &rnd)
{
    const size_t n = rnd() % 6;
    std::vector<xlz_7z_entry> e(n);
    std::vector<xlz_7z_want> w(n);
    const bool huge = rnd() % 3 == 0;
    for (size_t i = 0; i < n; i++) {
        memset(&e[i], 0, sizeof e[i]);
        e[i].size = huge && rnd() % 2 ? kTop - rnd() % 100 : rnd() % 100;
        w[i].entry = i, w[i].dst_off = w[i].dst_cap = 12345;
    }
    const uint64_t align = rnd() % 4 == 0 ? 1 : 1 + rnd() % 64;
    unsigned __int128 at = 0;
    bool fits = true;
    std::vector<uint64_t> off(n);
    for (size_t i = 0; i < n; i++) {
        at = (at + align - 1) / align * align;
        if (at > kTop) fits = false;
        off[i] = (uint64_t)at;
        at += e[i].size;
        if (at > kTop) fits = false;
    }
    uint64_t total = 777;
    const bool got = layout(e.data(), w.data(), n, align, &total);
    CHECK(got == fits);
    if (got && fits) {
        CHECK(total == (uint64_t)at);
        for (size_t i = 0; i < n; i++) CHECK(w[i].dst_off == off[i] && w[i].dst_cap == e[i].size && w[i].dst_off % align == 0);
    }
}

// ---- what a stream must end in, and the verdict: every combination
static void verdict_cases()
{
    const int32_t statuses[] = {XLZ_OK, XLZ_OK_INPUT_EOF, XLZ_ERR_RESULT, XLZ_ERR_UNEXPECTED_EOF, XLZ_ERR_OUT_CAP, XLZ_ERR_RC_INIT};
    const Cut cuts[] = {{100, 40, kWhole}, {60, 40, kCapCut}, {60, 25, kUnitCut}};
    for (const Cut &c : cuts)
        for (int32_t st : statuses)
            for (int dout = -1; dout <= 1; dout++)
                for (int din = -1; din <= 1; din++) {
                    const uint64_t out_len = c.decode_len + dout, in_used = c.in_len + din;
                    const int32_t got = stream_status(c, st, out_len, in_used);
                    bool good;
                    if (c.kind == kWhole)
                        good = st >= 0 && dout == 0;
                    else if (c.kind == kCapCut)
                        good = st == XLZ_ERR_OUT_CAP && dout == 0;
                    else
                        good = st == XLZ_ERR_UNEXPECTED_EOF && dout == 0 && din == 0;
                    CHECK((got == XLZ_OK) == good);
                    if (!good) {
                        CHECK(got < 0);
                        const bool own = st < 0 && st != expected_status(c.kind); // its own status, but the one that would have been good
                        CHECK(got == (own ? st : (int32_t)XLZ_ERR_RESULT));
                    }
                    CHECK(expected_status(c.kind) == (c.kind == kWhole ? XLZ_OK : c.kind == kCapCut ? XLZ_ERR_OUT_CAP : XLZ_ERR_UNEXPECTED_EOF));
                }
    const int32_t pres[] = {XLZ_OK, XLZ_ERR_OUT_CAP, XLZ_ERR_UNSUPPORTED};
    const int32_t folder_sts[] = {XLZ_OK, XLZ_ERR_RESULT, XLZ_ERR_UNEXPECTED_EOF, XLZ_ERR_RC_INIT};
    for (int32_t pre : pres)
        for (int32_t fst : folder_sts)
            for (uint8_t dg : {kDigestGood, kDigestBad, kDigestNone})
                for (int verify = 0; verify < 2; verify++)
                    for (int has_crc = 0; has_crc < 2; has_crc++)
                        for (int kind = 0; kind < 3; kind++) { // bytes, a stream of no bytes, no stream
                            xlz_7z_entry x;
                            memset(&x, 0, sizeof x);
                            x.flags = (kind < 2 ? XLZ_7Z_ENTRY_HAS_STREAM : 0) | (has_crc ? XLZ_7Z_ENTRY_HAS_CRC : 0);
                            x.size = kind == 0 ? 17 : 0;
                            const xlz_7z_file_result r = verdict(pre, x, fst, dg, verify != 0);
                            xlz_7z_file_result want = {XLZ_OK, 0, 0};
                            if (pre < 0)
                                want.status = pre;
                            else if (kind != 0)
                                want.status = XLZ_OK;
                            else if (fst < 0)
                                want.status = fst;
                            else if (verify && dg == kDigestBad)
                                want.status = XLZ_ERR_RESULT;
                            else
                                want.out_len = 17, want.unverified = verify && !has_crc;
                            CHECK(r.status == want.status && r.out_len == want.out_len && r.unverified == want.unverified);
                        }
}

// ---- FilesInfo: names and the refusals that need no archive around them
static std::vector<uint8_t> names_prop(const std::vector<uint16_t> &units)
{
    std::vector<uint8_t> p = {kNames, (uint8_t)(1 + 2 * units.size()), 0};
    for (uint16_t u : units) p.push_back((uint8_t)u), p.push_back((uint8_t)(u >> 8));
    return p;
}
static void files_cases()
{
    {
        // "a", U+00E9, U+4E2D, U+1F600 as a pair, a lone high surrogate, a lone low one, a high one at the very end
        std::vector<uint8_t> s = {3};
        const std::vector<uint8_t> n = names_prop({'a', 0xE9, 0, 0x4E2D, 0xD83D, 0xDE00, 0, 0xD800, 'x', 0xDC00, 0xD800, 0});
        s.insert(s.end(), n.begin(), n.end());
        s.push_back(0);
        Files f;
        size_t used = 0;
        CHECK(parse_files(s.data(), s.size(), f, &used) == XLZ_OK && used == s.size());
        const std::string pool(f.names.begin(), f.names.end());
        const std::string want = std::string("a\xC3\xA9") + '\0' + "\xE4\xB8\xAD\xF0\x9F\x98\x80" + '\0' + "\xEF\xBF\xBDx\xEF\xBF\xBD\xEF\xBF\xBD" + '\0';
        CHECK(pool == want && f.name_off.size() == 3 && f.name_off[1] == 4 && f.name_len[1] == 7 && f.name_len[2] == 10);
    }
    auto status = [](std::vector<uint8_t> s) {
        Files f;
        size_t used = 0;
        return parse_files(s.data(), s.size(), f, &used);
    };
    CHECK(status({2, kNames, 5, 0, 'a', 0, 0, 0, 0}) == XLZ_ERR_RESULT);           // one name, two entries
    CHECK(status({1, kNames, 7, 0, 'a', 0, 0, 0, 'b', 0, 0}) == XLZ_ERR_RESULT);   // two names (the second unterminated), one entry
    CHECK(status({1, kNames, 3, 0, 'a', 0, 0}) == XLZ_ERR_RESULT);                 // unterminated
    CHECK(status({1, kNames, 4, 0, 'a', 0, 0, 0}) == XLZ_ERR_RESULT);              // an odd pool
    CHECK(status({1, kNames, 5, 1, 'a', 0, 0, 0, 0}) == XLZ_ERR_UNSUPPORTED);      // External
    CHECK(status({1, kNames, 5, 0, 'a', 0, 0, 0, 0}) == XLZ_OK);
    CHECK(status({9, kEmptyStream, 2, 0x80, 0x80, 0}) == XLZ_OK);
    CHECK(status({9, kEmptyStream, 3, 0x80, 0x80, 0, 0}) == XLZ_ERR_RESULT);       // does not fill its size
    CHECK(status({9, kEmptyStream, 1, 0x80, 0}) == XLZ_ERR_RESULT);                // overruns its size
    CHECK(status({1, kMTime, 10, 1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 0}) == XLZ_OK);
    CHECK(status({1, kMTime, 10, 1, 1, 1, 2, 3, 4, 5, 6, 7, 8, 0}) == XLZ_ERR_UNSUPPORTED);
    CHECK(status({1, kMTime, 9, 1, 0, 1, 2, 3, 4, 5, 6, 7, 0}) == XLZ_ERR_RESULT);
    CHECK(status({2, kWinAttributes, 7, 0, 0x40, 0, 1, 2, 3, 4, 0}) == XLZ_OK);    // the second of two defined
    CHECK(status({2, kWinAttributes, 11, 0, 0x40, 0, 1, 2, 3, 4, 5, 6, 7, 8, 0}) == XLZ_ERR_RESULT);
    CHECK(status({1, 0x19, 3, 0, 0, 0, 0x77, 1, 9, 0}) == XLZ_OK);                 // dummy and unknown: skipped
    CHECK(status({1, 0x19, 9, 0, 0, 0}) == XLZ_ERR_RESULT);                        // a size the span does not hold
    CHECK(status({1, kNames}) == XLZ_ERR_RESULT && status({1}) == XLZ_ERR_RESULT && status({}) == XLZ_ERR_RESULT);
    CHECK(status({0xE1, 0, 0, 1, 0}) == XLZ_ERR_UNSUPPORTED);                       // more entries than kMaxItems
}

int main()
{
    std::mt19937_64 rnd(20261019);
    for (int i = 0; i < 20000; i++) plan_case(rnd);
    for (int i = 0; i < 20000; i++) windows_case(rnd);
    for (int i = 0; i < 20000; i++) layout_case(rnd);
    verdict_cases();
    files_cases();
    // the unit-boundary rule on tables made by hand: three units of 10, 0 and 20 bytes, then one of 5
    {
        xlz_lzma2_unit u[4] = {{0, 4, 0, 10, 0, 0}, {4, 1, 10, 0, 0, 0}, {5, 6, 10, 20, 1, 0}, {11, 3, 30, 5, 1, 0}};
        auto cut = [&](uint64_t P) { return cut_folder(XLZ_7Z_LZMA2, false, 35, 15, u, 4, P); };
        CHECK(cut(1).kind == kUnitCut && cut(1).decode_len == 10 && cut(1).in_len == 4);
        CHECK(cut(10).kind == kUnitCut && cut(10).decode_len == 10 && cut(10).in_len == 4);
        CHECK(cut(11).kind == kUnitCut && cut(11).decode_len == 30 && cut(11).in_len == 11);
        CHECK(cut(30).decode_len == 30 && cut(31).kind == kWhole && cut(35).kind == kWhole && cut(35).in_len == 15);
        CHECK(cut_folder(XLZ_7Z_LZMA2, true, 35, 15, u, 4, 1).kind == kWhole);   // a chain is never cut
        CHECK(cut_folder(XLZ_7Z_LZMA2, false, 35, 15, u, 1, 7).kind == kCapCut); // one unit: by capacity
        CHECK(cut_folder(XLZ_7Z_LZMA2, false, 35, 15, u, 0, 7).kind == kWhole);  // no table: whole
        CHECK(cut_folder(XLZ_7Z_LZMA, false, 35, 15, nullptr, 0, 7).decode_len == 7);
        CHECK(cut_folder(XLZ_7Z_COPY, false, 35, 35, nullptr, 0, 7).kind == kWhole && cut_folder(XLZ_7Z_BCJ2, false, 35, 15, nullptr, 0, 7).kind == kWhole);
    }
    if (fails) {
        printf("FAILED: %d checks\n", fails);
        return 1;
    }
    printf("ok\n");
    return 0;
}
