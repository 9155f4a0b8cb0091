// zip_selftest.cpp -- lzma_amd/csrc/xlz_zip.h without a GPU and without the library, against brute-force models: where the
// end record is (every comment length that matters, bytes behind the comment, decoys inside the comment), the ZIP64 end
// record and the ZIP64 extra field, the shift of an archive with bytes in front of it, the windows and their layout, the
// plan and the verdicts.  The archives are written here, record by record, from APPNOTE.TXT.
//   g++ -std=c++17 -O2 -I lzma_amd/csrc tests/c/zip_selftest.cpp -o t && ./t
#include <cstdio>
#include <cstdlib>
#include <string>

#include "xlz_zip.h"

using namespace xlzzip;

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_seed ^= g_seed << 13, g_seed ^= g_seed >> 7, g_seed ^= g_seed << 17;
    return (uint32_t)(g_seed >> 11);
}
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);       \
            exit(1);                                                  \
        }                                                             \
    } while (0)

typedef std::vector<uint8_t> Bytes;
static void p16(Bytes &b, uint32_t v) { b.push_back((uint8_t)v), b.push_back((uint8_t)(v >> 8)); }
static void p32(Bytes &b, uint32_t v) { p16(b, v & 0xFFFF), p16(b, v >> 16); }
static void p64(Bytes &b, uint64_t v) { p32(b, (uint32_t)v), p32(b, (uint32_t)(v >> 32)); }
static void put(Bytes &b, const Bytes &x) { b.insert(b.end(), x.begin(), x.end()); }

struct Member {
    std::string name;
    uint16_t method, flags;
    Bytes payload;
    uint64_t size;
    uint32_t crc;
    bool zip64;
    size_t local_extra; // bytes of an unknown extra field in the LOCAL header only
};
struct Written {
    Bytes file;
    std::vector<uint64_t> header_off, data_off; // with the bytes in front
};

static Written write_zip(const std::vector<Member> &ms, size_t prepend, bool end64, size_t comment, size_t trailing)
{
    Written w;
    Bytes &f = w.file;
    f.assign(prepend, 0x90);
    Bytes cd;
    for (const Member &m : ms) {
        const uint64_t off = f.size() - prepend;
        w.header_off.push_back(f.size());
        Bytes lx, cx;
        if (m.zip64) {
            p16(lx, 1), p16(lx, 16), p64(lx, m.size), p64(lx, m.payload.size());
            p16(cx, 0x7075), p16(cx, 3), cx.push_back(1), cx.push_back(2), cx.push_back(3); // (another field in front)
            p16(cx, 1), p16(cx, 24), p64(cx, m.size), p64(cx, m.payload.size()), p64(cx, off);
        }
        if (m.local_extra) p16(lx, 0x6375), p16(lx, (uint32_t)m.local_extra), lx.insert(lx.end(), m.local_extra, 0);
        const uint32_t s32 = m.zip64 ? 0xFFFFFFFFu : (uint32_t)m.size, c32 = m.zip64 ? 0xFFFFFFFFu : (uint32_t)m.payload.size();
        p32(f, kSigLocal), p16(f, 45), p16(f, m.flags), p16(f, m.method), p16(f, 0x6000), p16(f, 0x5821);
        p32(f, m.crc), p32(f, c32), p32(f, s32), p16(f, (uint32_t)m.name.size()), p16(f, (uint32_t)lx.size());
        f.insert(f.end(), m.name.begin(), m.name.end()), put(f, lx);
        w.data_off.push_back(f.size());
        put(f, m.payload);
        p32(cd, kSigCentral), p16(cd, 63), p16(cd, 45), p16(cd, m.flags), p16(cd, m.method), p16(cd, 0x6000), p16(cd, 0x5821);
        p32(cd, m.crc), p32(cd, c32), p32(cd, s32), p16(cd, (uint32_t)m.name.size()), p16(cd, (uint32_t)cx.size()), p16(cd, 2);
        p16(cd, 0), p16(cd, 0), p32(cd, 0x81A40000u), p32(cd, m.zip64 ? 0xFFFFFFFFu : (uint32_t)off);
        cd.insert(cd.end(), m.name.begin(), m.name.end()), put(cd, cx), cd.push_back('h'), cd.push_back('i'); // (an entry comment)
    }
    const uint64_t cd_off = f.size() - prepend;
    put(f, cd);
    if (end64) {
        const uint64_t at = f.size() - prepend;
        p32(f, kSigEnd64), p64(f, 44), p16(f, 45), p16(f, 45), p32(f, 0), p32(f, 0), p64(f, ms.size()), p64(f, ms.size()), p64(f, cd.size()), p64(f, cd_off);
        p32(f, kSigLocator), p32(f, 0), p64(f, at), p32(f, 1);
        p32(f, kSigEnd), p16(f, 0xFFFF), p16(f, 0xFFFF), p16(f, 0xFFFF), p16(f, 0xFFFF), p32(f, 0xFFFFFFFFu), p32(f, 0xFFFFFFFFu);
    } else {
        p32(f, kSigEnd), p16(f, 0), p16(f, 0), p16(f, (uint32_t)ms.size()), p16(f, (uint32_t)ms.size()), p32(f, (uint32_t)cd.size()), p32(f, (uint32_t)cd_off);
    }
    p16(f, (uint32_t)comment);
    for (size_t k = 0; k < comment; k++) f.push_back((uint8_t)('a' + k % 26));
    f.insert(f.end(), trailing, 0);
    return w;
}

static Bytes lzma_payload(size_t stream, uint8_t props = 0x5D, uint16_t prop_size = 5)
{
    Bytes p;
    p.push_back(9), p.push_back(20), p16(p, prop_size), p.push_back(props), p32(p, 1u << 16);
    for (size_t k = 0; k < stream; k++) p.push_back((uint8_t)rnd());
    return p;
}

static std::vector<Member> members()
{
    std::vector<Member> ms;
    ms.push_back({"dir/", 0, 0, {}, 0, 0, false, 0});
    ms.push_back({"dir/a.txt", 14, 2, lzma_payload(40), 100, 0x11111111u, false, 7});
    ms.push_back({"b", 0, 0, Bytes(33, 'b'), 33, 0x22222222u, true, 0});
    ms.push_back({"c-no-marker", 14, 0, lzma_payload(12), 57, 0x33333333u, true, 3});
    ms.push_back({"deflated", 8, 0, Bytes(10, 1), 50, 1, false, 0});
    ms.push_back({"encrypted", 14, 3, lzma_payload(20), 60, 2, false, 0});
    ms.push_back({"empty-lzma", 14, 2, lzma_payload(10), 0, 0, false, 0});
    ms.push_back({"props225", 14, 2, lzma_payload(10, 225), 9, 3, false, 0});
    ms.push_back({"propsize4", 14, 2, lzma_payload(10, 0x5D, 4), 9, 4, false, 0});
    ms.push_back({"stored-sizes-differ", 0, 0, Bytes(5, 's'), 6, 5, false, 0});
    return ms;
}

// ---- the end record: the model scans forward and keeps the last acceptable position
static void test_find_end()
{
    for (int round = 0; round < 3000; round++) {
        const size_t comment = rnd() % 4 == 0 ? 65535 - rnd() % 3 : rnd() % 70, trailing = rnd() % 3 ? 0 : rnd() % 40;
        Written w = write_zip({members()[2]}, rnd() % 50, rnd() % 2, comment, trailing);
        Bytes &f = w.file;
        for (int d = rnd() % 3; d > 0 && comment >= 22; d--) { // decoys inside the comment: signatures with any comment length
            const size_t at = f.size() - trailing - comment + rnd() % (comment - 21);
            f[at] = 'P', f[at + 1] = 'K', f[at + 2] = 5, f[at + 3] = 6;
            if (rnd() % 2) f[at + 20] = (uint8_t)rnd(), f[at + 21] = (uint8_t)(rnd() % 2);
        }
        if (rnd() % 8 == 0) f.resize(f.size() - rnd() % std::min<size_t>(f.size(), 30)); // cut
        size_t model = ~(size_t)0;
        for (size_t p = 0; p + 22 <= f.size(); p++)
            if (f.size() - p <= kEndSearch && le32(&f[p]) == kSigEnd && p + 22 + le16(&f[p + 20]) <= f.size()) model = p;
        size_t got = ~(size_t)0;
        const bool found = find_end(f.data(), f.size(), &got);
        CHECK(found == (model != ~(size_t)0));
        if (found) CHECK(got == model);
    }
    size_t pos;
    CHECK(!find_end(nullptr, 0, &pos));
    // an end record further than 65 557 bytes from the end is not looked for
    Written w = write_zip({members()[2]}, 0, false, 0, 65536);
    CHECK(!find_end(w.file.data(), w.file.size(), &pos));
    w = write_zip({members()[2]}, 0, false, 0, 65535);
    CHECK(find_end(w.file.data(), w.file.size(), &pos));
}

// ---- the table: ZIP64 fields, the shift, the classes
static void test_table()
{
    const std::vector<Member> ms = members();
    for (size_t prepend : {(size_t)0, (size_t)1, (size_t)1000, (size_t)70000})
        for (int end64 = 0; end64 < 2; end64++) {
            const Written w = write_zip(ms, prepend, end64 != 0, 5, 3);
            Table t;
            CHECK(parse(w.file.data(), w.file.size(), t) == XLZ_OK);
            CHECK(t.end.shift == prepend && t.end.zip64 == (end64 != 0) && t.entries.size() == ms.size());
            uint64_t total = 0;
            for (size_t i = 0; i < ms.size(); i++) {
                const xlz_zip_entry &x = t.entries[i];
                const Member &m = ms[i];
                CHECK(x.size == m.size && x.comp_size == m.payload.size() && x.crc == m.crc && x.method == m.method && x.gp_flags == m.flags);
                CHECK(x.header_off == w.header_off[i] && x.data_off == w.data_off[i]);
                CHECK(x.name_len == m.name.size() && std::string(&t.names[x.name_off]) == m.name);
                CHECK(!!(x.flags & XLZ_ZIP_ENTRY_ZIP64) == m.zip64 && x.external_attr == 0x81A40000u && x.dos_time_date == 0x58216000u);
                CHECK(!!(x.flags & XLZ_ZIP_ENTRY_IS_DIR) == (m.name.back() == '/'));
                CHECK(!!(x.flags & XLZ_ZIP_ENTRY_END_MARKER) == (m.method == 14 && (m.flags & 2)));
                if (has_bytes(x)) total += x.size;
            }
            CHECK(t.total_size == total);
            auto cls = [&](const char *name) {
                for (size_t i = 0; i < ms.size(); i++)
                    if (ms[i].name == name) return t.entries[i].flags & (XLZ_ZIP_ENTRY_SUPPORTED | XLZ_ZIP_ENTRY_BAD);
                CHECK(false);
                return 0u;
            };
            for (const char *n : {"dir/", "dir/a.txt", "b", "c-no-marker", "empty-lzma"}) CHECK(cls(n) == XLZ_ZIP_ENTRY_SUPPORTED);
            for (const char *n : {"deflated", "encrypted", "stored-sizes-differ"}) CHECK(cls(n) == 0);
            for (const char *n : {"props225", "propsize4"}) CHECK(cls(n) == XLZ_ZIP_ENTRY_BAD);
            CHECK(t.entries[1].props == 0x5D && t.entries[1].dict_size == (1u << 16));
        }
    // a ZIP64 extra field that is too short for the values it must hold: that entry is bad, open is not
    Written w = write_zip(ms, 0, false, 0, 0);
    const uint8_t needle[4] = {1, 0, 24, 0};
    auto it = std::search(w.file.begin() + (long)w.data_off.back(), w.file.end(), needle, needle + 4);
    CHECK(it != w.file.end());
    it[2] = 16, it[20] = 0x75, it[21] = 0x70, it[22] = 4, it[23] = 0; // (the last 8 bytes become a field of their own)
    Table t;
    CHECK(parse(w.file.data(), w.file.size(), t) == XLZ_OK);
    CHECK((t.entries[2].flags & XLZ_ZIP_ENTRY_BAD) && t.entries[2].data_off == 0 && !(t.entries[3].flags & XLZ_ZIP_ENTRY_BAD));
}

// ---- windows and layout
static void test_windows()
{
    const Written w = write_zip(members(), 0, false, 0, 0);
    Table t;
    CHECK(parse(w.file.data(), w.file.size(), t) == XLZ_OK);
    const xlz_zip_entry *e = t.entries.data();
    const size_t ne = t.entries.size();
    for (int round = 0; round < 20000; round++) {
        const size_t n = rnd() % 5;
        const uint64_t out_cap = rnd() % 300;
        std::vector<xlz_zip_want> ws(n);
        for (auto &x : ws) x = {rnd() % (ne + (rnd() % 16 == 0)), rnd() % 8 == 0 ? ~(uint64_t)0 - rnd() % 3 : rnd() % 320, rnd() % 120};
        bool model = true;
        std::vector<int> used(300, 0);
        for (const auto &x : ws) {
            if (x.entry >= ne) {
                model = false;
                break;
            }
            if (!has_bytes(e[x.entry]) || !x.dst_cap) continue;
            if (x.dst_off > out_cap || x.dst_cap > out_cap - x.dst_off) {
                model = false;
                break;
            }
            for (uint64_t b = x.dst_off; b < x.dst_off + x.dst_cap; b++)
                if (used[b]++) model = false;
        }
        CHECK(wants_ok(e, ne, ws.data(), n, out_cap) == model);
    }
    for (uint64_t align : {(uint64_t)1, (uint64_t)7, (uint64_t)16, (uint64_t)256}) {
        std::vector<xlz_zip_want> ws;
        for (size_t i = 0; i < ne; i++) ws.push_back({(i * 7) % ne, 99, 99});
        uint64_t total = 0, at = 0;
        CHECK(layout(e, ws.data(), ws.size(), align, &total));
        for (const auto &x : ws) {
            while (at % align) at++;
            CHECK(x.dst_off == at && x.dst_cap == (has_bytes(e[x.entry]) ? e[x.entry].size : 0));
            at += x.dst_cap;
        }
        CHECK(total == at);
    }
    xlz_zip_want two[2] = {{1, 0, 0}, {2, 0, 0}};
    uint64_t total;
    CHECK(layout(e, two, 2, 1ull << 63, &total) && total == (1ull << 63) + 33);
    xlz_zip_want three[3] = {{1, 0, 0}, {2, 0, 0}, {3, 0, 0}};
    CHECK(!layout(e, three, 3, 1ull << 63, &total)); // the third window would begin at 2^64
}

// ---- the plan and the verdicts
static void test_plan()
{
    const std::vector<Member> ms = members();
    const Written w = write_zip(ms, 11, true, 0, 0);
    Table t;
    CHECK(parse(w.file.data(), w.file.size(), t) == XLZ_OK);
    const xlz_zip_entry *e = t.entries.data();
    for (int round = 0; round < 5000; round++) {
        const size_t n = rnd() % 12;
        std::vector<xlz_zip_want> ws(n);
        std::vector<uint64_t> dst(n);
        for (size_t i = 0; i < n; i++) {
            const uint64_t en = rnd() % ms.size();
            ws[i] = {en, 1000 * i, rnd() % 4 == 0 ? e[en].size - (e[en].size ? 1 : 0) : e[en].size + rnd() % 3};
            dst[i] = ws[i].dst_off;
        }
        Plan p;
        plan(w.file.data(), e, ws.data(), dst.data(), n, p);
        size_t ks = 0, kp = 0;
        for (size_t i = 0; i < n; i++) {
            const Member &m = ms[ws[i].entry];
            const bool bytes = m.size && m.name.back() != '/';
            const bool unsup = (m.method != 0 && m.method != 14) || (m.flags & 1) || (m.method == 0 && m.size != m.payload.size());
            const bool bad = m.name == "props225" || m.name == "propsize4";
            int32_t model = XLZ_OK;
            if (bytes && ws[i].dst_cap < m.size) model = XLZ_ERR_OUT_CAP;
            else if (bytes && unsup) model = XLZ_ERR_UNSUPPORTED;
            else if (bytes && bad) model = XLZ_ERR_RESULT;
            CHECK(p.pre[i] == model);
            if (!bytes || model != XLZ_OK) continue;
            if (m.method == 0) {
                CHECK(kp < p.spans.size() && p.span_want[kp] == i && p.spans[kp].dst == dst[i] && p.spans[kp].len == m.size);
                CHECK(p.spans[kp].src_off == w.data_off[ws[i].entry]);
                kp++;
            } else {
                CHECK(ks < p.streams.size() && p.stream_want[ks] == i);
                const xlz_stream_desc &d = p.streams[ks];
                CHECK(d.in == w.file.data() + w.data_off[ws[i].entry] + 9 && d.in_len == m.payload.size() - 9 && d.out_cap == m.size);
                CHECK(d.format == XLZ_FMT_LZMA_RAW && d.props == 0x5D && d.dict_size == (1u << 16) && d.out == nullptr);
                CHECK(d.unpack_size == ((m.flags & 2) ? ~(uint64_t)0 : m.size));
                CHECK(p.items[ks].stream == ks && p.items[ks].off == 0 && p.items[ks].len == m.size && p.items[ks].dst_off == dst[i]);
                ks++;
            }
        }
        CHECK(ks == p.streams.size() && kp == p.spans.size());
        std::vector<xlz_check_range> cr;
        std::vector<size_t> range_of;
        check_ranges(p, n, cr, range_of);
        CHECK(cr.size() == ks + kp);
        for (size_t i = 0; i < n; i++) {
            const bool planned = p.pre[i] == XLZ_OK && has_bytes(e[ws[i].entry]);
            CHECK((range_of[i] != kNone) == planned);
            if (!planned) continue;
            const xlz_check_range &c = cr[range_of[i]];
            CHECK(c.kind == XLZ_CHECK_CRC32 && c.len == e[ws[i].entry].size);
            if (e[ws[i].entry].method == 0) CHECK(c.stream == kDestStream && c.off == dst[i]);
            else CHECK(c.stream < ks && p.stream_want[(size_t)c.stream] == i && c.off == 0);
        }
    }
    // the verdicts, in their order
    const xlz_zip_entry &mk = t.entries[1], &nm = t.entries[3], &dir = t.entries[0];
    auto same = [](xlz_zip_file_result r, int32_t st, uint64_t n) { return r.status == st && r.out_len == n && r.reserved == 0; };
    CHECK(same(verdict(XLZ_ERR_OUT_CAP, dir, XLZ_ERR_RESULT, kDigestBad, true), XLZ_OK, 0)); // (an entry without bytes, whatever else)
    CHECK(same(verdict(XLZ_ERR_OUT_CAP, mk, XLZ_ERR_RESULT, kDigestBad, true), XLZ_ERR_OUT_CAP, 0));
    CHECK(same(verdict(XLZ_OK, mk, XLZ_ERR_PROPS, kDigestBad, true), XLZ_ERR_PROPS, 0));
    CHECK(same(verdict(XLZ_OK, mk, XLZ_OK, kDigestBad, true), XLZ_ERR_RESULT, 0));
    CHECK(same(verdict(XLZ_OK, mk, XLZ_OK, kDigestBad, false), XLZ_OK, mk.size));
    CHECK(same(verdict(XLZ_OK, mk, XLZ_OK, kDigestGood, true), XLZ_OK, mk.size));
    CHECK(stream_status(mk, XLZ_OK, mk.size) == XLZ_OK && stream_status(mk, XLZ_OK_INPUT_EOF, mk.size) == XLZ_OK);
    CHECK(stream_status(mk, XLZ_OK, mk.size - 1) == XLZ_ERR_RESULT);
    CHECK(stream_status(mk, XLZ_ERR_OUT_CAP, mk.size) == XLZ_ERR_RESULT); // (an end-marker stream that wanted to go on)
    CHECK(stream_status(nm, XLZ_ERR_OUT_CAP, nm.size) == XLZ_ERR_OUT_CAP);
    CHECK(stream_status(mk, XLZ_ERR_RC_INIT, 0) == XLZ_ERR_RC_INIT);
}

int main()
{
    test_find_end();
    test_table();
    test_windows();
    test_plan();
    printf("ok\n");
    return 0;
}
