// xlz_tar_walk.h -- the member table of a .tar image: the host's walk along the header chain.  Plain C++, no HIP.  ONE
// routine (walk) reads blocks through a Source: for xlz_tar_parse_host that is a pointer into a host image, for
// xlz_tar_scan_device a lookup in the candidate blocks the device gathered -- so the two forms cannot drift apart.  The
// reference has no tar code.  The rules reproduce what Python's tarfile.open(...).getmembers() reports for name,
// linkname, size, type, offset and offset_data (tarfile.py: TarInfo.frombuf, _proc_builtin, _proc_gnulong, _proc_pax,
// _apply_pax_info); where tarfile is lenient about a malformed number or record this walk refuses instead
// (XLZ_ERR_RESULT), it is never more lenient.
//
// The chain.  From block 0: a zero block ends the archive (what follows is ignored); no byte left at a header position is
// a clean end; 1-511 bytes left: XLZ_ERR_UNEXPECTED_EOF; a non-zero block that is no header candidate (xlz_tar_dev.h), or a
// candidate with a field that does not parse: XLZ_ERR_RESULT.  Data follows a header, rounded up to 512, for the types
// '0', '\0', '7' and every unknown letter; '1'-'6' have none whatever their size field says.  A member whose rounded data
// reaches past the image: XLZ_ERR_UNEXPECTED_EOF, and the member is not listed (tarfile lists it and fails at the next).
// In the error cases the table built so far stays; end_status / end_off say what happened at which header.
//
// Numbers (tarfile.nti): octal up to the first NUL, blanks stripped, empty = 0; base-256 behind a first byte 0x80; a
// negative base-256 number (0xFF) for mtime only -- a size with it is XLZ_ERR_RESULT.  mode, uid and gid must fit 32 bits.
// Names: NUL-terminated bytes, never interpreted as paths.  A '\0'-type entry whose name field ends in '/' is a
// directory (and has no data); trailing slashes of a directory's name field go; a non-empty ustar prefix (bytes 345-499)
// is put in front with a '/'.
//
// Meta entries.  'L' / 'K': the name / link name of the next member, their data up to the first NUL (a directory loses
// ONE trailing slash of such a name).  'x' (and Solaris 'X'): pax records "<len> <key>=<value>\n" for the next member;
// 'g': for every following one.  Applied: path (all trailing slashes go), linkpath, size, mtime, uid, gid; a member takes
// the global records first, then its own.  An 'x' size also moves the chain; a 'g' size only changes what is reported
// (tarfile).  Of two meta entries that name the same thing for one member the first wins.  A member's hdr_off is the
// offset of its first 'L' / 'K' / 'x' header (tarfile's offset).  Meta data over 1 MiB, a malformed record or number:
// XLZ_ERR_RESULT.  A meta entry that no member follows: XLZ_ERR_RESULT (zero block) or XLZ_ERR_UNEXPECTED_EOF (the end).
// 'S' (old GNU sparse), 'M' (multi-volume continuation) and any GNU.sparse.* pax key: XLZ_ERR_UNSUPPORTED at that entry.
//
// A Source that does not hold a meta entry's data yet returns nullptr: the walk notes the blocks it wants (Table::wants),
// goes on as if the entry said nothing, and the caller runs it again once it has fetched them.  Everything in front of
// the first missing entry is final, so every run gets at least one entry further.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/xlz.h"

namespace xlztar {

constexpr uint64_t kBlk = 512;
constexpr uint64_t kMaxMeta = 1u << 20;

// the serial form of the classify kernel, one block: 2 all zero, 1 header candidate, 0 anything else
inline uint8_t classify_block(const uint8_t *b)
{
    uint32_t sum = 256, high = 0, any = 0;
    for (uint32_t i = 0; i < kBlk; i++) {
        any |= b[i];
        if (i >= 148 && i < 156) continue;
        sum += b[i], high += b[i] >> 7;
    }
    if (!any) return 2;
    uint32_t i = 148, digits = 0, v = 0;
    while (i < 156 && b[i] == ' ') i++;
    while (i < 156 && b[i] >= '0' && b[i] <= '7') v = v * 8 + (b[i] - '0'), digits++, i++;
    if (digits == 0 || digits > 7) return 0;
    for (; i < 156; i++)
        if (b[i] != 0 && b[i] != ' ') return 0;
    return v == sum || (int64_t)v == (int64_t)sum - 256 * (int64_t)high ? 1 : 0;
}

struct Source {
    virtual int flag(uint64_t blk) = 0;                         // of a complete block of the image
    virtual const uint8_t *header(uint64_t blk) = 0;            // the 512 bytes of a block whose flag is 1
    virtual const uint8_t *meta(uint64_t blk, uint64_t n) = 0;  // n whole blocks from blk on, or nullptr: not fetched yet
    virtual ~Source() {}
};

struct MetaWant {
    uint64_t blk, n;
};

struct Table {
    std::vector<xlz_tar_entry> entries;
    std::string names; // every name and link name, each NUL-terminated
    int end_status = XLZ_OK;
    uint64_t end_off = 0;
    uint64_t header_blocks = 0; // headers the walk reached, meta entries included
    std::vector<MetaWant> wants;
};

// ---- numbers ----
inline bool is_blank(uint8_t c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

// tarfile.nti over s[0 .. n): -> false: no number, or one that does not fit 64 bits.  neg: the 0xFF form.
inline bool number(const uint8_t *s, size_t n, uint64_t &mag, bool &neg)
{
    mag = 0, neg = false;
    if (s[0] == 0x80 || s[0] == 0xFF) {
        neg = s[0] == 0xFF;
        const uint8_t fill = neg ? 0xFF : 0;
        size_t i = 1;
        for (; n - i > 8; i++)
            if (s[i] != fill) return false;
        for (; i < n; i++) mag = mag << 8 | s[i];
        if (neg) {
            if (n - 1 >= 8 && !(mag >> 63)) return false; // below -2^63
            if (n - 1 < 8) mag |= ~(uint64_t)0 << (8 * (n - 1));
            mag = 0 - mag; // the magnitude
        }
        return true;
    }
    size_t a = 0, b = 0;
    while (b < n && s[b]) b++;
    while (a < b && is_blank(s[a])) a++;
    while (b > a && is_blank(s[b - 1])) b--;
    for (; a < b; a++) {
        if (s[a] < '0' || s[a] > '7' || mag >> 61) return false;
        mag = mag << 3 | (uint64_t)(s[a] - '0');
    }
    return true;
}
inline bool number_u32(const uint8_t *s, size_t n, uint32_t &out)
{
    uint64_t mag;
    bool neg;
    if (!number(s, n, mag, neg) || neg || mag > 0xFFFFFFFFull) return false;
    out = (uint32_t)mag;
    return true;
}

inline std::string field_str(const uint8_t *s, size_t n)
{
    size_t k = 0;
    while (k < n && s[k]) k++;
    return std::string(reinterpret_cast<const char *>(s), k);
}
inline void strip_slashes(std::string &s)
{
    while (!s.empty() && s.back() == '/') s.pop_back();
}

// ---- what meta entries say about a member ----
struct Over {
    bool have_name = false, name_is_pax = false, have_link = false, have_size = false, have_mtime = false, have_uid = false, have_gid = false;
    std::string name, link;
    uint64_t size = 0;
    int64_t mtime_s = 0;
    uint32_t mtime_ns = 0, uid = 0, gid = 0;
};

inline bool dec_u64(const uint8_t *p, size_t n, uint64_t &out)
{
    out = 0;
    if (!n) return false;
    for (size_t i = 0; i < n; i++) {
        if (p[i] < '0' || p[i] > '9') return false;
        const uint64_t d = (uint64_t)(p[i] - '0');
        if (out > (~(uint64_t)0 - d) / 10) return false;
        out = out * 10 + d;
    }
    return true;
}
// "[-]digits[.digits]" -> whole seconds (floor) and nanoseconds
inline bool dec_time(const uint8_t *p, size_t n, int64_t &s, uint32_t &ns)
{
    const bool neg = n && p[0] == '-';
    if (neg) p++, n--;
    size_t dot = 0;
    while (dot < n && p[dot] != '.') dot++;
    uint64_t whole;
    if (!dec_u64(p, dot, whole) || whole >> 62) return false;
    uint64_t frac = 0;
    uint32_t fd = 0;
    for (size_t i = dot + 1; i < n; i++) {
        if (p[i] < '0' || p[i] > '9') return false;
        if (fd < 9) frac = frac * 10 + (uint64_t)(p[i] - '0'), fd++;
    }
    if (dot < n && dot + 1 == n) return false; // "12."
    for (; fd < 9; fd++) frac *= 10;
    s = (int64_t)whole, ns = (uint32_t)frac;
    if (neg) {
        s = -s;
        if (ns) s -= 1, ns = 1000000000u - ns;
    }
    return true;
}

// pax records in d[0 .. size) -> XLZ_OK, XLZ_ERR_RESULT (malformed) or XLZ_ERR_UNSUPPORTED (a GNU.sparse.* key); a later
// record of a key replaces an earlier one (tarfile keeps them in a dict)
inline int pax_records(const uint8_t *d, uint64_t size, Over &o)
{
    uint64_t pos = 0;
    while (pos < size && d[pos] != 0) {
        uint64_t p = pos, len = 0;
        while (p < size && d[p] >= '0' && d[p] <= '9') {
            len = len * 10 + (uint64_t)(d[p] - '0');
            if (len > 2 * kMaxMeta) return XLZ_ERR_RESULT;
            p++;
        }
        if (p == pos || p >= size || d[p] != ' ') return XLZ_ERR_RESULT;
        if (len < 5 || len > size - pos) return XLZ_ERR_RESULT;
        const uint64_t last = pos + len - 1, key0 = p + 1;
        if (d[last] != '\n' || key0 >= last) return XLZ_ERR_RESULT;
        uint64_t eq = key0;
        while (eq < last && d[eq] != '=') eq++;
        if (eq == last || eq == key0) return XLZ_ERR_RESULT;
        const std::string key(reinterpret_cast<const char *>(d + key0), (size_t)(eq - key0));
        const uint8_t *v = d + eq + 1;
        const size_t vn = (size_t)(last - eq - 1);
        if (key.compare(0, 11, "GNU.sparse.") == 0) return XLZ_ERR_UNSUPPORTED;
        if (key == "path") {
            o.have_name = o.name_is_pax = true, o.name.assign(reinterpret_cast<const char *>(v), vn);
        } else if (key == "linkpath") {
            o.have_link = true, o.link.assign(reinterpret_cast<const char *>(v), vn);
        } else if (key == "size") {
            if (!dec_u64(v, vn, o.size)) return XLZ_ERR_RESULT;
            o.have_size = true;
        } else if (key == "uid" || key == "gid") {
            uint64_t x;
            if (!dec_u64(v, vn, x) || x > 0xFFFFFFFFull) return XLZ_ERR_RESULT;
            if (key == "uid") o.have_uid = true, o.uid = (uint32_t)x;
            else o.have_gid = true, o.gid = (uint32_t)x;
        } else if (key == "mtime") {
            if (!dec_time(v, vn, o.mtime_s, o.mtime_ns)) return XLZ_ERR_RESULT;
            o.have_mtime = true;
        }
        pos += len;
    }
    return XLZ_OK;
}

// what `from` says goes into `to`: replace -- the global records, a later header replaces an earlier one; else the
// first entry that names a thing for a member keeps it
inline void merge(Over &to, const Over &from, bool replace)
{
    if (from.have_name && (replace || !to.have_name)) to.have_name = true, to.name_is_pax = from.name_is_pax, to.name = from.name;
    if (from.have_link && (replace || !to.have_link)) to.have_link = true, to.link = from.link;
    if (from.have_size && (replace || !to.have_size)) to.have_size = true, to.size = from.size;
    if (from.have_mtime && (replace || !to.have_mtime)) to.have_mtime = true, to.mtime_s = from.mtime_s, to.mtime_ns = from.mtime_ns;
    if (from.have_uid && (replace || !to.have_uid)) to.have_uid = true, to.uid = from.uid;
    if (from.have_gid && (replace || !to.have_gid)) to.have_gid = true, to.gid = from.gid;
}

struct Member {
    std::string name, link;
    uint64_t size = 0;
    int64_t mtime_s = 0;
    uint32_t mtime_ns = 0, mode = 0, uid = 0, gid = 0;
    uint8_t type = 0;
};
inline void apply(Member &m, const Over &o, bool is_dir)
{
    if (o.have_name) {
        m.name = o.name;
        if (o.name_is_pax) strip_slashes(m.name);
        else if (is_dir && !m.name.empty() && m.name.back() == '/') m.name.pop_back();
    }
    if (o.have_link) m.link = o.link;
    if (o.have_size) m.size = o.size;
    if (o.have_mtime) m.mtime_s = o.mtime_s, m.mtime_ns = o.mtime_ns;
    if (o.have_uid) m.uid = o.uid;
    if (o.have_gid) m.gid = o.gid;
}

inline void walk(Source &src, uint64_t len, Table &t)
{
    t = Table();
    Over global, pending;
    bool after_meta = false, have_first = false;
    uint64_t first_off = 0, off = 0;
    auto end = [&](int st, uint64_t at) { t.end_status = st, t.end_off = at; };
    for (;;) {
        if (len - off < kBlk) return end(len == off ? (after_meta ? XLZ_ERR_UNEXPECTED_EOF : XLZ_OK) : XLZ_ERR_UNEXPECTED_EOF, off);
        const uint64_t blk = off / kBlk;
        const int f = src.flag(blk);
        if (f == 2) return end(after_meta ? XLZ_ERR_RESULT : XLZ_OK, off);
        if (f != 1) return end(XLZ_ERR_RESULT, off);
        const uint8_t *h = src.header(blk);
        if (!h) return end(XLZ_ERR_RESULT, off);
        t.header_blocks++;
        Member m;
        uint64_t mag;
        bool neg;
        if (!number(h + 124, 12, m.size, neg) || neg) return end(XLZ_ERR_RESULT, off);
        if (!number_u32(h + 100, 8, m.mode) || !number_u32(h + 108, 8, m.uid) || !number_u32(h + 116, 8, m.gid)) return end(XLZ_ERR_RESULT, off);
        if (!number(h + 136, 12, mag, neg) || (!neg && mag >> 63)) return end(XLZ_ERR_RESULT, off);
        m.mtime_s = neg ? (int64_t)(0 - mag) : (int64_t)mag;
        m.type = h[156];
        const uint64_t data_off = off + kBlk; // (off + 512 <= len)
        if (m.type == 'S' || m.type == 'M') return end(XLZ_ERR_UNSUPPORTED, off);
        if (m.type == 'L' || m.type == 'K' || m.type == 'x' || m.type == 'X' || m.type == 'g') {
            if (m.size > kMaxMeta) return end(XLZ_ERR_RESULT, off);
            const uint64_t padded = (m.size + kBlk - 1) / kBlk * kBlk;
            if (padded > len - data_off) return end(XLZ_ERR_UNEXPECTED_EOF, off);
            if (m.type != 'g' && !have_first) have_first = true, first_off = off;
            const uint8_t *d = padded ? src.meta(data_off / kBlk, padded / kBlk) : h;
            if (!d) {
                t.wants.push_back(MetaWant{data_off / kBlk, padded / kBlk});
            } else if (m.type == 'L' || m.type == 'K') {
                Over o;
                if (m.type == 'L') o.have_name = true, o.name = field_str(d, (size_t)m.size);
                else o.have_link = true, o.link = field_str(d, (size_t)m.size);
                merge(pending, o, false);
            } else {
                Over o;
                const int st = pax_records(d, m.size, o);
                if (st != XLZ_OK) return end(st, off);
                if (m.type == 'g') merge(global, o, true);
                else merge(pending, o, false);
            }
            after_meta = true;
            off = data_off + padded;
            continue;
        }
        m.name = field_str(h, 100);
        m.link = field_str(h + 157, 100);
        if (m.type == 0 && !m.name.empty() && m.name.back() == '/') m.type = '5';
        const bool is_dir = m.type == '5';
        if (is_dir) strip_slashes(m.name);
        const std::string prefix = field_str(h + 345, 155);
        if (!prefix.empty()) m.name = prefix + "/" + m.name;
        const bool has_data = !(m.type >= '1' && m.type <= '6');
        uint64_t chain = m.size;
        apply(m, global, is_dir);
        if (is_dir) strip_slashes(m.name);
        if (pending.have_size) chain = pending.size;
        apply(m, pending, is_dir);
        uint64_t padded = 0;
        if (has_data) {
            const uint64_t most = chain > m.size ? chain : m.size;
            if (most > len - data_off) return end(XLZ_ERR_UNEXPECTED_EOF, off);
            padded = (chain + kBlk - 1) / kBlk * kBlk; // (chain <= len: no overflow)
            if (padded > len - data_off) return end(XLZ_ERR_UNEXPECTED_EOF, off);
        }
        if (m.name.size() > 0xFFFFFFFFull || m.link.size() > 0xFFFFFFFFull || t.names.size() > 0xFFFFFFFFull - m.name.size() - m.link.size() - 2)
            return end(XLZ_ERR_UNSUPPORTED, off); // (name_off / link_off are 32 bits)
        xlz_tar_entry e;
        memset(&e, 0, sizeof e);
        e.hdr_off = have_first ? first_off : off, e.data_off = data_off, e.size = m.size;
        e.mtime_s = m.mtime_s, e.mtime_ns = m.mtime_ns, e.mode = m.mode, e.uid = m.uid, e.gid = m.gid, e.type = m.type;
        e.name_off = (uint32_t)t.names.size(), e.name_len = (uint32_t)m.name.size();
        t.names.append(m.name), t.names.push_back('\0');
        e.link_off = (uint32_t)t.names.size(), e.link_len = (uint32_t)m.link.size();
        t.names.append(m.link), t.names.push_back('\0');
        t.entries.push_back(e);
        pending = Over(), after_meta = have_first = false;
        off = data_off + padded;
    }
}

// the Source of xlz_tar_parse_host: every block is there
struct HostSource : Source {
    const uint8_t *image;
    explicit HostSource(const uint8_t *p) : image(p) {}
    int flag(uint64_t blk) override { return classify_block(image + blk * kBlk); }
    const uint8_t *header(uint64_t blk) override { return image + blk * kBlk; }
    const uint8_t *meta(uint64_t blk, uint64_t) override { return image + blk * kBlk; }
};

} // namespace xlztar
