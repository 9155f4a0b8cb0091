// xlz_7z.hip -- .7z container front-end: folder list -> batch of raw LZMA / LZMA2 streams.
//
// SURVEY.md section 8(f) rank 3.  The reference's only real plugin API are the two bodgit/sevenzip
// decompressor constructors (reader1.go:28-61 method id 03 01 01, reader2.go:45-75 method id 21):
// a .7z archive stores its data in "folders", each one compressed stream with out-of-band
// properties -- exactly what those constructors take (props byte + LE32 dictionary size +
// unpackSize for LZMA; one dictionary byte for LZMA2).  Folders are independent, so an archive is
// ONE call of the batch engine: folder i = stream i (XLZ_FMT_LZMA_RAW / XLZ_FMT_LZMA2_RAW).
//
// Host-only code (no kernels here).  Format restated from 7-Zip's published 7zFormat.txt; nothing
// of it exists in the reference.  Only what feeds the LZMA paths is implemented: folders with ONE
// coder that is LZMA, LZMA2 or Copy and one packed stream; in filter mode 1 lines of Delta / BCJ filters
// behind one such coder; in bcj2 mode 1 / 2 the two BCJ2 forms (find_bcj2), whose four streams are merged
// on the device (xlz_bcj2_dev.hip).  Other coder graphs, encryption and multi-volume archives are reported
// per folder as unsupported.  The index and decode calls do not
// look at file names and attributes (FilesInfo): their output is the folders' bytes back to back, which is
// the archive's files back to back.  xlz_7z_open (at the end of this file) parses FilesInfo too -- xlz_7z_files.h -- and
// keeps the table; xlz_7z_extract.hip extracts chosen files with it.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/xlz.h"
#include "xlz_7z_files.h"
#include "xlz_check.h"
#include "xlz_check_host.h"

namespace {

enum : uint8_t {
    kEnd = 0x00, kHeader = 0x01, kArchiveProperties = 0x02, kAdditionalStreamsInfo = 0x03, kMainStreamsInfo = 0x04,
    kFilesInfo = 0x05, kPackInfo = 0x06, kUnPackInfo = 0x07, kSubStreamsInfo = 0x08, kSize = 0x09, kCRC = 0x0A,
    kFolder = 0x0B, kCodersUnPackSize = 0x0C, kNumUnPackStream = 0x0D, kEncodedHeader = 0x17
};

const uint8_t kMagic[6] = {'7', 'z', 0xBC, 0xAF, 0x27, 0x1C};
using xlz7zf::kMaxItems; // folders / streams / files we are willing to index

uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
uint64_t le64(const uint8_t *p) { return (uint64_t)le32(p) | (uint64_t)le32(p + 4) << 32; }

using xlz7zf::Rd; // bounded reader over a header

struct Digests {
    std::vector<uint8_t> defined;
    std::vector<uint32_t> crc;
};

bool read_digests(Rd &r, uint64_t count, Digests &d)
{
    if (count > kMaxItems || count > 8 * (uint64_t)r.left()) return false; // >= 1 bit of header per digest
    d.defined.assign((size_t)count, 1);
    d.crc.assign((size_t)count, 0);
    if (r.byte() == 0) { // not all defined: a bit vector, MSB first
        uint8_t b = 0, mask = 0;
        for (uint64_t i = 0; i < count; i++) {
            if (!mask) {
                b = r.byte();
                mask = 0x80;
            }
            d.defined[(size_t)i] = (b & mask) != 0;
            mask >>= 1;
        }
    }
    for (uint64_t i = 0; i < count; i++)
        if (d.defined[(size_t)i]) {
            if (r.n - r.pos < 4) return false;
            d.crc[(size_t)i] = le32(r.p + r.pos);
            r.pos += 4;
        }
    return !r.bad;
}

struct Folder {
    uint32_t method = 0; // XLZ_7Z_*
    uint8_t props = 0;
    uint32_t dict_size = 0;
    uint32_t n_pack = 1;    // packed streams it consumes
    uint32_t n_out = 1;     // output streams of its coder graph
    uint64_t unpack_size = 0;
    bool has_crc = false;
    uint32_t crc = 0;
    uint64_t n_sub = 1;
    // a LINE of 2-4 coders with one input and one output each, one packed stream, an LZMA / LZMA2 coder reading it and
    // Delta / BCJ filters behind it (xlz_7z_index_chains, filter mode 1): the LZMA coder's method and properties, the
    // filters in the order a decoder applies them
    bool chain = false;
    uint32_t chain_method = 0, chain_dict = 0;
    uint8_t chain_props = 0;
    std::vector<std::pair<uint32_t, uint32_t>> steps; // (XLZ_FILTER_*, parameter)
    // one of the two BCJ2 forms (xlz_7z_index_bcj2, bcj2 mode 1 / 2): for main / call / jump the coder that feeds BCJ2's
    // input (XLZ_7Z_LZMA / XLZ_7Z_LZMA2 with its properties and the index of its output stream) or XLZ_7Z_COPY for a packed
    // stream read raw, and which of the folder's packed streams it reads; the packed stream of the range coder; BCJ2's output
    struct Bcj2Sub {
        uint32_t method = 0, dict = 0, pack_k = 0, out_index = 0;
        uint8_t props = 0;
        uint64_t unpack = 0;
    };
    bool bcj2 = false;
    Bcj2Sub bsub[3];
    uint32_t rc_pack_k = 0, bcj2_out_index = 0;
    uint64_t bcj2_final = 0;
};

// the filter a 7z method id names (7-Zip's Methods.txt), or 0
uint32_t filter_of_method(const uint8_t *id, unsigned id_size)
{
    if (id_size == 1 && id[0] == 0x03) return XLZ_FILTER_DELTA;
    if (id_size != 4 || id[0] != 0x03 || id[1] != 0x03) return 0;
    const uint32_t m = (uint32_t)id[2] << 8 | id[3];
    switch (m) {
    case 0x0103: return XLZ_FILTER_X86;
    case 0x0205: return XLZ_FILTER_POWERPC;
    case 0x0401: return XLZ_FILTER_IA64;
    case 0x0501: return XLZ_FILTER_ARM;
    case 0x0701: return XLZ_FILTER_ARMTHUMB;
    case 0x0805: return XLZ_FILTER_SPARC;
    default: return 0;
    }
}

struct Streams {
    uint64_t pack_pos = 0;
    std::vector<uint64_t> pack_sizes;
    std::vector<Folder> folders;
    std::vector<xlz_7z_substream> subs; // in folder order
};

// Is the coder graph one of the two BCJ2 forms?  nodes: the coders in header order (kind 1 LZMA, 2 LZMA2, 50 BCJ2; input
// and output streams are numbered through the coders in that order), binds: (input stream, output stream), packed: the
// input stream every packed stream of the folder feeds.  Four coders: three LZMA / LZMA2 coders feed BCJ2's inputs 0-2;
// two: one feeds input 0, inputs 1 and 2 are packed streams.  Input 3 (the range coder's bytes) is a packed stream.
template <class Node>
void find_bcj2(const std::vector<Node> &nodes, const std::vector<std::pair<uint64_t, uint64_t>> &binds, const std::vector<uint64_t> &packed,
               Folder &f)
{
    const size_t nc = nodes.size();
    if ((nc != 2 && nc != 4) || packed.size() != 4 || binds.size() != nc - 1) return;
    std::vector<uint32_t> in_base(nc), out_base(nc);
    uint32_t ti = 0, to = 0;
    size_t B = nc;
    for (size_t c = 0; c < nc; c++) {
        in_base[c] = ti, out_base[c] = to;
        ti += nodes[c].n_in, to += nodes[c].n_out;
        if (nodes[c].kind == 50) {
            if (B != nc) return;
            B = c;
        } else if (nodes[c].kind != XLZ_7Z_LZMA && nodes[c].kind != XLZ_7Z_LZMA2) {
            return;
        }
    }
    if (B == nc || ti != nc + 3 || to != nc) return;
    std::vector<int> in_from(ti, -1), in_pack(ti, -1), out_used(to, 0);
    for (const auto &bp : binds) {
        if (bp.first >= ti || bp.second >= to || in_from[(size_t)bp.first] >= 0 || out_used[(size_t)bp.second]) return; // (bound twice)
        in_from[(size_t)bp.first] = (int)bp.second, out_used[(size_t)bp.second] = 1;
    }
    for (size_t k = 0; k < 4; k++) {
        if (packed[k] >= ti || in_from[(size_t)packed[k]] >= 0 || in_pack[(size_t)packed[k]] >= 0) return;
        in_pack[(size_t)packed[k]] = (int)k;
    }
    if (out_used[out_base[B]]) return; // BCJ2's output is the folder's
    Folder::Bcj2Sub sub[3];
    for (uint32_t j = 0; j < 3; j++) {
        const uint32_t in = in_base[B] + j;
        if (in_from[in] >= 0) {
            size_t c = 0;
            while (c < nc && out_base[c] != (uint32_t)in_from[in]) c++;
            if (c == nc || c == B || in_pack[in_base[c]] < 0) return;
            sub[j].method = nodes[c].kind, sub[j].props = nodes[c].props, sub[j].dict = nodes[c].dict;
            sub[j].pack_k = (uint32_t)in_pack[in_base[c]], sub[j].out_index = out_base[c];
        } else {
            if (nc == 4 || j == 0) return; // (four coders: all three are fed by coders; two: the main stream is)
            sub[j].method = XLZ_7Z_COPY, sub[j].pack_k = (uint32_t)in_pack[in];
        }
    }
    if (in_pack[in_base[B] + 3] < 0) return; // (the range coder's bytes fed by a coder)
    f.bcj2 = true;
    for (uint32_t j = 0; j < 3; j++) f.bsub[j] = sub[j];
    f.rc_pack_k = (uint32_t)in_pack[in_base[B] + 3], f.bcj2_out_index = out_base[B];
}

// one folder (7zFormat.txt "Folder"): coders, bind pairs, packed stream indices
bool read_folder(Rd &r, Folder &f)
{
    const uint64_t n_coders = r.number();
    if (n_coders == 0 || n_coders > 32) return false;
    uint64_t total_in = 0, total_out = 0;
    uint32_t method = XLZ_7Z_UNSUPPORTED;
    struct Coder {
        uint32_t kind = 0; // XLZ_7Z_LZMA / XLZ_7Z_LZMA2, 100: a filter, 0: anything else
        uint32_t fid = 0, fparam = 0, dict = 0;
        uint8_t props = 0;
    };
    std::vector<Coder> coders;
    struct Node { // every coder, for the BCJ2 forms: 1 LZMA, 2 LZMA2, 50 BCJ2 (4 in, 1 out, no properties), 0 anything else
        uint32_t kind = 0, dict = 0, n_in = 1, n_out = 1;
        uint8_t props = 0;
    };
    std::vector<Node> nodes;
    bool simple = n_coders >= 2 && n_coders <= 4; // every coder one input, one output
    for (uint64_t c = 0; c < n_coders; c++) {
        const uint8_t mb = r.byte();
        if (mb & 0xC0) return false; // reserved / alternative methods
        const unsigned id_size = mb & 0x0F;
        uint8_t id[16] = {0};
        for (unsigned k = 0; k < id_size; k++) id[k] = r.byte();
        uint64_t n_in = 1, n_out = 1;
        if (mb & 0x10) {
            n_in = r.number();
            n_out = r.number();
            // a coder without an input or an output stream does not exist (7-Zip refuses it); with n_in == 0 the
            // folder below would claim zero packed streams and place_folders would index past PackInfo
            if (n_in == 0 || n_out == 0 || n_in > 32 || n_out > 32) return false;
        }
        uint64_t psz = 0;
        size_t ppos = r.pos;
        if (mb & 0x20) {
            psz = r.number();
            ppos = r.pos;
            if (!r.skip(psz)) return false;
        }
        total_in += n_in;
        total_out += n_out;
        {
            Node nd;
            nd.n_in = (uint32_t)n_in, nd.n_out = (uint32_t)n_out;
            if (n_in == 1 && n_out == 1 && id_size == 3 && id[0] == 0x03 && id[1] == 0x01 && id[2] == 0x01 && psz == 5 && !r.bad)
                nd.kind = XLZ_7Z_LZMA, nd.props = r.p[ppos], nd.dict = le32(r.p + ppos + 1);
            else if (n_in == 1 && n_out == 1 && id_size == 1 && id[0] == 0x21 && psz == 1 && !r.bad)
                nd.kind = XLZ_7Z_LZMA2, nd.props = r.p[ppos];
            else if (n_in == 4 && n_out == 1 && id_size == 4 && id[0] == 0x03 && id[1] == 0x03 && id[2] == 0x01 && id[3] == 0x1B && !(mb & 0x20))
                nd.kind = 50;
            nodes.push_back(nd);
        }
        if (n_in != 1 || n_out != 1) simple = false;
        if (simple) {
            Coder cd;
            const uint32_t fid = filter_of_method(id, id_size);
            if (id_size == 3 && id[0] == 0x03 && id[1] == 0x01 && id[2] == 0x01 && psz == 5)
                cd.kind = XLZ_7Z_LZMA, cd.props = r.p[ppos], cd.dict = le32(r.p + ppos + 1);
            else if (id_size == 1 && id[0] == 0x21 && psz == 1)
                cd.kind = XLZ_7Z_LZMA2, cd.props = r.p[ppos];
            else if (fid == XLZ_FILTER_DELTA && psz == 1) // exactly one property byte (distance - 1), as 7-Zip demands
                cd.kind = 100, cd.fid = fid, cd.fparam = (uint32_t)r.p[ppos] + 1;
            else if (fid && fid != XLZ_FILTER_DELTA && psz == 0)
                cd.kind = 100, cd.fid = fid;
            coders.push_back(cd);
        }
        if (n_coders == 1 && n_in == 1 && n_out == 1) {
            if (id_size == 3 && id[0] == 0x03 && id[1] == 0x01 && id[2] == 0x01 && psz == 5) { // LZMA, reader1.go:31
                method = XLZ_7Z_LZMA;
                f.props = r.p[ppos];
                f.dict_size = le32(r.p + ppos + 1);
            } else if (id_size == 1 && id[0] == 0x21 && psz == 1) { // LZMA2, reader2.go:48
                method = XLZ_7Z_LZMA2;
                f.props = r.p[ppos];
            } else if (id_size == 1 && id[0] == 0x00) { // Copy
                method = XLZ_7Z_COPY;
            }
        }
    }
    if (total_out == 0) return false;
    const uint64_t n_bind = total_out - 1;
    if (total_in < n_bind) return false;
    std::vector<std::pair<uint64_t, uint64_t>> binds; // (input stream, the output stream that feeds it)
    std::vector<std::pair<uint64_t, uint64_t>> all_binds;
    std::vector<uint64_t> packed_list; // the input stream each packed stream feeds
    for (uint64_t k = 0; k < n_bind; k++) {
        const uint64_t in_index = r.number(), out_index = r.number();
        if (simple) binds.emplace_back(in_index, out_index);
        all_binds.emplace_back(in_index, out_index);
    }
    const uint64_t n_packed = total_in - n_bind;
    if (n_packed == 0) return false; // every folder consumes at least one packed stream
    if (n_packed > 1)
        for (uint64_t k = 0; k < n_packed; k++) packed_list.push_back(r.number());
    if (!r.bad) find_bcj2(nodes, all_binds, packed_list, f);
    f.method = method;
    f.n_pack = (uint32_t)n_packed;
    f.n_out = (uint32_t)total_out;
    if (simple && n_packed == 1 && !r.bad) {
        // with one stream in and out per coder, stream c is coder c's.  feeds[c] = the coder whose input coder c's output
        // is, fed[c] = coder c's input comes from a coder; the line starts at the one coder that reads the packed stream
        const size_t nc = coders.size();
        std::vector<int> feeds(nc, -1), fed(nc, 0);
        bool ok = true;
        for (const auto &bp : binds) {
            if (bp.first >= nc || bp.second >= nc || fed[(size_t)bp.first] || feeds[(size_t)bp.second] >= 0) ok = false;
            if (!ok) break;
            fed[(size_t)bp.first] = 1, feeds[(size_t)bp.second] = (int)bp.first;
        }
        size_t at = nc;
        for (size_t c = 0; ok && c < nc; c++)
            if (!fed[c]) at = c; // (exactly one: n_packed == 1)
        ok = ok && at < nc && (coders[at].kind == XLZ_7Z_LZMA || coders[at].kind == XLZ_7Z_LZMA2);
        if (ok) {
            f.chain_method = coders[at].kind, f.chain_props = coders[at].props, f.chain_dict = coders[at].dict;
            size_t seen = 1;
            while (ok && feeds[at] >= 0) {
                at = (size_t)feeds[at];
                if (coders[at].kind != 100 || ++seen > nc) ok = false;
                else f.steps.emplace_back(coders[at].fid, coders[at].fparam);
            }
            ok = ok && seen == nc;
        }
        if (!ok) f.steps.clear();
        f.chain = ok;
    }
    return !r.bad;
}

// bcj2: a folder that is one of the BCJ2 forms gets the size of BCJ2's output as its unpack size (bcj2 mode 1 / 2,
// xlz_7z_index_bcj2); otherwise such a folder is read as ever
int read_streams_info(Rd &r, Streams &s, bool bcj2 = false)
{
    uint8_t id = r.byte();
    if (id == kPackInfo) {
        s.pack_pos = r.number();
        const uint64_t n = r.number();
        if (n > kMaxItems) return XLZ_ERR_UNSUPPORTED;
        id = r.byte();
        if (id == kSize) {
            if (n > r.left()) return XLZ_ERR_RESULT; // every size is at least one byte: no allocation the header cannot back
            s.pack_sizes.resize((size_t)n);
            for (auto &v : s.pack_sizes) v = r.number();
            id = r.byte();
        }
        if (id == kCRC) {
            Digests d;
            if (!read_digests(r, n, d)) return XLZ_ERR_RESULT;
            id = r.byte();
        }
        if (id != kEnd || r.bad) return XLZ_ERR_RESULT;
        id = r.byte();
    }
    if (id == kUnPackInfo) {
        if (r.byte() != kFolder) return XLZ_ERR_RESULT;
        const uint64_t nf = r.number();
        if (nf > kMaxItems) return XLZ_ERR_UNSUPPORTED;
        if (r.byte() != 0) return XLZ_ERR_UNSUPPORTED; // external folder definitions
        if (nf > r.left() / 3) return XLZ_ERR_RESULT; // a folder takes >= 2 header bytes + 1 byte of unpack size
        s.folders.resize((size_t)nf);
        for (auto &f : s.folders)
            if (!read_folder(r, f)) return XLZ_ERR_RESULT;
        if (r.byte() != kCodersUnPackSize) return XLZ_ERR_RESULT;
        for (auto &f : s.folders) {
            uint64_t main_size = 0;
            bool same = true;
            for (uint32_t k = 0; k < f.n_out; k++) {
                const uint64_t v = r.number();
                if (f.bcj2) {
                    for (auto &sb : f.bsub)
                        if (sb.method != XLZ_7Z_COPY && sb.out_index == k) sb.unpack = v;
                    if (f.bcj2_out_index == k) f.bcj2_final = v;
                }
                if (k + 1 == f.n_out || f.n_out == 1) f.unpack_size = v; // single coder: its one output
                if (k == 0) main_size = v;
                same = same && v == main_size;
            }
            // a chain's filters keep the size: the folder's unpack size is that of the output no bind pair consumes, and
            // every intermediate size must equal it
            if (f.chain && !same) f.chain = false, f.steps.clear();
            if (f.bcj2 && bcj2) f.unpack_size = f.bcj2_final;
        }
        id = r.byte();
        if (id == kCRC) {
            Digests d;
            if (!read_digests(r, nf, d)) return XLZ_ERR_RESULT;
            for (size_t i = 0; i < s.folders.size(); i++) {
                s.folders[i].has_crc = d.defined[i];
                s.folders[i].crc = d.crc[i];
            }
            id = r.byte();
        }
        if (id != kEnd || r.bad) return XLZ_ERR_RESULT;
        id = r.byte();
    }
    bool have_sub = false;
    if (id == kSubStreamsInfo) {
        have_sub = true;
        id = r.byte();
        if (id == kNumUnPackStream) {
            for (auto &f : s.folders) {
                f.n_sub = r.number();
                if (f.n_sub > kMaxItems) return XLZ_ERR_UNSUPPORTED;
            }
            id = r.byte();
        }
        uint64_t total_sub = 0, sized = 0;
        for (auto &f : s.folders) {
            total_sub += f.n_sub;
            sized += f.n_sub ? f.n_sub - 1 : 0; // sizes in the header: all but the last of each folder
        }
        if (total_sub > kMaxItems) return XLZ_ERR_UNSUPPORTED;
        // the sizes must be in the header (one byte each at least); without a kSize attribute a folder has at most
        // one stream whose size is known at all
        if (sized > (id == kSize ? (uint64_t)r.left() : 0)) return XLZ_ERR_RESULT;
        s.subs.clear();
        for (auto &f : s.folders) { // sizes: all but the last of each folder, the last is the rest
            uint64_t sum = 0;
            for (uint64_t k = 0; k + 1 < f.n_sub; k++) {
                const uint64_t v = id == kSize ? r.number() : 0;
                if (v > f.unpack_size - sum) return XLZ_ERR_RESULT;
                sum += v;
                s.subs.push_back({v, 0, 0});
            }
            if (f.n_sub) s.subs.push_back({f.unpack_size - sum, 0, 0});
        }
        if (id == kSize) id = r.byte();
        if (id == kCRC) { // digests of the streams whose CRC is not known from the folder
            uint64_t need = 0;
            for (auto &f : s.folders)
                if (!(f.n_sub == 1 && f.has_crc)) need += f.n_sub;
            Digests d;
            if (!read_digests(r, need, d)) return XLZ_ERR_RESULT;
            size_t di = 0, si = 0;
            for (auto &f : s.folders) {
                for (uint64_t k = 0; k < f.n_sub; k++, si++) {
                    if (f.n_sub == 1 && f.has_crc) {
                        s.subs[si].crc = f.crc;
                        s.subs[si].has_crc = 1;
                    } else {
                        s.subs[si].crc = d.crc[di];
                        s.subs[si].has_crc = d.defined[di];
                        di++;
                    }
                }
            }
            id = r.byte();
        } else {
            size_t si = 0;
            for (auto &f : s.folders)
                for (uint64_t k = 0; k < f.n_sub; k++, si++)
                    if (f.n_sub == 1 && f.has_crc) {
                        s.subs[si].crc = f.crc;
                        s.subs[si].has_crc = 1;
                    }
        }
        if (id != kEnd || r.bad) return XLZ_ERR_RESULT;
        id = r.byte();
    }
    if (!have_sub) { // one stream per folder
        s.subs.clear();
        for (auto &f : s.folders) s.subs.push_back({f.unpack_size, f.has_crc ? f.crc : 0u, f.has_crc ? 1u : 0u});
    }
    if (id != kEnd || r.bad) return XLZ_ERR_RESULT;
    return XLZ_OK;
}

// lay the folders of a StreamsInfo out against the file: packed streams follow each other from
// 32 + PackPos
// chains: folders that are a chain (Folder::chain) are laid out as their LZMA / LZMA2 coder
// bcj2: folders that are one of the BCJ2 forms (Folder::bcj2) come back as XLZ_7Z_BCJ2, each with a record in *bcj2
int place_folders(const Streams &s, size_t file_len, std::vector<xlz_7z_folder> &out, bool chains = false, std::vector<xlz_7z_bcj2> *bcj2 = nullptr)
{
    out.clear();
    if (bcj2) bcj2->clear();
    uint64_t off = 32 + s.pack_pos, uoff = 0;
    size_t pi = 0, si = 0;
    for (const Folder &f0 : s.folders) {
        Folder f = f0;
        if (chains && f.chain) f.method = f.chain_method, f.props = f.chain_props, f.dict_size = f.chain_dict;
        xlz_7z_folder o;
        memset(&o, 0, sizeof o);
        o.method = f.method;
        if (f.n_pack != 1) o.method = XLZ_7Z_UNSUPPORTED;
        if (f.n_pack < 1 || pi >= s.pack_sizes.size() || f.n_pack > s.pack_sizes.size() - pi) return XLZ_ERR_RESULT;
        o.pack_off = off;
        o.pack_len = s.pack_sizes[pi];
        if (bcj2 && f.bcj2 && f.n_pack == 4) {
            xlz_7z_bcj2 rec;
            memset(&rec, 0, sizeof rec);
            rec.folder = out.size();
            uint64_t offk[4], at = off;
            for (uint32_t k = 0; k < 4; k++) offk[k] = at, at += s.pack_sizes[pi + k]; // (checked against the file below)
            bool ok = true;
            xlz_7z_bcj2_sub *dst[3] = {&rec.main_s, &rec.call_s, &rec.jump_s};
            for (uint32_t j = 0; j < 3; j++) {
                const Folder::Bcj2Sub &sb = f.bsub[j];
                xlz_7z_bcj2_sub &d = *dst[j];
                d.pack_off = offk[sb.pack_k], d.pack_len = s.pack_sizes[pi + sb.pack_k];
                d.method = sb.method, d.props = sb.props;
                d.unpack_len = sb.method == XLZ_7Z_COPY ? d.pack_len : sb.unpack;
                d.dict_size = sb.method == XLZ_7Z_LZMA2 ? (sb.props == 40 ? 0xFFFFFFFFu : xlz_decode_dict_size2(sb.props)) : sb.dict;
                if (sb.method == XLZ_7Z_LZMA2 && sb.props > 40) ok = false;
                if (j && (d.unpack_len & 3)) ok = false; // call / jump: four bytes per operand
            }
            rec.rc_off = offk[f.rc_pack_k], rec.rc_len = s.pack_sizes[pi + f.rc_pack_k];
            if (ok) {
                o.method = XLZ_7Z_BCJ2;
                bcj2->push_back(rec);
            }
        }
        for (uint32_t k = 0; k < f.n_pack; k++) {
            const uint64_t sz = s.pack_sizes[pi + k];
            if (off > file_len || sz > file_len - off) return XLZ_ERR_UNEXPECTED_EOF;
            off += sz;
        }
        pi += f.n_pack;
        o.unpack_off = uoff;
        o.unpack_len = f.unpack_size;
        if (f.unpack_size > ~0ull - uoff) return XLZ_ERR_RESULT;
        uoff += f.unpack_size;
        o.props = f.props;
        o.dict_size = f.method == XLZ_7Z_LZMA2 ? xlz_decode_dict_size2(f.props) : f.dict_size;
        if (f.method == XLZ_7Z_LZMA2 && f.props > 40) o.method = XLZ_7Z_UNSUPPORTED;
        if (f.method == XLZ_7Z_LZMA2 && f.props == 40) o.dict_size = 0xFFFFFFFFu;
        o.has_crc = f.has_crc;
        o.crc = f.crc;
        o.first_substream = (uint32_t)si;
        o.n_substreams = (uint32_t)f.n_sub;
        si += (size_t)f.n_sub;
        out.push_back(o);
    }
    return XLZ_OK;
}

// fn(off, len, crc) for every file of the folder that carries a CRC, in the folder's order (off: inside the folder's
// bytes), then for the folder itself if it carries one.  -> how many that were
template <class Fn> size_t each_crc(const xlz_7z_folder &f, const std::vector<xlz_7z_substream> &subs, Fn &&fn)
{
    size_t n = 0;
    uint64_t o = 0;
    for (uint32_t j = 0; j < f.n_substreams; j++) {
        const xlz_7z_substream &ss = subs[f.first_substream + j];
        if (ss.has_crc) fn(o, ss.size, ss.crc), n++;
        o += ss.size;
    }
    if (f.has_crc) fn((uint64_t)0, f.unpack_len, f.crc), n++;
    return n;
}

// what a call of decode_folders is asked for
struct FolderOpts {
    uint8_t *out = nullptr; // the host destination, or ...
    void *d_out = nullptr;  // ... the device destination of d_cap bytes (xlz_7z_decode_device)
    size_t d_cap = 0;
    int verify = 0;
    size_t *unverified = nullptr;
    const std::vector<Folder> *chains = nullptr;    // filter mode 1: the folders' filter steps (Folder::steps)
    const std::vector<xlz_7z_bcj2> *brecs = nullptr; // bcj2 mode 1 / 2 (d_out only): the BCJ2 folders' records
    int bcj2_mode = 0;
};

// The folders as one batch.  LZMA / LZMA2 folders are streams (which[k]: stream k's folder); a BCJ2 folder's LZMA / LZMA2
// sub-streams are further streams (no_pack: not packed) and the folder an item that is merged into the device destination
// behind the pack; Copy folders go to the destination from the file as they are.  dev_checks: cr[first[i] ...] = the
// CRC32 ranges of folder i in each_crc's order, over its stream or -- a BCJ2 folder -- over the destination.
struct FolderPlan {
    std::vector<xlz_stream_desc> d;
    std::vector<size_t> which;
    std::vector<uint8_t> no_pack;
    std::vector<uint64_t> want_out, dst_off;
    std::vector<xlz_filter_step> fs;
    std::vector<DeviceCopy> copies;
    std::vector<xlz_bcj2_item> bitems;
    std::vector<xlz_check_range> cr;
    std::vector<size_t> first;
};
int plan_folders(const uint8_t *file, const std::vector<xlz_7z_folder> &fo, const std::vector<xlz_7z_substream> &subs, const FolderOpts &o,
                 bool dev_checks, FolderPlan &p)
{
    size_t next_rec = 0;
    p.first.assign(fo.size(), 0);
    auto add_stream = [&](size_t folder, uint32_t method, uint64_t pack_off, uint64_t pack_len, uint64_t unpack_len, uint8_t props,
                          uint32_t dict_size, bool packed, uint64_t dst) {
        xlz_stream_desc s;
        memset(&s, 0, sizeof s);
        s.in = file + pack_off, s.in_len = (size_t)pack_len, s.out_cap = (size_t)unpack_len;
        s.out = packed && !o.d_out ? o.out + dst : nullptr;
        s.dict_size = dict_size; // (the batch engine applies DecodeDictSize's 4096 floor)
        if (method == XLZ_7Z_LZMA) // NewLZMADecompressorForSevenZip(props, unpackSize, readers), reader1.go:32-61
            s.format = XLZ_FMT_LZMA_RAW, s.props = props, s.unpack_size = unpack_len;
        else // NewLZMA2DecompressorForSevenZip(props, _, readers), reader2.go:49-75
            s.format = XLZ_FMT_LZMA2_RAW;
        p.d.push_back(s), p.which.push_back(folder), p.no_pack.push_back(!packed);
        p.want_out.push_back(unpack_len), p.dst_off.push_back(dst);
    };
    for (size_t i = 0; i < fo.size(); i++) {
        const xlz_7z_folder &f = fo[i];
        xlz_check_range c;
        memset(&c, 0, sizeof c);
        c.stream = p.d.size(), c.kind = XLZ_CHECK_CRC32;
        uint64_t c_base = 0; // where the folder's bytes begin in what c.stream names
        if (f.method == XLZ_7Z_UNSUPPORTED) return XLZ_ERR_UNSUPPORTED;
        if (f.method == XLZ_7Z_COPY) {
            if (f.pack_len != f.unpack_len) return XLZ_ERR_RESULT;
            p.copies.push_back(DeviceCopy{f.unpack_off, file + f.pack_off, f.unpack_len});
            continue; // (its CRCs are the host's)
        }
        if (f.method == XLZ_7Z_BCJ2) {
            if (!o.d_out || !o.brecs || next_rec >= o.brecs->size() || (*o.brecs)[next_rec].folder != i) return XLZ_ERR_UNSUPPORTED;
            const xlz_7z_bcj2 &rec = (*o.brecs)[next_rec++];
            if (f.unpack_len > 0xFFFFFFFFull) return XLZ_ERR_UNSUPPORTED; // (a folder of 4 GiB or more)
            xlz_bcj2_item it;
            memset(&it, 0, sizeof it);
            const xlz_7z_bcj2_sub *sub[3] = {&rec.main_s, &rec.call_s, &rec.jump_s};
            xlz_bcj2_src *src[3] = {&it.main_s, &it.call_s, &it.jump_s};
            for (int j = 0; j < 3; j++) {
                if (sub[j]->method == XLZ_7Z_COPY) { // read raw: it goes up from the file with the call
                    src[j]->stream = XLZ_BCJ2_RAW, src[j]->raw = file + sub[j]->pack_off, src[j]->raw_len = sub[j]->pack_len;
                    continue;
                }
                src[j]->stream = p.d.size();
                add_stream(i, sub[j]->method, sub[j]->pack_off, sub[j]->pack_len, sub[j]->unpack_len, sub[j]->props, sub[j]->dict_size, false, 0);
            }
            it.rc = file + rec.rc_off, it.rc_len = rec.rc_len, it.out_len = f.unpack_len, it.dst_off = f.unpack_off;
            p.bitems.push_back(it);
            c.stream = xlzpost::kDestStream, c_base = f.unpack_off; // (the merged bytes never sit in the arena)
        } else {
            if (o.chains && (*o.chains)[i].chain)
                for (const auto &stp : (*o.chains)[i].steps) {
                    xlz_filter_step q;
                    memset(&q, 0, sizeof q);
                    q.stream = p.d.size(), q.id = stp.first, q.param = stp.second;
                    p.fs.push_back(q);
                }
            add_stream(i, f.method, f.pack_off, f.pack_len, f.unpack_len, f.props, f.dict_size, true, f.unpack_off);
        }
        p.first[i] = p.cr.size();
        if (dev_checks)
            each_crc(f, subs, [&](uint64_t off, uint64_t len, uint32_t) {
                c.off = c_base + off, c.len = len;
                p.cr.push_back(c);
            });
    }
    return XLZ_OK;
}

// decode the given folders (all of a StreamsInfo) into o.out or o.d_out, verify their CRCs.  ctxs[0] runs the batch; more
// than one context: the folders are dealt to several GPUs (xlz_decode_batch_multi)
int decode_folders(xlz_ctx *const *ctxs, size_t n_ctx, const uint8_t *file, const std::vector<xlz_7z_folder> &fo,
                   const std::vector<xlz_7z_substream> &subs, const FolderOpts &o)
{
    xlz_ctx *ctx = ctxs[0];
    // check mode 1 (xlz_ctx_set_check_mode; one context): the CRC32 of every file and folder that the batch decodes comes
    // from the device with the batch's results -- per-file ranges inside solid folders
    // (a device destination: there are no bytes on the host to check, so always)
    const bool dev = o.verify && n_ctx <= 1 && ctx && (o.d_out || xlz_ctx_check_mode(ctx) >= 1);
    FolderPlan p;
    int st = plan_folders(file, fo, subs, o, dev, p);
    if (st != XLZ_OK) return st;
    // run: the host batch, the multi-GPU batch, or (a device destination) one batch with the pack, the merges and the
    // Copy folders' upload behind it
    std::vector<xlz_result> r(p.d.size());
    std::vector<xlz_bcj2_result> bres(p.bitems.size());
    std::vector<uint64_t> dg(p.cr.size());
    if (!o.d_out)
        for (const DeviceCopy &c : p.copies) memcpy(o.out + c.dst_off, c.src, (size_t)c.len);
    if (dev || !p.fs.empty() || o.d_out) { // (without dev the CRCs, if asked for, on host threads below: over the filtered bytes)
        const PostWork w = {p.fs.data(), p.fs.size(), p.cr.data(), p.cr.size(), dg.data(), nullptr, true};
        if (o.d_out) {
            DeviceDest dest;
            dest.d_dst = o.d_out, dest.cap = o.d_cap, dest.want_out = p.want_out.data(), dest.dst_off = p.dst_off.data();
            dest.copies = p.copies.data(), dest.n_copies = p.copies.size(), dest.no_pack = p.no_pack.data();
            dest.bcj2 = p.bitems.data(), dest.n_bcj2 = p.bitems.size(), dest.bcj2_res = bres.data(), dest.bcj2_mode = o.bcj2_mode;
            st = xlz_internal_decode_device(ctx, p.d.data(), p.d.size(), r.data(), w, dest);
        } else if (!p.d.empty())
            st = xlz_internal_decode_batch(ctx, p.d.data(), p.d.size(), r.data(), w);
    } else if (!p.d.empty())
        st = n_ctx > 1 ? xlz_decode_batch_multi(ctxs, n_ctx, p.d.data(), p.d.size(), r.data())
                       : xlz_decode_batch(ctx, p.d.data(), p.d.size(), r.data());
    if (st != XLZ_OK) return st;
    for (size_t k = 0; k < p.d.size(); k++) {
        if (r[k].status < 0) return r[k].status;
        if (r[k].out_len != p.want_out[k]) return XLZ_ERR_RESULT; // a folder (a BCJ2 folder's stream) decodes to exactly its size
    }
    for (const xlz_bcj2_result &q : bres)
        if (q.status < 0) return q.status == XLZ_ERR_UNSUPPORTED ? XLZ_ERR_UNSUPPORTED : XLZ_ERR_RESULT; // a merge that failed
    if (!o.verify) return XLZ_OK;
    // verify: every CRC against the device's digest, or against the host's over the folder's bytes -- in the caller's
    // buffer, or (a device destination, where only Copy folders are the host's) in the file
    std::vector<int> bad(fo.size(), 0); // 1: a CRC differs, 2: there was none
    xlzpost::parallel_for(fo.size(), xlzpost::host_thread_cap(16), [&](size_t i) {
        const xlz_7z_folder &f = fo[i];
        const uint8_t *fb = o.d_out ? file + f.pack_off : o.out + f.unpack_off;
        const bool on_dev = dev && f.method != XLZ_7Z_COPY; // (Copy folders never were on the device)
        size_t q = p.first[i];
        bool differs = false;
        const size_t n = each_crc(f, subs, [&](uint64_t off, uint64_t len, uint32_t crc) {
            if ((on_dev ? (uint32_t)dg[q++] : xlzcheck::crc32(fb + off, (size_t)len)) != crc) differs = true;
        });
        bad[i] = differs ? 1 : n ? 0 : 2;
    });
    for (size_t i = 0; i < fo.size() && dev; i++) // (the Copy folders' CRCs were the host's)
        if (fo[i].method == XLZ_7Z_COPY) {
            uint64_t nbytes = 0;
            const size_t nr = each_crc(fo[i], subs, [&](uint64_t, uint64_t len, uint32_t) { nbytes += len; });
            if (nr) xlz_internal_check_stats_host(ctx, nr, nbytes);
        }
    size_t nu = 0;
    for (size_t i = 0; i < fo.size(); i++) {
        if (bad[i] == 1) return XLZ_ERR_RESULT;
        nu += bad[i] == 2;
    }
    if (o.unverified) *o.unverified = nu;
    return XLZ_OK;
}

// signature header -> the (possibly still encoded) header bytes
int locate_header(const uint8_t *file, size_t len, const uint8_t *&hdr, size_t &hdr_len)
{
    if (len < 32) return XLZ_ERR_UNEXPECTED_EOF;
    if (memcmp(file, kMagic, 6) != 0) return XLZ_ERR_RESULT;
    if (file[6] != 0) return XLZ_ERR_UNSUPPORTED; // major version
    if (xlzcheck::crc32(file + 12, 20) != le32(file + 8)) return XLZ_ERR_RESULT;
    const uint64_t off = le64(file + 12), size = le64(file + 20);
    if (off > len - 32 || size > len - 32 - off) return XLZ_ERR_UNEXPECTED_EOF;
    hdr = file + 32 + off;
    hdr_len = (size_t)size;
    if (size && xlzcheck::crc32(hdr, hdr_len) != le32(file + 28)) return XLZ_ERR_RESULT;
    return XLZ_OK;
}

// the archive's MAIN StreamsInfo.  An encoded header (what 7-Zip writes by default) is itself a
// folder: it is decoded with the batch engine first (needs ctx).
// rest (optional, xlz_7z_open): what follows the StreamsInfo inside the header -- FilesInfo, if there is one; it points into
// the file or into decoded_header
struct HeaderRest {
    const uint8_t *p = nullptr;
    size_t n = 0;
};
int main_streams(xlz_ctx *ctx, const uint8_t *file, size_t len, Streams &s, std::vector<uint8_t> &decoded_header, bool bcj2 = false,
                 HeaderRest *rest = nullptr)
{
    const uint8_t *hdr;
    size_t hl;
    int st = locate_header(file, len, hdr, hl);
    if (st != XLZ_OK) return st;
    if (hl == 0) return XLZ_OK; // empty archive
    for (int depth = 0; depth < 4; depth++) {
        Rd r{hdr, hl};
        const uint8_t id = r.byte();
        if (id == kEncodedHeader) {
            Streams es;
            st = read_streams_info(r, es);
            if (st != XLZ_OK) return st;
            std::vector<xlz_7z_folder> fo;
            st = place_folders(es, len, fo);
            if (st != XLZ_OK) return st;
            if (fo.size() != 1) return XLZ_ERR_UNSUPPORTED;
            if (fo[0].unpack_len > (256u << 20)) return XLZ_ERR_UNSUPPORTED;
            if (!ctx && fo[0].method != XLZ_7Z_COPY) return XLZ_ERR_DEVICE; // decoding the header needs the GPU
            std::vector<uint8_t> next((size_t)fo[0].unpack_len + 1);
            FolderOpts o;
            o.out = next.data(), o.verify = 1;
            st = decode_folders(&ctx, 1, file, fo, es.subs, o);
            if (st != XLZ_OK) return st;
            next.resize((size_t)fo[0].unpack_len);
            decoded_header.swap(next);
            hdr = decoded_header.data();
            hl = decoded_header.size();
            continue;
        }
        if (id != kHeader) return XLZ_ERR_RESULT;
        uint8_t t = r.byte();
        if (t == kArchiveProperties) {
            for (;;) {
                const uint8_t pt = r.byte();
                if (pt == kEnd || r.bad) break;
                if (!r.skip(r.number())) return XLZ_ERR_RESULT;
            }
            t = r.byte();
        }
        if (t == kAdditionalStreamsInfo) return XLZ_ERR_UNSUPPORTED;
        if (t == kMainStreamsInfo) {
            st = read_streams_info(r, s, bcj2);
            if (st == XLZ_OK && rest) rest->p = r.p + r.pos, rest->n = r.left();
            return st;
        }
        if (!r.bad && rest) rest->p = r.p + r.pos - 1, rest->n = r.left() + 1; // (from the byte that was no StreamsInfo)
        return r.bad ? XLZ_ERR_RESULT : XLZ_OK; // no streams: only empty files
    }
    return XLZ_ERR_UNSUPPORTED;
}

} // namespace

extern "C" int xlz_7z_index(xlz_ctx *ctx, const uint8_t *file, size_t len, xlz_7z_folder *folders, size_t max_folders,
                            size_t *n_folders, xlz_7z_substream *substreams, size_t max_substreams, size_t *n_substreams,
                            uint64_t *total_unpacked)
{
    if (!file || !n_folders || (!folders && max_folders) || (!substreams && max_substreams)) return XLZ_ERR_BAD_ARG;
    *n_folders = 0;
    if (n_substreams) *n_substreams = 0;
    if (total_unpacked) *total_unpacked = 0;
    Streams s;
    std::vector<uint8_t> dh;
    int st = main_streams(ctx, file, len, s, dh);
    if (st != XLZ_OK) return st;
    std::vector<xlz_7z_folder> fo;
    st = place_folders(s, len, fo);
    if (st != XLZ_OK) return st;
    uint64_t total = 0;
    for (size_t i = 0; i < fo.size(); i++) {
        if (i < max_folders) folders[i] = fo[i];
        total += fo[i].unpack_len;
    }
    for (size_t i = 0; i < s.subs.size() && i < max_substreams; i++) substreams[i] = s.subs[i];
    *n_folders = fo.size();
    if (n_substreams) *n_substreams = s.subs.size();
    if (total_unpacked) *total_unpacked = total;
    if ((max_folders && fo.size() > max_folders) || (max_substreams && s.subs.size() > max_substreams)) return XLZ_ERR_OUT_CAP;
    return XLZ_OK;
}

// xlz_7z_index for archives whose folders are coder chains: a folder that is a line of Delta / BCJ filters behind one LZMA /
// LZMA2 coder comes back with that coder's method, props and dictionary, and its filters as steps in the order a decoder
// applies them, step.stream = the folder's index.
extern "C" int xlz_7z_index_chains(xlz_ctx *ctx, const uint8_t *file, size_t len, xlz_7z_folder *folders, size_t max_folders,
                                   size_t *n_folders, xlz_7z_substream *substreams, size_t max_substreams, size_t *n_substreams,
                                   xlz_filter_step *steps, size_t max_steps, size_t *n_steps, uint64_t *total_unpacked)
{
    if (!file || !n_folders || !n_steps || (!folders && max_folders) || (!substreams && max_substreams) || (!steps && max_steps))
        return XLZ_ERR_BAD_ARG;
    *n_folders = 0, *n_steps = 0;
    if (n_substreams) *n_substreams = 0;
    if (total_unpacked) *total_unpacked = 0;
    Streams s;
    std::vector<uint8_t> dh;
    int st = main_streams(ctx, file, len, s, dh);
    if (st != XLZ_OK) return st;
    std::vector<xlz_7z_folder> fo;
    st = place_folders(s, len, fo, true);
    if (st != XLZ_OK) return st;
    uint64_t total = 0;
    size_t ns = 0;
    for (size_t i = 0; i < fo.size(); i++) {
        if (i < max_folders) folders[i] = fo[i];
        total += fo[i].unpack_len;
        if (s.folders[i].chain)
            for (const auto &stp : s.folders[i].steps) {
                if (ns < max_steps) {
                    memset(&steps[ns], 0, sizeof steps[ns]);
                    steps[ns].stream = i, steps[ns].id = stp.first, steps[ns].param = stp.second;
                }
                ns++;
            }
    }
    for (size_t i = 0; i < s.subs.size() && i < max_substreams; i++) substreams[i] = s.subs[i];
    *n_folders = fo.size(), *n_steps = ns;
    if (n_substreams) *n_substreams = s.subs.size();
    if (total_unpacked) *total_unpacked = total;
    if ((max_folders && fo.size() > max_folders) || (max_substreams && s.subs.size() > max_substreams) || (max_steps && ns > max_steps))
        return XLZ_ERR_OUT_CAP;
    return XLZ_OK;
}

// xlz_7z_index_chains plus the BCJ2 folders: method XLZ_7Z_BCJ2, the size of the merged bytes, and a record each that
// places main, call, jump and the range coder's bytes inside the file.
extern "C" int xlz_7z_index_bcj2(xlz_ctx *ctx, const uint8_t *file, size_t len, xlz_7z_folder *folders, size_t max_folders, size_t *n_folders,
                                 xlz_7z_substream *substreams, size_t max_substreams, size_t *n_substreams, xlz_filter_step *steps,
                                 size_t max_steps, size_t *n_steps, xlz_7z_bcj2 *bcj2, size_t max_bcj2, size_t *n_bcj2, uint64_t *total_unpacked)
{
    if (!file || !n_folders || !n_steps || !n_bcj2 || (!folders && max_folders) || (!substreams && max_substreams) || (!steps && max_steps) ||
        (!bcj2 && max_bcj2))
        return XLZ_ERR_BAD_ARG;
    *n_folders = 0, *n_steps = 0, *n_bcj2 = 0;
    if (n_substreams) *n_substreams = 0;
    if (total_unpacked) *total_unpacked = 0;
    Streams s;
    std::vector<uint8_t> dh;
    int st = main_streams(ctx, file, len, s, dh, true);
    if (st != XLZ_OK) return st;
    std::vector<xlz_7z_folder> fo;
    std::vector<xlz_7z_bcj2> recs;
    st = place_folders(s, len, fo, true, &recs);
    if (st != XLZ_OK) return st;
    uint64_t total = 0;
    size_t ns = 0;
    for (size_t i = 0; i < fo.size(); i++) {
        if (i < max_folders) folders[i] = fo[i];
        total += fo[i].unpack_len;
        if (s.folders[i].chain)
            for (const auto &stp : s.folders[i].steps) {
                if (ns < max_steps) {
                    memset(&steps[ns], 0, sizeof steps[ns]);
                    steps[ns].stream = i, steps[ns].id = stp.first, steps[ns].param = stp.second;
                }
                ns++;
            }
    }
    for (size_t i = 0; i < s.subs.size() && i < max_substreams; i++) substreams[i] = s.subs[i];
    for (size_t i = 0; i < recs.size() && i < max_bcj2; i++) bcj2[i] = recs[i];
    *n_folders = fo.size(), *n_steps = ns, *n_bcj2 = recs.size();
    if (n_substreams) *n_substreams = s.subs.size();
    if (total_unpacked) *total_unpacked = total;
    if ((max_folders && fo.size() > max_folders) || (max_substreams && s.subs.size() > max_substreams) || (max_steps && ns > max_steps) ||
        (max_bcj2 && recs.size() > max_bcj2))
        return XLZ_ERR_OUT_CAP;
    return XLZ_OK;
}

static int sz_decode(xlz_ctx *const *ctxs, size_t n_ctx, const uint8_t *file, size_t len, uint8_t *out, size_t out_cap,
                     uint64_t *out_len, int verify, size_t *unverified, void *d_out = nullptr);

// Into device memory: the same parse, batch and comparisons as xlz_7z_decode; the CRCs of what the batch decodes always come
// from the device (as in check mode 1), Copy folders are uploaded from the file and checked there, and a pack puts the
// folders side by side in d_out (xlz_internal_decode_device).  An encoded header is decoded into host memory as ever.
extern "C" int xlz_7z_decode_device(xlz_ctx *ctx, const uint8_t *file, size_t len, void *d_out, size_t out_cap, uint64_t *out_len,
                                    int verify, size_t *unverified)
{
    if (!ctx || (!d_out && out_cap)) return XLZ_ERR_BAD_ARG;
    uint8_t none = 0; // (an empty archive needs no destination)
    const int st = sz_decode(&ctx, 1, file, len, nullptr, out_cap, out_len, verify, unverified, d_out ? d_out : &none);
    if (st != XLZ_OK && out_len) *out_len = 0;
    return st;
}

extern "C" int xlz_7z_decode(xlz_ctx *ctx, const uint8_t *file, size_t len, uint8_t *out, size_t out_cap, uint64_t *out_len,
                             int verify, size_t *unverified)
{
    return sz_decode(&ctx, 1, file, len, out, out_cap, out_len, verify, unverified);
}

// several contexts (one per GPU): the folders, and the units inside large LZMA2 folders, are dealt by
// xlz_decode_batch_multi; encoded headers are decoded on the first context
extern "C" int xlz_7z_decode_multi(xlz_ctx *const *ctxs, size_t n_ctx, const uint8_t *file, size_t len, uint8_t *out,
                                   size_t out_cap, uint64_t *out_len, int verify, size_t *unverified)
{
    if (!ctxs || !n_ctx) return XLZ_ERR_BAD_ARG;
    return sz_decode(ctxs, n_ctx, file, len, out, out_cap, out_len, verify, unverified);
}

static int sz_decode(xlz_ctx *const *ctxs, size_t n_ctx, const uint8_t *file, size_t len, uint8_t *out, size_t out_cap,
                     uint64_t *out_len, int verify, size_t *unverified, void *d_out)
{
    for (size_t c = 0; c < n_ctx; c++)
        if (!ctxs[c]) return XLZ_ERR_BAD_ARG;
    xlz_ctx *ctx = ctxs[0];
    if (!file || (!out && out_cap && !d_out) || !out_len) return XLZ_ERR_BAD_ARG;
    *out_len = 0;
    if (unverified) *unverified = 0;
    if (verify && n_ctx == 1 && (d_out || xlz_ctx_check_mode(ctx) >= 1)) xlz_internal_check_stats_reset(ctx); // (an encoded header's batch counts too)
    // bcj2 mode 1 / 2 (xlz_ctx_set_bcj2_mode; one context): BCJ2 folders are decoded, merged into device memory
    const int bmode = n_ctx == 1 ? xlz_ctx_bcj2_mode(ctx) : 0;
    if (bmode > 0) xlz_internal_bcj2_stats_reset(ctx);
    Streams s;
    std::vector<uint8_t> dh;
    int st = main_streams(ctx, file, len, s, dh, bmode > 0);
    if (st != XLZ_OK) return st;
    // filter mode 1 (xlz_ctx_set_filter_mode; one context): folders that are a chain of filters behind an LZMA / LZMA2 coder
    const bool chains = n_ctx == 1 && xlz_ctx_filter_mode(ctx) == 1;
    if (chains) xlz_internal_filter_stats_reset(ctx);
    std::vector<xlz_7z_folder> fo;
    std::vector<xlz_7z_bcj2> brecs;
    st = place_folders(s, len, fo, chains, bmode > 0 ? &brecs : nullptr);
    if (st != XLZ_OK) return st;
    uint64_t total = 0;
    for (auto &f : fo) total += f.unpack_len;
    if (total > out_cap) return XLZ_ERR_OUT_CAP;
    FolderOpts o;
    o.out = out, o.d_out = d_out, o.d_cap = out_cap, o.verify = verify, o.unverified = unverified;
    o.chains = chains ? &s.folders : nullptr, o.brecs = &brecs, o.bcj2_mode = bmode;
    // an archive that HAS a BCJ2 folder: the device-destination path -- for a host destination into a block from the
    // context's pool, followed by one download
    void *blk = nullptr;
    for (auto &f : fo)
        if (!brecs.empty() && f.method == XLZ_7Z_UNSUPPORTED) return XLZ_ERR_UNSUPPORTED;
    if (!brecs.empty() && !d_out) {
        st = xlz_internal_device_block(ctx, (size_t)total, &blk);
        if (st != XLZ_OK) return st;
        if (verify) xlz_internal_check_stats_reset(ctx);
        o.out = nullptr, o.d_out = blk, o.d_cap = (size_t)total;
    }
    st = decode_folders(ctxs, n_ctx, file, fo, s.subs, o);
    if (st == XLZ_OK && blk) st = xlz_internal_device_block_download(ctx, blk, out, (size_t)total);
    xlz_internal_device_block_release(ctx, blk);
    if (st != XLZ_OK) return st;
    *out_len = total;
    return XLZ_OK;
}

// ---------------------------------------------------------------- the file table ----
// xlz_7z_index_bcj2's parse, then FilesInfo (xlz_7z_files.h).  What uses the table on the device is in xlz_7z_extract.hip.
extern "C" int xlz_7z_open(xlz_ctx *ctx, const uint8_t *file, size_t len, xlz_7z_archive **a)
{
    if (!a) return XLZ_ERR_BAD_ARG;
    *a = nullptr;
    if (!file) return XLZ_ERR_BAD_ARG;
    Streams s;
    std::vector<uint8_t> dh;
    HeaderRest rest;
    int st = main_streams(ctx, file, len, s, dh, true, &rest);
    if (st != XLZ_OK) return st;
    xlz_7z_archive *h = new (std::nothrow) xlz_7z_archive;
    if (!h) return XLZ_ERR_DEVICE;
    h->file = file, h->len = len;
    std::vector<xlz_7z_bcj2> recs;
    st = place_folders(s, len, h->folders, true, &recs);
    xlz7zf::Files files;
    if (st == XLZ_OK && rest.n && rest.p[0] == kFilesInfo) {
        size_t used = 0;
        st = xlz7zf::parse_files(rest.p + 1, rest.n - 1, files, &used);
        // (behind the section: the header's end mark)
        if (st == XLZ_OK && !(rest.n - 1 - used >= 1 && rest.p[1 + used] == kEnd)) st = XLZ_ERR_RESULT;
    } else if (st == XLZ_OK && rest.n && rest.p[0] != kEnd) {
        st = XLZ_ERR_RESULT;
    }
    if (st == XLZ_OK) st = xlz7zf::build_entries(files, h->folders.data(), h->folders.size(), s.subs.data(), s.subs.size(), h->entries);
    if (st != XLZ_OK) {
        delete h;
        return st;
    }
    h->subs.swap(s.subs), h->names.swap(files.names);
    for (size_t i = 0; i < h->folders.size(); i++)
        if (s.folders[i].chain)
            for (const auto &stp : s.folders[i].steps) {
                xlz_filter_step q;
                memset(&q, 0, sizeof q);
                q.stream = i, q.id = stp.first, q.param = stp.second;
                h->steps.push_back(q);
            }
    for (const xlz_7z_entry &e : h->entries) h->total_size += e.size; // (no wrap: the folders' sizes add up, place_folders)
    *a = h;
    return XLZ_OK;
}

extern "C" void xlz_7z_close(xlz_7z_archive *a) { delete a; }

extern "C" int xlz_7z_archive_info(const xlz_7z_archive *a, size_t *n_entries, size_t *n_folders, size_t *name_bytes, uint64_t *total_size)
{
    if (!a) return XLZ_ERR_BAD_ARG;
    if (n_entries) *n_entries = a->entries.size();
    if (n_folders) *n_folders = a->folders.size();
    if (name_bytes) *name_bytes = a->names.size();
    if (total_size) *total_size = a->total_size;
    return XLZ_OK;
}

extern "C" int xlz_7z_archive_entries(const xlz_7z_archive *a, xlz_7z_entry *entries, size_t max_entries, char *names, size_t names_cap)
{
    if (!a || (!entries && max_entries) || (!names && names_cap)) return XLZ_ERR_BAD_ARG;
    std::copy_n(a->entries.begin(), std::min(max_entries, a->entries.size()), entries);
    std::copy_n(a->names.begin(), std::min(names_cap, a->names.size()), names);
    return a->entries.size() > max_entries || a->names.size() > names_cap ? XLZ_ERR_OUT_CAP : XLZ_OK;
}

extern "C" int xlz_7z_archive_folders(const xlz_7z_archive *a, xlz_7z_folder *folders, size_t max_folders)
{
    if (!a || (!folders && max_folders)) return XLZ_ERR_BAD_ARG;
    std::copy_n(a->folders.begin(), std::min(max_folders, a->folders.size()), folders);
    return a->folders.size() > max_folders ? XLZ_ERR_OUT_CAP : XLZ_OK;
}
