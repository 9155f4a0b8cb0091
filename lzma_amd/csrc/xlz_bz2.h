// xlz_bz2.h -- what a .bz2 file needs that needs no device: the stream header, the scan for the two 48-bit magics at
// every bit offset, the chain rule, the combined CRC, the verdict per file and the serial twin's file loop.  Plain C++
// over the standard library and xlz_bz2_dev.h's serial twin (tests/c/bz2_fuzz.cpp runs it without a GPU); host only, not
// part of the C ABI.  The block format is at the head of xlz_bz2_dev.h.
//
// THE SCAN.  A block opens with 0x314159265359 and a stream closes with 0x177245385090, at any bit offset.  Both are found
// without decoding: the two bytes behind the byte a magic begins in are fixed for each of the eight offsets, so ONE lookup
// in a table of 65536 bit masks per input byte says at which offsets a magic can begin there, and only those are compared
// in full.  One thread scans roughly 1 GiB in a second (an estimate from the loop's length, not a measurement); inputs
// above kScanPiece bytes are scanned in pieces by up to kScanThreads threads.  A hit is a CANDIDATE, nothing more: the 48
// bits also occur by chance (once in 2^48 offsets) and on purpose inside junk.
//
// THE CHAIN RULE.  A candidate belongs to the file iff it begins at the bit where the stream header or the previous chain
// block ended.  What follows a chain block is another block, or the end magic -- then the combined CRC, padding to a byte and
// either the end of the file or another "BZh?" stream --, or a defect.  Candidates off the chain are discarded.
//
// THE VERDICT is that of a serial reader which joins concatenated streams (Python's bz2.decompress is the yardstick):
//   - the FIRST defect in stream order decides; the input ending with no defect in front of it is XLZ_ERR_UNEXPECTED_EOF
//   - a stream of no block is valid and empty; an input of no byte is valid and empty, of no stream
//   - once one stream is complete, a following stream with a DEFECT (bad header, damaged block, wrong CRC) is ignored
//     together with everything behind it and the file is XLZ_OK: in_consumed, the end of the last good stream, shows it
//   - a following stream that is merely CUT is XLZ_ERR_UNEXPECTED_EOF
//   - a defect in the first stream is XLZ_ERR_RESULT (a randomised block: XLZ_ERR_UNSUPPORTED)
//   - a window smaller than what is kept is XLZ_ERR_OUT_CAP with out_len = that size
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/xlz.h"
#include "xlz_bz2_dev.h"

namespace xlzbz2 {

constexpr uint64_t kScanPiece = 4ull << 20;
constexpr unsigned kScanThreads = 16;

struct Magic {
    uint64_t bit; // where the 48 bits begin
    bool end;     // the end magic
};

inline uint64_t bits48(const uint8_t *in, uint64_t bit) // the 48 bits at `bit`; the caller has seen to bit + 48 <= 8 len
{
    const uint64_t at = bit >> 3;
    const uint32_t s = (uint32_t)(bit & 7);
    uint64_t v = 0;
    for (uint32_t k = 0; k < 6; k++) v = v << 8 | in[at + k];
    if (!s) return v;
    return ((v << s) | (in[at + 6] >> (8 - s))) & 0xFFFFFFFFFFFFull;
}

struct ScanTable {
    uint8_t block[65536], end[65536]; // bit s: bytes (i + 1, i + 2) allow the magic to begin at bit s of byte i
    ScanTable()
    {
        memset(block, 0, sizeof block), memset(end, 0, sizeof end);
        for (uint32_t s = 0; s < 8; s++) {
            block[(kBlockMagic >> (24 + s)) & 0xFFFF] |= (uint8_t)(1u << s);
            end[(kEndMagic >> (24 + s)) & 0xFFFF] |= (uint8_t)(1u << s);
        }
    }
};
inline const ScanTable &scan_table()
{
    static const ScanTable t;
    return t;
}
// the magics that begin in bytes [from, to) of in[0 .. len), in order
inline void scan_piece(const uint8_t *in, uint64_t len, uint64_t from, uint64_t to, std::vector<Magic> &out)
{
    const ScanTable &t = scan_table();
    for (uint64_t i = from; i < to && i + 6 <= len; i++) {
        const uint32_t key = (uint32_t)in[i + 1] << 8 | in[i + 2];
        const uint32_t mb = t.block[key], me = t.end[key];
        if (!(mb | me)) continue;
        for (uint32_t s = 0; s < 8; s++) {
            if (!((mb | me) >> s & 1) || 8 * i + s + 48 > 8 * len) continue;
            const uint64_t v = bits48(in, 8 * i + s);
            if (v == kBlockMagic)
                out.push_back(Magic{8 * i + s, false});
            else if (v == kEndMagic)
                out.push_back(Magic{8 * i + s, true});
        }
    }
}
inline std::vector<Magic> scan(const uint8_t *in, uint64_t len)
{
    const uint64_t pieces = (len + kScanPiece - 1) / kScanPiece;
    std::vector<Magic> all;
    if (pieces <= 1) {
        scan_piece(in, len, 0, len, all);
        return all;
    }
    std::vector<std::vector<Magic>> found(pieces);
    const unsigned n_threads = (unsigned)std::min<uint64_t>(pieces, kScanThreads);
    std::vector<std::thread> th;
    for (unsigned k = 0; k < n_threads; k++)
        th.emplace_back([&, k] {
            for (uint64_t p = k; p < pieces; p += n_threads) scan_piece(in, len, p * kScanPiece, std::min(len, (p + 1) * kScanPiece), found[p]);
        });
    for (std::thread &x : th) x.join();
    for (const std::vector<Magic> &f : found) all.insert(all.end(), f.begin(), f.end());
    return all;
}

// ---------------------------------------------------------------- the chain ----
struct ChainBlock {
    uint64_t bit;     // where its magic begins
    uint64_t out_off; // in the file's decoded bytes
    uint32_t out_len, stored_crc, stream, nblock;
};
struct ChainStream { // a complete one
    uint64_t end_byte, out_end;
    uint32_t blocks_end; // blocks of the file up to its end
};
enum ChainEvent { kRunning = 0, kClean, kDefect, kCut };
struct Chain {
    const uint8_t *in = nullptr;
    uint64_t len = 0;
    bool verify = true;
    uint64_t bit = 0; // where the next thing is expected
    bool in_stream = false;
    uint32_t level = 0, combined = 0;
    uint64_t out_len = 0;
    std::vector<ChainBlock> blocks;
    std::vector<ChainStream> streams;
    ChainEvent event = kRunning;
    int defect_status = XLZ_ERR_RESULT; // of a kDefect
};
inline void chain_open(Chain &c, const uint8_t *in, uint64_t len, bool verify)
{
    c = Chain{};
    c.in = in, c.len = len, c.verify = verify;
}
inline bool chain_byte(const Chain &c, uint64_t bit, uint32_t *v) // the eight bits at `bit`; false: the input ends in front of them
{
    if (bit + 8 > 8 * c.len) return false;
    const uint64_t at = bit >> 3;
    const uint32_t s = (uint32_t)(bit & 7);
    *v = s ? ((c.in[at] << s) | (c.in[at + 1] >> (8 - s))) & 255 : c.in[at];
    return true;
}
// Goes on until a block is needed -> true, c.bit is where its magic begins and the caller answers with chain_block();
// or until the file has ended -> false, c.event says how.
inline bool chain_step(Chain &c)
{
    while (c.event == kRunning) {
        uint32_t v = 0;
        if (!c.in_stream) {
            const uint64_t at = c.bit >> 3;
            if (at == c.len) {
                c.event = kClean;
                break;
            }
            static const char head[3] = {'B', 'Z', 'h'};
            for (uint32_t k = 0; k < 4 && c.event == kRunning; k++) {
                if (at + k >= c.len)
                    c.event = kCut;
                else if (k < 3 ? c.in[at + k] != (uint8_t)head[k] : (c.in[at + k] < '1' || c.in[at + k] > '9'))
                    c.event = kDefect;
            }
            if (c.event != kRunning) break;
            c.level = c.in[at + 3] - '0', c.combined = 0, c.in_stream = true, c.bit = 8 * (at + 4);
            continue;
        }
        if (!chain_byte(c, c.bit, &v)) {
            c.event = kCut;
            break;
        }
        const bool end = v == 0x17;
        if (!end && v != 0x31) {
            c.event = kDefect;
            break;
        }
        const uint64_t magic = end ? kEndMagic : kBlockMagic;
        for (uint32_t k = 1; k < 6 && c.event == kRunning; k++) {
            if (!chain_byte(c, c.bit + 8 * k, &v))
                c.event = kCut;
            else if (v != ((magic >> (8 * (5 - k))) & 255))
                c.event = kDefect;
        }
        if (c.event != kRunning) break;
        if (!end) return true;
        uint32_t stored = 0;
        for (uint32_t k = 0; k < 4 && c.event == kRunning; k++) {
            if (!chain_byte(c, c.bit + 48 + 8 * k, &v))
                c.event = kCut;
            else
                stored = stored << 8 | v;
        }
        if (c.event != kRunning) break;
        if (c.verify && stored != c.combined) {
            c.event = kDefect;
            break;
        }
        const uint64_t end_byte = (c.bit + 80 + 7) >> 3;
        c.streams.push_back(ChainStream{end_byte, c.out_len, (uint32_t)c.blocks.size()});
        c.in_stream = false, c.bit = 8 * end_byte;
    }
    return false;
}
// the answer to chain_step() == true: what the block at c.bit decoded to (end_bit: of the file)
inline void chain_block(Chain &c, int status, uint64_t end_bit, uint32_t nblock, uint32_t out_len, uint32_t stored_crc)
{
    if (status != kStOk) {
        c.event = status == kStEof ? kCut : kDefect;
        c.defect_status = status == kStUnsupported ? XLZ_ERR_UNSUPPORTED : XLZ_ERR_RESULT;
        return;
    }
    c.blocks.push_back(ChainBlock{c.bit, c.out_len, out_len, stored_crc, (uint32_t)c.streams.size(), nblock});
    c.out_len += out_len;
    c.combined = ((c.combined << 1) | (c.combined >> 31)) ^ stored_crc;
    c.bit = end_bit;
}

// What is kept of a file whose chain has ended, as far as the chain alone says (no block CRC compared yet): *streams
// complete streams are kept, -> the status
inline int chain_verdict(const Chain &c, size_t *streams)
{
    *streams = c.streams.size();
    if (c.event == kClean) return XLZ_OK;
    if (c.event == kCut) return XLZ_ERR_UNEXPECTED_EOF;
    return c.streams.empty() ? c.defect_status : (int)XLZ_OK; // a defect behind a complete stream: ignored with all behind it
}
inline xlz_bz2_result result_of(const Chain &c, int status, size_t streams)
{
    xlz_bz2_result r = {};
    r.status = status;
    if (status == XLZ_OK && streams) {
        const ChainStream &s = c.streams[streams - 1];
        r.out_len = s.out_end, r.in_consumed = s.end_byte, r.blocks = s.blocks_end, r.streams = (uint32_t)streams;
    }
    return r;
}
// The verdict with the blocks' CRCs formed (crc[k]: of block k; looked at up to the kept streams' blocks, with verify on):
// the first block whose CRC differs is a defect of its stream.
inline xlz_bz2_result verdict(const Chain &c, const uint32_t *crc)
{
    size_t streams = 0;
    int st = chain_verdict(c, &streams);
    const size_t kept_blocks = st == XLZ_OK && streams ? c.streams[streams - 1].blocks_end : (st == XLZ_OK ? 0 : c.blocks.size());
    for (size_t k = 0; c.verify && crc && k < kept_blocks && k < c.blocks.size(); k++)
        if (crc[k] != c.blocks[k].stored_crc) {
            streams = c.blocks[k].stream; // the complete streams in front of it
            st = streams ? (int)XLZ_OK : (int)XLZ_ERR_RESULT;
            break;
        }
    return result_of(c, st, streams);
}
// the bytes a window must hold for what the chain alone keeps
inline uint64_t chain_need(const Chain &c)
{
    size_t streams = 0;
    return chain_verdict(c, &streams) == XLZ_OK && streams ? c.streams[streams - 1].out_end : 0;
}

// ---------------------------------------------------------------- the serial twin's file loop ----
struct HostBlockBuffers {
    std::vector<uint8_t> ll, pre;
    std::vector<uint32_t> tt;
    void room(uint32_t cap)
    {
        if (ll.size() < cap) ll.resize(cap), pre.resize(cap), tt.resize(cap);
    }
};
inline int decode_host(const uint8_t *in, uint64_t len, uint8_t *out, uint64_t out_cap, bool verify, xlz_bz2_result *r)
{
    Chain c;
    chain_open(c, in, len, verify);
    HostBlockBuffers buf;
    std::vector<uint32_t> crc;
    while (chain_step(c)) {
        const uint32_t cap = c.level * kLevelBytes;
        buf.room(cap);
        BlockInfo bi;
        host_block(in, len, c.bit, cap, buf.ll.data(), buf.tt.data(), buf.pre.data(), &bi);
        const uint64_t at = c.out_len;
        if (bi.status == kStOk) {
            if (at + bi.out_len <= out_cap) {
                host_expand(buf.pre.data(), bi.nblock, out + at);
                crc.push_back(verify ? host_crc(0, out + at, bi.out_len) : bi.crc);
            } else { // measured only: the CRC is that of a scratch copy
                std::vector<uint8_t> tmp(bi.out_len);
                host_expand(buf.pre.data(), bi.nblock, tmp.data());
                crc.push_back(verify ? host_crc(0, tmp.data(), bi.out_len) : bi.crc);
            }
            // (a serial reader compares the block's CRC before it reads on)
            if (verify && crc.back() != bi.crc) {
                chain_block(c, kStResult, 0, 0, 0, 0);
                break;
            }
        }
        chain_block(c, bi.status, bi.end_bit, bi.nblock, bi.out_len, bi.crc);
    }
    *r = verdict(c, nullptr);
    if (r->status == XLZ_OK && r->out_len > out_cap) {
        const uint64_t need = r->out_len;
        *r = xlz_bz2_result{};
        r->status = XLZ_ERR_OUT_CAP, r->out_len = need;
    }
    return XLZ_OK;
}

inline int probe(const uint8_t *in, uint64_t len, xlz_bz2_info *out)
{
    *out = xlz_bz2_info{};
    if (len < 4) return XLZ_ERR_UNEXPECTED_EOF;
    if (in[0] != 'B' || in[1] != 'Z' || in[2] != 'h' || in[3] < '1' || in[3] > '9') return XLZ_ERR_RESULT;
    out->level = in[3] - '0';
    for (const Magic &m : scan(in, len)) (m.end ? out->streams : out->candidates)++;
    out->size_hint = out->candidates * (uint64_t)out->level * kLevelBytes;
    out->size_bound = out->candidates * (uint64_t)kMaxBlock / 5 * 259 + out->candidates * 259;
    return XLZ_OK;
}

} // namespace xlzbz2
