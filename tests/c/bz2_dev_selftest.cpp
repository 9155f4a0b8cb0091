// bz2_dev_selftest.cpp -- the lane scheme of lzma_amd/csrc/xlz_bz2_dev.h (phases A to D and the CRC) on the CPU, lane by
// lane, under the chain rule and the verdict of xlz_bz2.h: what the kernels of xlz_bz2.hip compute, without a GPU.
//   g++ -O1 -std=c++17 -pthread -I include tests/c/bz2_dev_selftest.cpp -o t
//   ./t --list LIST IN OUT RES    LIST: one line "in_len out_cap" per file, IN: the files back to back; RES gets one line
//                                 "status out_len in_consumed blocks streams" per file, OUT the bytes of the XLZ_OK files
//                                 back to back; stdout: "gave up N", the blocks whose walk stopped at a lane's share and
//                                 which the twin decoded instead.  Exit code 0 whenever every file was run.
//   ./t                           a built-in round trip of the CRC pieces
// Every candidate of a file -- on the chain or not -- runs phases A to C with guard bytes around its scratch; the guards
// and the bytes behind every window are compared afterwards (exit code 3).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../lzma_amd/csrc/xlz_bz2.h"

using namespace xlzbz2;

static constexpr size_t kGuard = 64;
static unsigned g_gave_up = 0; // blocks that the walk gave up (kStSlow): --list prints their number

static int run_file(const uint8_t *file, uint64_t len, uint64_t out_cap, std::vector<uint8_t> &out, xlz_bz2_result *res, WaveA &wa, WaveW &ww)
{
    // the image: at a multiple of 16, padded to one, 0xEE behind the file (the scheme must not look at it)
    std::vector<uint8_t> image_store(round16(len) + 32 + 16, 0xEE);
    uint8_t *image = image_store.data() + (16 - ((uintptr_t)image_store.data() & 15)) % 16;
    if (len) memcpy(image, file, len);
    std::vector<Magic> magics = scan(file, len);
    uint32_t level = len >= 4 && file[3] >= '1' && file[3] <= '9' ? file[3] - '0' : 9;
    struct C {
        DevCand c;
        uint64_t bit;
        DevState st;
        std::vector<uint8_t> scratch;
        uint8_t *base;
    };
    std::vector<C> cands;
    for (const Magic &m : magics) {
        if (m.end) {
            const uint64_t at = (m.bit + 80 + 7) >> 3;
            if (at + 4 <= len && file[at] == 'B' && file[at + 1] == 'Z' && file[at + 2] == 'h' && file[at + 3] >= '1' && file[at + 3] <= '9') level = file[at + 3] - '0';
            continue;
        }
        C c{};
        const uint64_t rel = (m.bit >> 3) & ~15ull;
        c.bit = m.bit;
        c.c.in_off = rel, c.c.in_len = (uint32_t)std::min<uint64_t>(len - rel, kMaxInput), c.c.start_bit = (uint32_t)(m.bit - 8 * rel);
        c.c.cap = level * kLevelBytes, c.c.scratch_off = 0;
        cands.push_back(std::move(c));
    }
    for (C &c : cands) {
        const size_t bytes = (size_t)scratch_bytes(c.c.cap);
        c.scratch.assign(bytes + 2 * kGuard + 16, 0xC3);
        c.base = c.scratch.data() + kGuard;
        c.base += (16 - ((uintptr_t)c.base & 15)) % 16;
        c.st = DevState{};
        c.st.status = -100;
        wave_symbols(wa, c.c, image, c.base, &c.st);
        wave_walk(ww, c.c, c.base, &c.st);
        g_gave_up += c.st.status == kStSlow;
        for (uint8_t *p = c.scratch.data(); p < c.base; p++)
            if (*p != 0xC3) return 3;
        for (uint8_t *p = c.base + bytes; p < c.scratch.data() + c.scratch.size(); p++)
            if (*p != 0xC3) return 3;
    }
    Chain ch;
    chain_open(ch, file, len, true);
    std::vector<size_t> block_cand;
    HostBlockBuffers redo;
    std::vector<std::vector<uint8_t>> redone;
    while (chain_step(ch)) {
        size_t k = 0;
        while (k < cands.size() && cands[k].bit != ch.bit) k++;
        if (k == cands.size()) return 4; // the chain saw a magic that the scan did not
        C &c = cands[k];
        if (c.c.cap != ch.level * kLevelBytes || c.st.status == kStSlow) { // as xlz_bz2.hip: decoded again by the twin
            redo.room(ch.level * kLevelBytes);
            BlockInfo bi;
            host_block(file, len, ch.bit, ch.level * kLevelBytes, redo.ll.data(), redo.tt.data(), redo.pre.data(), &bi);
            redone.resize(ch.blocks.size() + 1);
            if (bi.status == kStOk) redone.back().assign(redo.pre.begin(), redo.pre.begin() + bi.nblock);
            if (bi.status == kStOk) {
                std::vector<uint8_t> tmp(bi.out_len);
                host_expand(redone.back().data(), bi.nblock, tmp.data());
                if (host_crc(0, tmp.data(), tmp.size()) != bi.crc) bi.status = kStResult;
            }
            block_cand.push_back(k);
            chain_block(ch, bi.status, bi.end_bit, bi.nblock, bi.out_len, bi.crc);
            continue;
        }
        if (c.st.status == kStOk && c.st.calc_crc != c.st.crc) { // as xlz_bz2.hip: the block's CRC, known since phase C
            chain_block(ch, kStResult, 0, 0, 0, 0);
            break;
        }
        block_cand.push_back(k);
        chain_block(ch, c.st.status, 8 * c.c.in_off + c.st.end_bit, c.st.nblock, c.st.out_len, c.st.crc);
    }
    const uint64_t need = chain_need(ch);
    out.assign((size_t)out_cap + kGuard, 0xA5);
    if (need > out_cap) {
        *res = xlz_bz2_result{};
        res->status = XLZ_ERR_OUT_CAP, res->out_len = need;
    } else {
        std::vector<uint32_t> table(256), part(kLanes);
        for (size_t k = 0; k < ch.blocks.size(); k++) {
            const ChainBlock &b = ch.blocks[k];
            if (b.out_off + b.out_len > need) continue;
            uint8_t *dst = out.data() + b.out_off;
            if (k < redone.size() && !redone[k].empty())
                host_expand(redone[k].data(), b.nblock, dst);
            else
                wave_expand(cands[block_cand[k]].c, cands[block_cand[k]].base, cands[block_cand[k]].st, dst, b.out_len);
            // the CRC over the destination, folded, against the serial one and against what phase C formed without writing
            const uint32_t crc = wave_crc(table.data(), part.data(), dst, b.out_len);
            if (crc != host_crc(0, dst, b.out_len) || crc != b.stored_crc) return 5;
        }
        *res = verdict(ch, nullptr);
    }
    for (size_t i = (size_t)(need <= out_cap ? need : 0); i < out.size(); i++)
        if (out[i] != 0xA5) return 3;
    out.resize(res->status == XLZ_OK ? (size_t)res->out_len : 0);
    return 0;
}

static int list(const char *list_path, const char *in_path, const char *out_path, const char *res_path)
{
    FILE *lst = fopen(list_path, "r"), *in = fopen(in_path, "rb"), *out = fopen(out_path, "wb"), *res = fopen(res_path, "w");
    if (!lst || !in || !out || !res) return 2;
    std::unique_ptr<WaveA> wa(new WaveA);
    std::unique_ptr<WaveW> ww(new WaveW);
    unsigned long in_len, out_cap;
    int rc = 0;
    while (rc == 0 && fscanf(lst, "%lu %lu", &in_len, &out_cap) == 2) {
        std::vector<uint8_t> file(in_len), o;
        if (in_len && fread(file.data(), 1, in_len, in) != in_len) return 2;
        memset(wa.get(), 0x5A, sizeof(WaveA)), memset(ww.get(), 0x5A, sizeof(WaveW)); // (what another block left in LDS)
        xlz_bz2_result r = {};
        rc = run_file(file.data(), in_len, out_cap, o, &r, *wa, *ww);
        fprintf(res, "%d %llu %llu %u %u\n", r.status, (unsigned long long)r.out_len, (unsigned long long)r.in_consumed, r.blocks, r.streams);
        if (!o.empty()) fwrite(o.data(), 1, o.size(), out);
    }
    fclose(lst), fclose(in), fclose(out), fclose(res);
    printf("gave up %u\n", g_gave_up);
    return rc;
}

int main(int argc, char **argv)
{
    if (argc == 6 && !strcmp(argv[1], "--list")) return list(argv[2], argv[3], argv[4], argv[5]);
    // CRC-32/BZIP2 of "123456789" is 0xFC891918; folded over lanes it is the same at every length
    const char *check = "123456789";
    if (host_crc(0, (const uint8_t *)check, 9) != 0xFC891918u) return 1;
    std::vector<uint8_t> data(100000);
    uint32_t x = 12345;
    for (uint8_t &b : data) b = (uint8_t)((x = x * 1664525u + 1013904223u) >> 24);
    std::vector<uint32_t> table(256), part(kLanes);
    for (uint32_t len : {0u, 1u, 2u, 63u, 64u, 65u, 127u, 128u, 129u, 4095u, 4096u, 4097u, 100000u})
        if (wave_crc(table.data(), part.data(), data.data(), len) != host_crc(0, data.data(), len)) return 1;
    if (host_crc(host_crc(0, data.data(), 1000), data.data() + 1000, 5000) != host_crc(0, data.data(), 6000)) return 1;
    puts("ok");
    return 0;
}
