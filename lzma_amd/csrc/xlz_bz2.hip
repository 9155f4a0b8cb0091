// xlz_bz2.hip -- .bz2 files as ONE batch (xlz_bz2_probe / xlz_bz2_decode_host / xlz_bz2_decode_many /
// xlz_bz2_decode_many_device).  The block decoder's scheme is xlz_bz2_dev.h (it also runs on the
// CPU: tests/c/bz2_dev_selftest.cpp); what needs no device -- the scan, the chain rule, the verdict -- is xlz_bz2.h.  This
// file holds the four kernels, their launches and the rounds.  The reference has nothing of the kind.
//
// Every kernel is a grid of one-wave workgroups that stays: workgroup g takes items g, g + grid, ...  No scratch memory,
// no inline assembly; the only atomics are the LDS adds of the histogram.
//   bz2_symbols_kernel   phase A, about 37 KiB of LDS: four workgroups per CU
//   bz2_walk_kernel      phases B and C and the measuring of the run-length code, about 16 KiB of LDS: eight per CU
//   bz2_expand_kernel    phase D, no LDS
//   bz2_crc_kernel       the block CRCs over the destination, 1.25 KiB of LDS
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/xlz.h"
#include "xlz_bz2.h"
#include "xlz_check_host.h"
#include "xlz_windows.h"

using namespace xlzbz2;

static_assert(sizeof(xlz_bz2_info) == 40 && sizeof(xlz_bz2_file) == 32 && sizeof(xlz_bz2_result) == 32 && sizeof(xlz_bz2_stats) == 112,
              "include/xlz.h: the structs hold no implicit padding");
static_assert(sizeof(DevCand) == 32 && sizeof(DevState) == 32 && sizeof(DevChunk) == 16 && sizeof(DevPlace) == 16, "xlz_bz2_dev.h: the device tables");
static_assert(kStOk == XLZ_OK && kStResult == XLZ_ERR_RESULT && kStEof == XLZ_ERR_UNEXPECTED_EOF && kStUnsupported == XLZ_ERR_UNSUPPORTED,
              "xlz_bz2_dev.h names the statuses of include/xlz.h");

namespace xlz {

__global__ __launch_bounds__(64) void bz2_symbols_kernel(const DevCand *__restrict__ cands, uint32_t n, const uint8_t *__restrict__ image,
                                                         uint8_t *scratch, DevState *states)
{
    __shared__ WaveA w;
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const DevCand c = cands[i];
        wave_symbols(w, c, image, scratch, states + i);
        __syncthreads();
    }
}
__global__ __launch_bounds__(64) void bz2_walk_kernel(const DevCand *__restrict__ cands, uint32_t n, uint8_t *scratch, DevState *states)
{
    __shared__ WaveW w;
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const DevCand c = cands[i];
        wave_walk(w, c, scratch, states + i);
        __syncthreads();
    }
}
__global__ __launch_bounds__(64) void bz2_expand_kernel(const DevPlace *__restrict__ places, uint32_t n, const DevCand *__restrict__ cands,
                                                        const DevState *__restrict__ states, uint8_t *scratch, uint8_t *dst)
{
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const DevPlace p = places[i];
        wave_expand(cands[p.cand], scratch, states[p.cand], dst + p.dst_off, p.out_len);
    }
}
__global__ __launch_bounds__(64) void bz2_crc_kernel(const DevPlace *__restrict__ places, uint32_t n, const uint8_t *dst, uint32_t *digests)
{
    __shared__ uint32_t table[256], part[kLanes];
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const DevPlace p = places[i];
        const uint32_t crc = wave_crc(table, part, dst + p.dst_off, p.out_len);
        if (threadIdx.x == 0) digests[i] = crc;
        __syncthreads();
    }
}

} // namespace xlz

extern "C" int xlz_bz2_probe(const uint8_t *in, size_t in_len, xlz_bz2_info *out)
{
    if (!out || (!in && in_len)) return XLZ_ERR_BAD_ARG;
    return probe(in, in_len, out);
}
extern "C" int xlz_bz2_decode_host(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap, int verify, xlz_bz2_result *r)
{
    if (!r) return XLZ_ERR_BAD_ARG;
    *r = xlz_bz2_result{};
    if ((!in && in_len) || (!out && out_cap)) return XLZ_ERR_BAD_ARG;
    return decode_host(in, in_len, out, out_cap, verify != 0, r);
}
extern "C" uint32_t xlz_crc32_bzip2_host(uint32_t crc, const uint8_t *p, size_t n) { return p || !n ? host_crc(crc, p, n) : crc; }

namespace {

constexpr uint64_t kDefaultScratch = 6ull << 30; // include/xlz.h: xlz_ctx_set_bz2_scratch
constexpr uint32_t kSymbolsWgPerCu = 4, kWalkWgPerCu = 8, kExpandWgPerCu = 16;

struct Cand {
    size_t file;
    uint64_t bit; // of the file
    uint32_t cap;
    bool used;
};
struct HostBlock { // a block decoded on a host thread: what it expands to, and bi.calc_crc
    BlockInfo bi;
    std::vector<uint8_t> out;
};
void host_decode(const uint8_t *in, uint64_t len, uint64_t bit, uint32_t cap, bool verify, HostBlockBuffers &buf, HostBlock &hb)
{
    buf.room(cap);
    host_block(in, len, bit, cap, buf.ll.data(), buf.tt.data(), buf.pre.data(), &hb.bi);
    hb.bi.calc_crc = hb.bi.crc;
    if (hb.bi.status != kStOk) return;
    hb.out.resize(hb.bi.out_len);
    host_expand(buf.pre.data(), hb.bi.nblock, hb.out.data());
    if (verify) hb.bi.calc_crc = host_crc(0, hb.out.data(), hb.out.size());
}
struct FileRun {
    Chain chain;
    size_t c0 = 0, c1 = 0;            // its candidates
    std::vector<size_t> block_cand;   // chain block k's candidate
    size_t placed = 0;                // chain blocks looked at for placing
    int first_round = -1;             // of its first chain block
    bool done = false;
};

uint32_t grid_of(size_t n, int num_cus, uint32_t per_cu)
{
    const uint64_t cap = (uint64_t)(num_cus > 0 ? num_cus : 1) * per_cu;
    return (uint32_t)std::min<uint64_t>(n, cap);
}

struct Timer { // the time of what was queued between begin() and end(), read behind a wait
    hipEvent_t a = nullptr, b = nullptr;
    bool ok = true;
    Timer() { ok = hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess; }
    ~Timer()
    {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
    void begin(hipStream_t s) { ok = ok && hipEventRecord(a, s) == hipSuccess; }
    void end(hipStream_t s) { ok = ok && hipEventRecord(b, s) == hipSuccess; }
    double ms()
    {
        float t = 0;
        return ok && hipEventElapsedTime(&t, a, b) == hipSuccess ? t : 0.0;
    }
};

// dst: the host form (d_dst == NULL) -- every window lies in a staging block of the context's pool, back to back in the
// order of the files, and comes down from there in one copy
int bz2_decode_many(xlz_ctx *ctx, const xlz_bz2_file *files, size_t n, uint8_t *dst, void *d_dst, bool device, size_t dst_cap, int verify,
                    xlz_bz2_result *results)
{
    // ---- the arguments: all of them before the context is used, but the last
    if (!ctx) return XLZ_ERR_BAD_ARG;
    if (!n) return XLZ_OK;
    if (!files || !results || (dst_cap && !(device ? d_dst != nullptr : dst != nullptr))) return XLZ_ERR_BAD_ARG;
    std::vector<xlzwin::Window> win;
    for (size_t i = 0; i < n; i++) {
        if (!files[i].in && files[i].in_len) return XLZ_ERR_BAD_ARG;
        win.emplace_back(files[i].dst_off, files[i].dst_cap);
    }
    if (!xlzwin::disjoint_within(std::move(win), dst_cap)) return XLZ_ERR_BAD_ARG;
    if (device && dst_cap) {
        const int ok = xlz_internal_device_dst_ok(ctx, d_dst, dst_cap);
        if (ok != XLZ_OK) return ok;
    }
    Bz2Env env;
    int st = xlz_internal_bz2_env(ctx, &env);
    if (st != XLZ_OK) return st;
    const bool on_host = env.mode == 2;
    const uint64_t budget = env.scratch ? env.scratch : kDefaultScratch;
    hipStream_t stream = static_cast<hipStream_t>(env.stream);
    // ---- the windows: the caller's, or the staging block's
    HostStaging staging(ctx);
    std::vector<uint64_t> base(n);
    for (size_t i = 0; i < n; i++) base[i] = device ? files[i].dst_off : staging.add(files[i].dst_cap);
    st = staging.acquire();
    uint8_t *d = static_cast<uint8_t *>(device ? d_dst : staging.d_dst());
    // ---- the candidates of all files, and where the files lie in the image
    xlz_bz2_stats bs = {};
    bs.files = n;
    std::vector<FileRun> run(n);
    std::vector<Cand> cands;
    std::vector<uint64_t> image_off(n);
    uint64_t image_len = 0;
    for (size_t i = 0; i < n; i++) {
        const uint8_t *in = files[i].in;
        const uint64_t len = files[i].in_len;
        chain_open(run[i].chain, in, len, verify != 0);
        image_off[i] = image_len;
        image_len += round16(len) + kInputAlign;
        run[i].c0 = cands.size();
        uint32_t level = len >= 4 && in[3] >= '1' && in[3] <= '9' ? in[3] - '0' : 9;
        for (const Magic &m : scan(in, len)) {
            if (!m.end) {
                cands.push_back(Cand{i, m.bit, level * kLevelBytes, false});
                continue;
            }
            // the level of the stream that may begin behind this end (the chain checks it: a block whose candidate was
            // given another stream's size is decoded again, on the host)
            const uint64_t at = (m.bit + 80 + 7) >> 3;
            if (at + 4 <= len && in[at] == 'B' && in[at + 1] == 'Z' && in[at + 2] == 'h' && in[at + 3] >= '1' && in[at + 3] <= '9') level = in[at + 3] - '0';
        }
        run[i].c1 = cands.size();
    }
    bs.candidates = cands.size();
    // ---- the device's tables: | candidates, to a multiple of 256 | image |, ONE transfer
    const size_t nc = cands.size();
    const size_t tab_bytes = (nc * sizeof(DevCand) + 255) / 256 * 256;
    std::vector<DevCand> tab(nc);
    std::vector<DevState> states(nc);
    std::vector<HostBlock> host_blocks; // on_host: of the round's candidates
    void *d_in = nullptr, *d_scratch = nullptr, *d_small = nullptr;
    struct Blocks { // back to the pool whatever happens
        xlz_ctx *ctx;
        void **p[3];
        ~Blocks()
        {
            for (void **x : p) xlz_internal_device_block_release(ctx, *x);
        }
    } blocks{ctx, {&d_in, &d_scratch, &d_small}};
    // rounds: candidates in order while their scratch fits the budget
    std::vector<size_t> round_end;
    uint64_t max_round = 0;
    // ... and while the symbols kernel, whose workgroups take candidates in turn, stays below the launch-length cap by the
    // measured rate (xlz_bz2_dev.h): 256 CUs x 4 workgroups x 0.5 s are 2844 level-9 blocks
    const double time_budget = (double)(env.num_cus > 0 ? env.num_cus : 1) * kSymbolsWgPerCu * kLaunchCapNs;
    for (size_t k = 0; k < nc;) {
        uint64_t sum = 0;
        double ns = 0;
        size_t e = k;
        for (; e < nc && e - k < 0x7FFFFFFFull; e++) {
            const uint64_t need = scratch_bytes(cands[e].cap);
            const double est = cands[e].cap * kSymbolNs;
            if (e > k && (sum + need > budget || ns + est > time_budget)) break;
            tab[e].scratch_off = sum;
            sum += need, ns += est;
        }
        max_round = std::max(max_round, sum);
        round_end.push_back(e);
        k = e;
    }
    for (size_t k = 0; k < nc; k++) {
        const Cand &c = cands[k];
        const uint64_t rel = (c.bit >> 3) & ~(uint64_t)(kInputAlign - 1);
        tab[k].in_off = image_off[c.file] + rel;
        tab[k].in_len = (uint32_t)std::min<uint64_t>(files[c.file].in_len - rel, kMaxInput);
        tab[k].start_bit = (uint32_t)(c.bit - 8 * rel);
        tab[k].cap = c.cap, tab[k].reserved = 0;
    }
    size_t max_places = 0;
    for (size_t r = 0, k = 0; r < round_end.size(); k = round_end[r++]) max_places = std::max(max_places, round_end[r] - k);
    const size_t small_bytes = max_places * (sizeof(DevState) + sizeof(DevPlace) + sizeof(uint32_t));
    if (st == XLZ_OK && nc && !on_host) {
        std::vector<uint8_t> up(tab_bytes + image_len, 0);
        memcpy(up.data(), tab.data(), nc * sizeof(DevCand));
        xlzpost::parallel_for(n, xlzpost::host_thread_cap(8), [&](size_t i) {
            if (files[i].in_len) memcpy(up.data() + tab_bytes + image_off[i], files[i].in, (size_t)files[i].in_len);
        });
        st = xlz_internal_device_block(ctx, up.size(), &d_in);
        if (st == XLZ_OK) st = xlz_internal_device_block(ctx, (size_t)max_round, &d_scratch);
        if (st == XLZ_OK) st = xlz_internal_device_block(ctx, small_bytes, &d_small);
        if (st == XLZ_OK && (((uintptr_t)d_in | (uintptr_t)d_scratch) & 15)) st = XLZ_ERR_DEVICE;
        if (st == XLZ_OK) {
            xlz_internal_ctx_lock(ctx);
            if (hipSetDevice(env.device) != hipSuccess || hipMemcpyAsync(d_in, up.data(), up.size(), hipMemcpyHostToDevice, stream) != hipSuccess ||
                hipStreamSynchronize(stream) != hipSuccess)
                st = XLZ_ERR_DEVICE;
            xlz_internal_ctx_unlock(ctx);
            bs.uploads++;
        }
    }
    const DevCand *d_cands = static_cast<const DevCand *>(d_in);
    const uint8_t *d_image = static_cast<const uint8_t *>(d_in) + tab_bytes;
    DevState *d_states = static_cast<DevState *>(d_small);
    DevPlace *d_places = reinterpret_cast<DevPlace *>(static_cast<uint8_t *>(d_small) + max_places * sizeof(DevState));
    uint32_t *d_digests = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(d_small) + max_places * (sizeof(DevState) + sizeof(DevPlace)));
    Timer ta, tw, te, tc;
    HostBlockBuffers redo; // a chain block whose candidate was given another stream's size
    auto cand_base_bit = [&](size_t k) { return 8 * (tab[k].in_off - image_off[cands[k].file]); };
    // ---- the rounds.  Without a candidate there is still one turn: the chains of files of no block end in it.
    for (size_t r = 0, k0 = 0; st == XLZ_OK && (r < round_end.size() || (r == 0 && !nc)); r++) {
        const size_t k1 = nc ? round_end[r] : 0, cnt = k1 - k0;
        // -- phases A to C of candidates [k0, k1)
        if (cnt && on_host) {
            host_blocks.assign(cnt, HostBlock{});
            xlzpost::parallel_for(cnt, xlzpost::host_thread_cap(16), [&](size_t q) {
                const Cand &c = cands[k0 + q];
                HostBlockBuffers buf;
                HostBlock &hb = host_blocks[q];
                host_decode(files[c.file].in, files[c.file].in_len, c.bit, c.cap, verify != 0, buf, hb);
                DevState &s = states[k0 + q];
                s = DevState{};
                s.status = hb.bi.status, s.nblock = hb.bi.nblock, s.orig = hb.bi.orig, s.crc = hb.bi.crc, s.out_len = hb.bi.out_len;
                s.calc_crc = hb.bi.calc_crc;
                s.end_bit = hb.bi.end_bit - cand_base_bit(k0 + q);
            });
        } else if (cnt) {
            xlz_internal_ctx_lock(ctx);
            bool ok = hipSetDevice(env.device) == hipSuccess;
            ta.begin(stream);
            hipLaunchKernelGGL(xlz::bz2_symbols_kernel, dim3(grid_of(cnt, env.num_cus, kSymbolsWgPerCu)), dim3(kLanes), 0, stream, d_cands + k0,
                               (uint32_t)cnt, d_image, static_cast<uint8_t *>(d_scratch), d_states);
            ok = ok && hipGetLastError() == hipSuccess;
            ta.end(stream);
            tw.begin(stream);
            hipLaunchKernelGGL(xlz::bz2_walk_kernel, dim3(grid_of(cnt, env.num_cus, kWalkWgPerCu)), dim3(kLanes), 0, stream, d_cands + k0, (uint32_t)cnt,
                               static_cast<uint8_t *>(d_scratch), d_states);
            ok = ok && hipGetLastError() == hipSuccess;
            tw.end(stream);
            ok = ok && hipMemcpyAsync(states.data() + k0, d_states, cnt * sizeof(DevState), hipMemcpyDeviceToHost, stream) == hipSuccess;
            ok = hipStreamSynchronize(stream) == hipSuccess && ok;
            xlz_internal_ctx_unlock(ctx);
            if (!ok) {
                st = XLZ_ERR_DEVICE;
                break;
            }
            bs.symbols_ms += ta.ms(), bs.walk_ms += tw.ms();
        }
        bs.rounds += cnt != 0;
        // -- the chains, as far as this round's candidates carry them
        struct HostPlace {
            size_t file, block;
            std::vector<uint8_t> out; // of a block decoded again
            const HostBlock *hb;
            const std::vector<uint8_t> &bytes() const { return hb ? hb->out : out; }
        };
        std::vector<DevPlace> places;
        std::vector<std::pair<size_t, size_t>> place_owner; // (file, chain block) of places[q]
        std::vector<HostPlace> host_places;
        for (size_t i = 0; i < n; i++) {
            FileRun &f = run[i];
            if (f.done) continue;
            Chain &ch = f.chain;
            bool waits = false;
            const size_t po0 = place_owner.size(), hp0 = host_places.size();
            while (chain_step(ch)) {
                size_t lo = f.c0, hi = f.c1;
                while (lo < hi) {
                    const size_t mid = (lo + hi) / 2;
                    if (cands[mid].bit < ch.bit) lo = mid + 1; else hi = mid;
                }
                if (lo >= f.c1 || cands[lo].bit != ch.bit) { // (cannot be: the chain saw the magic the scan looks for)
                    chain_block(ch, kStResult, 0, 0, 0, 0);
                    break;
                }
                if (lo >= k1) {
                    waits = true;
                    break;
                }
                cands[lo].used = true;
                if (f.first_round < 0) f.first_round = (int)r;
                const uint32_t want_cap = ch.level * kLevelBytes;
                if (cands[lo].cap != want_cap || states[lo].status == kStSlow) { // (or the walk gave it up: xlz_bz2_dev.h, kWalkShare)
                    HostBlock hb;
                    host_decode(files[i].in, files[i].in_len, ch.bit, want_cap, verify != 0, redo, hb);
                    const BlockInfo &bi = hb.bi;
                    const bool sound = bi.status == kStOk && bi.calc_crc == bi.crc;
                    if (sound) host_places.push_back(HostPlace{i, ch.blocks.size(), std::move(hb.out), nullptr});
                    f.block_cand.push_back(lo);
                    chain_block(ch, bi.status == kStOk && !sound ? kStResult : bi.status, bi.end_bit, bi.nblock, bi.out_len, bi.crc);
                    continue;
                }
                const DevState &s = states[lo];
                if (s.status == kStOk && verify && s.calc_crc != s.crc) { // (a serial reader compares a block's CRC before it reads on)
                    chain_block(ch, kStResult, 0, 0, 0, 0);
                    break;
                }
                if (s.status == kStOk) {
                    if (on_host)
                        host_places.push_back(HostPlace{i, ch.blocks.size(), {}, &host_blocks[lo - k0]});
                    else
                        place_owner.emplace_back(i, ch.blocks.size());
                }
                f.block_cand.push_back(lo);
                chain_block(ch, s.status, cand_base_bit(lo) + s.end_bit, s.nblock, s.out_len, s.crc);
            }
            f.done = !waits;
            // which of the new chain blocks are written: of a file that began and ended in this round, what the chain keeps
            // -- if the window holds that, else nothing --; of a file that spans rounds, every block that lies inside the window
            const uint64_t room = files[i].dst_cap, need = f.done ? chain_need(ch) : 0;
            const uint64_t limit = f.done && (f.first_round < 0 || f.first_round == (int)r) ? (need <= room ? need : 0) : room;
            auto fits = [&](size_t k) { return ch.blocks[k].out_off + ch.blocks[k].out_len <= limit; };
            size_t keep = po0;
            for (size_t q = po0; q < place_owner.size(); q++) {
                const size_t k = place_owner[q].second;
                if (!fits(k)) continue;
                places.push_back(DevPlace{(uint32_t)(f.block_cand[k] - k0), ch.blocks[k].out_len, base[i] + ch.blocks[k].out_off});
                place_owner[keep++] = place_owner[q];
            }
            place_owner.resize(keep);
            keep = hp0;
            for (size_t q = hp0; q < host_places.size(); q++)
                if (fits(host_places[q].block)) {
                    if (keep != q) host_places[keep] = std::move(host_places[q]);
                    keep++;
                }
            host_places.resize(keep);
            f.placed = ch.blocks.size();
        }
        // -- phase D and the CRCs of the device's blocks
        if (!places.empty()) {
            std::vector<uint32_t> dig(places.size());
            xlz_internal_ctx_lock(ctx);
            bool ok = hipSetDevice(env.device) == hipSuccess;
            ok = ok && hipMemcpyAsync(d_places, places.data(), places.size() * sizeof(DevPlace), hipMemcpyHostToDevice, stream) == hipSuccess;
            te.begin(stream);
            hipLaunchKernelGGL(xlz::bz2_expand_kernel, dim3(grid_of(places.size(), env.num_cus, kExpandWgPerCu)), dim3(kLanes), 0, stream, d_places,
                               (uint32_t)places.size(), d_cands + k0, d_states, static_cast<uint8_t *>(d_scratch), d);
            ok = ok && hipGetLastError() == hipSuccess;
            te.end(stream);
            if (verify) {
                tc.begin(stream);
                hipLaunchKernelGGL(xlz::bz2_crc_kernel, dim3(grid_of(places.size(), env.num_cus, kExpandWgPerCu)), dim3(kLanes), 0, stream, d_places,
                                   (uint32_t)places.size(), d, d_digests);
                ok = ok && hipGetLastError() == hipSuccess;
                tc.end(stream);
                ok = ok && hipMemcpyAsync(dig.data(), d_digests, dig.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream) == hipSuccess;
            }
            ok = hipStreamSynchronize(stream) == hipSuccess && ok;
            xlz_internal_ctx_unlock(ctx);
            if (!ok) {
                st = XLZ_ERR_DEVICE;
                break;
            }
            bs.expand_ms += te.ms();
            if (verify) bs.crc_ms += tc.ms();
            for (size_t q = 0; q < places.size(); q++) {
                // (what phase D wrote is what phase C measured: else the device has failed, not the file)
                if (verify && dig[q] != states[k0 + places[q].cand].calc_crc) st = XLZ_ERR_DEVICE;
                bs.device_blocks++, bs.device_bytes += places[q].out_len;
            }
            if (st != XLZ_OK) break;
        }
        // -- the host's blocks: uploaded
        if (!host_places.empty()) {
            xlz_internal_ctx_lock(ctx);
            bool ok = hipSetDevice(env.device) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
            for (size_t q = 0; q < host_places.size() && ok; q++) {
                const HostPlace &p = host_places[q];
                const ChainBlock &b = run[p.file].chain.blocks[p.block];
                ok = hipMemcpy(d + base[p.file] + b.out_off, p.bytes().data(), p.bytes().size(), hipMemcpyHostToDevice) == hipSuccess;
                bs.host_blocks++, bs.host_bytes += b.out_len;
            }
            xlz_internal_ctx_unlock(ctx);
            if (!ok) {
                st = XLZ_ERR_DEVICE;
                break;
            }
        }
        k0 = k1;
    }
    // ---- the verdicts, and in the host form ONE copy of the staging block, the good files scattered
    std::vector<xlz_bz2_result> v(n);
    for (size_t i = 0; i < n && st == XLZ_OK; i++) {
        const Chain &ch = run[i].chain;
        const uint64_t need = chain_need(ch);
        if (need > files[i].dst_cap) {
            v[i] = xlz_bz2_result{};
            v[i].status = XLZ_ERR_OUT_CAP, v[i].out_len = need;
        } else {
            v[i] = verdict(ch, nullptr);
        }
        bs.chain_blocks += ch.blocks.size();
    }
    for (const Cand &c : cands) bs.discarded_blocks += !c.used;
    if (st == XLZ_OK && staging.d_dst()) {
        std::vector<HostStaging::Piece> good;
        for (size_t i = 0; i < n; i++)
            if (v[i].status == XLZ_OK && v[i].out_len) good.push_back({base[i], files[i].dst_off, v[i].out_len});
        st = staging.download(dst, good);
    }
    for (size_t i = 0; i < n; i++) {
        if (st != XLZ_OK) {
            v[i] = xlz_bz2_result{};
            v[i].status = st;
        }
        results[i] = v[i];
        bs.failed_files += results[i].status != XLZ_OK;
    }
    xlz_internal_bz2_stats_set(ctx, bs);
    return st;
}

} // namespace

extern "C" int xlz_bz2_decode_many_device(xlz_ctx *ctx, const xlz_bz2_file *files, size_t n, void *d_dst, size_t dst_cap, int verify,
                                          xlz_bz2_result *results)
{
    return bz2_decode_many(ctx, files, n, nullptr, d_dst, true, dst_cap, verify, results);
}
extern "C" int xlz_bz2_decode_many(xlz_ctx *ctx, const xlz_bz2_file *files, size_t n, uint8_t *dst, size_t dst_cap, int verify, xlz_bz2_result *results)
{
    return bz2_decode_many(ctx, files, n, dst, nullptr, false, dst_cap, verify, results);
}
