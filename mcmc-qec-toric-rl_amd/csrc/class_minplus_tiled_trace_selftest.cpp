// Stand-alone check of class_minplus_tiled_trace.hpp for the sanitizers (make minplus_tiled_trace_asan: -fsanitize=address,undefined): the trace plans
// of the small shapes under several widths of state vector and tile -- nothing held, holds forced by a narrow hbm_width --, their refusals under this
// entry point's names and the cap on one pair's decisions; the twins minplus_tiled_trace_host and ..._site_host over POISONED buffers of their exact
// size, against minplus_trace_host where the cut plans have the same stream; and a host walk of the DEVICE layout: the sweep run segment by segment
// and tile by tile in the tile's own coordinates (the device ops), every FORGET's decisions stored where the kernels store them -- D[off[fi] + x *
// words_per_tile + (h >> 6)], a whole word per 64 half-indices, over a dirty D of exactly words_per_pair words -- and read back through forget_tile
// from the global f, which must give the twin's chains byte for byte.  Exit status 0: all held.
#include "class_minplus_tiled_trace.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

using namespace qecmc;

namespace {

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t draw()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

// buffers of exactly n elements on the heap, so that one element too far is seen
template <class T> std::unique_ptr<T[]> exact(size_t n, int fill)
{
    std::unique_ptr<T[]> p(new T[n ? n : 1]);
    std::memset(p.get(), fill, (n ? n : 1) * sizeof(T));
    return p;
}

// One pair in the device's layout.  A: 2^state_bits entries, D: words_per_pair words, both dirty; rep: the representative under h*; cost(q, idx).
// The segments in order; within a segment every live tile alone: gather, the segment's device ops over a dirty tile, write back.
template <class Cost> void device_layout_trace(const minplus::TiledTracePlan &ttp, const uint32_t *rep, Cost cost, uint64_t *A, uint64_t *D)
{
    const sweep::TiledPlan &tp = ttp.tiled;
    const uint32_t entries = 1u << tp.tile_width;
    for (size_t s = 0; s < tp.segments.size(); ++s) {
        const sweep::Segment &sg = tp.segments[s];
        const uint32_t fixed_live = sg.live & ~sg.tile, local_in = sweep::bits_extract(sg.live_in, sg.tile), local_out = sweep::bits_extract(sg.live_out, sg.tile);
        for (uint32_t x = 0; x < sg.n_tiles; ++x) {
            const uint32_t base = sweep::bits_deposit(x, fixed_live);
            auto lds = exact<uint64_t>(entries, 0xA5);
            if (s == 0) lds[0] = 1ull;
            else
                for (uint32_t l = 0; l < entries; ++l)
                    if (!(l & ~local_in)) lds[l] = A[base + sweep::bits_deposit(l, sg.tile)];
            uint32_t fi = ttp.seg_forget[s];
            for (uint32_t o = sg.op_first; o < sg.op_first + sg.op_count; ++o) {
                const uint32_t *op = &tp.dev_ops[(size_t)o * sweep::kTiledDevOpWords];
                const uint32_t kind = op[0] & 15u, slot = (op[0] >> 4) & 15u, top = (op[0] >> 8) & 31u, mask = op[1], bit = 1u << slot;
                if (kind == sweep::kClose) {
                    const uint32_t q = op[3];
                    uint32_t cq = sweep::pauli_to_xz((rep[q >> 4] >> ((q & 15u) * 2u)) & 3u);
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t pr = (op[4] >> (8 * j)) & 0xFFu;
                        if ((base >> (pr & 31u)) & 1u) cq ^= pr >> 5;
                    }
                    for (uint32_t l = 0; l < (1u << top); ++l) {
                        if (l & ~mask) continue;
                        uint32_t idx = cq;
                        for (int j = 0; j < 4; ++j) {
                            const uint32_t pr = (op[2] >> (8 * j)) & 0xFFu;
                            if ((l >> (pr & 15u)) & 1u) idx ^= pr >> 4;
                        }
                        lds[l] += (uint64_t)cost(q, idx) << minplus::kCountBits;
                    }
                } else if (kind == sweep::kIntro) {
                    for (uint32_t h = 0; h < (1u << (top - 1u)); ++h) {
                        const uint32_t f = sweep::insert_zero(h, slot);
                        if (!(f & ~mask)) lds[f | bit] = lds[f];
                    }
                } else {
                    const uint32_t *ft = &ttp.forget_tile[(size_t)fi * minplus::kForgetTileWords];
                    uint64_t *words = D + ft[3] + (size_t)x * (size_t)ttp.words_per_tile;
                    for (uint32_t h0 = 0; h0 < (1u << (top - 1u)); h0 += 64u) {      // a wave's ballot: one whole word, dead and absent lanes 0
                        uint64_t word = 0;
                        for (uint32_t lane = 0; lane < 64u; ++lane) {
                            const uint32_t h = h0 + lane, f = sweep::insert_zero(h, slot);
                            if (h >= (1u << (top - 1u)) || (f & ~mask)) continue;
                            const uint64_t off = lds[f], on = lds[f | bit];
                            if ((on >> minplus::kCountBits) < (off >> minplus::kCountBits)) word |= 1ull << lane;
                            lds[f] = minplus::mp_combine(off, on);
                        }
                        words[h0 >> 6] = word;
                    }
                    ++fi;
                }
            }
            if (s + 1 != tp.segments.size())
                for (uint32_t l = 0; l < entries; ++l)
                    if (!(l & ~local_out)) A[base + sweep::bits_deposit(l, sg.tile)] = lds[l];
        }
    }
}

// the walk as the device does it: the bit of (fi, f) through forget_tile
uint32_t device_layout_walk(const minplus::TiledTracePlan &ttp, const uint64_t *D, uint32_t *chain)
{
    const sweep::TiledPlan &tp = ttp.tiled;
    uint32_t f = 0;
    int fi = ttp.n_forget;
    for (int o = tp.plan.n_ops - 1; o >= 0; --o) {
        const uint32_t w0 = tp.ops[(size_t)o * sweep::kTiledOpWords], kind = w0 & 15u, bit = 1u << ((w0 >> 4) & 31u);
        if (kind == sweep::kIntro) f &= ~bit;
        else if (kind == sweep::kForget) {
            --fi;
            const uint32_t *ft = &ttp.forget_tile[(size_t)fi * minplus::kForgetTileWords];
            const uint32_t x = sweep::bits_extract(f, ft[1]), h = minplus::remove_bit(sweep::bits_extract(f, ft[0]), ft[2]);
            if ((D[(size_t)ft[3] + (size_t)x * (size_t)ttp.words_per_tile + (h >> 6)] >> (h & 63u)) & 1ull) {
                f |= bit;
                for (int w = 0; w < tp.plan.W; ++w) chain[w] ^= ttp.forget_words[(size_t)fi * tp.plan.W + w];
            }
        }
    }
    return f;
}

int check_shape(int code, int L, int hbm_width, int tile_width, int cut_lds_width)
{
    const minplus::TiledTracePlan ttp = minplus::build_tiled_trace_plan(code, L, hbm_width, tile_width);
    const sweep::TiledPlan &tp = ttp.tiled;
    const sweep::Plan &p = tp.plan;
    if (p.refusal.code) { std::fprintf(stderr, "code %d L %d: refused: %s\n", code, L, p.refusal.msg.c_str()); return 1; }
    int fails = 0;
    // ---- the plan: every generator once, the offsets from the segment table
    std::vector<int> seen((size_t)p.n_gen, 0);
    for (const int g : tp.held) ++seen[(size_t)g];
    for (const int g : ttp.forget_gen) ++seen[(size_t)g];
    for (const int n : seen) fails += n != 1;
    uint64_t off = 0;
    uint32_t fi = 0;
    for (size_t s = 0; s < tp.segments.size(); ++s) {
        fails += ttp.seg_forget[s] != fi;
        for (uint32_t o = tp.segments[s].op_first; o < tp.segments[s].op_first + tp.segments[s].op_count; ++o)
            if ((tp.ops[(size_t)o * sweep::kTiledOpWords] & 15u) == sweep::kForget) {
                fails += ttp.forget_tile[(size_t)fi * 4 + 3] != off || ttp.forget_tile[(size_t)fi * 4] != tp.segments[s].tile;
                off += (uint64_t)tp.segments[s].n_tiles * (uint64_t)ttp.words_per_tile;
                ++fi;
            }
    }
    fails += (int)fi != ttp.n_forget || off != ttp.words_per_pair || ttp.n_forget != p.n_gen - tp.n_held;
    // ---- the twins over poisoned outputs of their exact size
    const uint64_t N = 2;
    const size_t n_out = (size_t)N * p.ncls, row = (size_t)p.nq * 4u;
    auto chains = exact<uint8_t>(N * p.nq, 0);
    for (uint64_t s = 1; s < N; ++s)
        for (int q = 0; q < p.nq; ++q) {
            const bool idle = p.code == QECMC_PLANAR && q >= p.L * p.L && ((q - p.L * p.L) / p.L == p.L - 1 || (q - p.L * p.L) % p.L == p.L - 1);
            if (!idle && draw() < 0x30000000u) chains[s * p.nq + q] = (uint8_t)(1 + draw() % 3);
        }
    auto out = exact<uint8_t>(n_out * p.nq, 0xEE), out2 = exact<uint8_t>(n_out * p.nq, 0xEE);
    auto cost = exact<uint32_t>(n_out, 0xEE), cost2 = exact<uint32_t>(n_out, 0xEE);
    auto count = exact<uint64_t>(n_out, 0xEE), count2 = exact<uint64_t>(n_out, 0xEE);
    auto cls = exact<int32_t>(N, 0xEE), cls2 = exact<int32_t>(N, 0xEE);
    const uint32_t costs[3][4] = {{0, 1, 1, 1}, {0, 1, 2, 1}, {1, 0, 2, 3}};
    for (const auto &c4 : costs) {
        minplus::minplus_tiled_trace_host(ttp, N, chains.get(), c4, out.get(), cost.get(), count.get(), cls.get(), 2);
        minplus::minplus_tiled_trace_host(ttp, N, chains.get(), c4, out2.get(), nullptr, nullptr, nullptr, 1);         // the three nullable outputs
        fails += std::memcmp(out.get(), out2.get(), n_out * p.nq) != 0;
        minplus::minplus_tiled_host(tp, N, chains.get(), c4, cost2.get(), count2.get(), cls2.get(), 1);
        fails += std::memcmp(cost.get(), cost2.get(), n_out * 4) != 0 || std::memcmp(count.get(), count2.get(), n_out * 8) != 0 || std::memcmp(cls.get(), cls2.get(), N * 4) != 0;
        if (cut_lds_width >= 0) {                                               // the cut plan has this stream: its twin's chains, byte for byte
            const minplus::TracePlan cut = minplus::build_trace_plan(code, L, cut_lds_width);
            if (cut.cut.plan.refusal.code) return 1;
            minplus::minplus_trace_host(cut, N, chains.get(), c4, out2.get(), cost2.get(), count2.get(), cls2.get(), 1);
            fails += std::memcmp(out.get(), out2.get(), n_out * p.nq) != 0 || std::memcmp(cost.get(), cost2.get(), n_out * 4) != 0;
        }
        // constant rows: the uniform twin, chains included
        auto cq = exact<uint8_t>(row, 0);
        for (size_t i = 0; i < row; ++i) cq[i] = (uint8_t)c4[i & 3u];
        minplus::minplus_tiled_trace_site_host(ttp, N, chains.get(), cq.get(), 1, out2.get(), cost2.get(), count2.get(), cls2.get(), 1);
        fails += std::memcmp(out.get(), out2.get(), n_out * p.nq) != 0 || std::memcmp(cost.get(), cost2.get(), n_out * 4) != 0;
        // ---- the device layout, pair by pair, over a dirty A and a dirty D of exactly words_per_pair words
        uint32_t cxz[4];
        minplus::costs_xz(c4, cxz);
        std::vector<uint32_t> reps((size_t)p.ncls * p.W), rep((size_t)p.W), fold_cost((size_t)p.ncls);
        std::vector<uint64_t> P((size_t)p.ncls << tp.n_held), fold_count((size_t)p.ncls);
        auto A = exact<uint64_t>((size_t)1 << tp.state_bits, 0x5A);
        auto D = exact<uint64_t>((size_t)ttp.words_per_pair, 0xC3);
        auto bytes = exact<uint8_t>((size_t)p.nq, 0xEE);
        for (uint64_t s = 0; s < N; ++s) {
            sweep::class_representatives(p, chains.get() + s * p.nq, reps.data());
            minplus::tiled_partials_fold(tp, reps.data(), 1, P.data(), fold_cost.data(), fold_count.data(),
                                         [&](const uint32_t *r, uint64_t *Am) { return minplus::minplus_one_wide(tp, r, cxz, Am); });
            for (int c = 0; c < p.ncls; ++c) {
                const uint32_t pick = minplus::pick_assignment(&P[(size_t)c << tp.n_held], tp.n_held);
                sweep::tiled_representative(tp, &reps[(size_t)c * p.W], pick, rep.data());
                device_layout_trace(ttp, rep.data(), [&](uint32_t, uint32_t idx) { return cxz[idx]; }, A.get(), D.get());
                fails += device_layout_walk(ttp, D.get(), rep.data()) != 0;
                minplus::unpack_chain(rep.data(), p.nq, bytes.get());
                fails += std::memcmp(bytes.get(), out.get() + (s * p.ncls + (uint64_t)c) * p.nq, (size_t)p.nq) != 0;
            }
        }
    }
    // random bytes, a row per syndrome: every syndrome as the one table of a call of its own
    auto cq = exact<uint8_t>(N * row, 0);
    for (size_t i = 0; i < N * row; ++i) cq[i] = (uint8_t)draw();
    minplus::minplus_tiled_trace_site_host(ttp, N, chains.get(), cq.get(), N, out.get(), cost.get(), count.get(), cls.get());
    for (uint64_t s = 0; s < N; ++s) {
        auto o1 = exact<uint8_t>((size_t)p.ncls * p.nq, 0xEE);
        minplus::minplus_tiled_trace_site_host(ttp, 1, chains.get() + s * p.nq, cq.get() + s * row, 1, o1.get(), nullptr, nullptr, nullptr, 1);
        fails += std::memcmp(o1.get(), out.get() + s * p.ncls * p.nq, (size_t)p.ncls * p.nq) != 0;
    }
    if (fails) std::fprintf(stderr, "code %d L %d hbm_width %d tile_width %d: %d checks failed\n", code, L, hbm_width, tile_width, fails);
    std::printf("code %d L %d hbm_width %d tile_width %d: %d held, width %d, %d FORGETs, %zu segments, %llu bytes per pair\n", code, L, hbm_width, tile_width, tp.n_held,
                p.width, ttp.n_forget, tp.segments.size(), (unsigned long long)minplus::tiled_trace_bytes_per_pair(ttp));
    return fails != 0;
}

int check_refusals()
{
    int rc = 0;
    const struct { int code, L, hbm_width, tile_width, want; } refused[] = {{QECMC_XZZX, 4, 0, 0, QECMC_ERR_INVALID}, {QECMC_TORIC, 4, 0, 0, QECMC_ERR_UNSUPPORTED},
                                                                          {QECMC_TORIC, 9, 0, 0, QECMC_ERR_UNSUPPORTED}, {QECMC_XZZX, 3, 0, 3, QECMC_ERR_INVALID},
                                                                          {QECMC_XZZX, 3, 25, 0, QECMC_ERR_INVALID}, {-1, 3, 0, 0, QECMC_ERR_INVALID}};
    for (const auto &s : refused)
        for (const char *entry : {"qecmc_class_minplus_tiled_chains", "qecmc_class_minplus_tiled_chains_site"}) {
            const sweep::TiledPlan plain = sweep::build_tiled_plan(s.code, s.L, s.hbm_width, s.tile_width);
            const minplus::TiledTracePlan ttp = minplus::build_tiled_trace_plan(s.code, s.L, s.hbm_width, s.tile_width, entry);
            const Refusal &r = ttp.tiled.plan.refusal;
            if (r.code != s.want || plain.plan.refusal.code != s.want || r.msg != std::string(entry) + ": " + plain.plan.refusal.msg) {
                std::fprintf(stderr, "code %d L %d hbm_width %d tile_width %d: refusal %d: %s\n", s.code, s.L, s.hbm_width, s.tile_width, r.code, r.msg.c_str());
                rc = 1;
            }
        }
    // the cap: one byte short refuses by name with the bytes, the exact size passes
    const minplus::TiledTracePlan fits = minplus::build_tiled_trace_plan(QECMC_ROTATED, 7, 0, 5);
    const uint64_t bytes = minplus::tiled_trace_bytes_per_pair(fits);
    const minplus::TiledTracePlan at = minplus::build_tiled_trace_plan(QECMC_ROTATED, 7, 0, 5, "qecmc_class_minplus_tiled_chains", bytes);
    const minplus::TiledTracePlan past = minplus::build_tiled_trace_plan(QECMC_ROTATED, 7, 0, 5, "qecmc_class_minplus_tiled_chains", bytes - 1);
    rc |= fits.tiled.plan.refusal.code != 0 || at.tiled.plan.refusal.code != 0 || past.tiled.plan.refusal.code != QECMC_ERR_UNSUPPORTED ||
          past.tiled.plan.refusal.msg.rfind("qecmc_class_minplus_tiled_chains: the decisions of one", 0) != 0 ||
          past.tiled.plan.refusal.msg.find(std::to_string(bytes) + " bytes") == std::string::npos;
    // the pairs of a pass
    rc |= minplus::tiled_trace_pass_pairs(24, 303650944ull, 16) != 7u || minplus::tiled_trace_pass_pairs(16, 496896ull, 4096) != 2048u ||
          minplus::tiled_trace_pass_pairs(16, 496896ull, 4096, 100ull * 496896ull) != 100u || minplus::tiled_trace_pass_pairs(24, 1ull << 40, 5) != 1u ||
          minplus::tiled_trace_pass_pairs(16, 8, 3) != 3u;
    const uint32_t top[4] = {0, 1, 256, 1}, far[4] = {0, 149, 1, 1};
    const sweep::TiledPlan r21 = sweep::build_tiled_plan(QECMC_ROTATED, 21, 0, 0);
    rc |= minplus::check_tiled_chain_costs(nullptr, top).msg.rfind("qecmc_class_minplus_tiled_chains: cost[2]=256", 0) != 0;
    rc |= minplus::check_tiled_chain_costs(&r21.plan, far).code != QECMC_ERR_UNSUPPORTED ||
          minplus::check_tiled_chain_costs(&r21.plan, far).msg.rfind("qecmc_class_minplus_tiled_chains: 441 qubits", 0) != 0;
    if (rc) std::fprintf(stderr, "the refusals failed\n");
    return rc;
}

}  // namespace

int main()
{
    int rc = check_refusals(), shapes_run = 0;
    // (code, L, hbm_width, tile_width, the lds_width of the cut plan with the same stream and holds or -1)
    const struct { int code, L, hbm_width, tile_width, cut; } shapes[] = {
        {QECMC_XZZX, 3, 0, 4, 0},     {QECMC_PLANAR, 3, 0, 0, 0},   {QECMC_TORIC, 3, 0, 6, -1},   {QECMC_TORIC, 3, 8, 4, -1},  {QECMC_TORIC, 3, 13, 5, 13},
        {QECMC_XZZX, 5, 0, 4, 0},     {QECMC_ROTATED, 5, 5, 4, -1}, {QECMC_ROTATED, 7, 0, 5, 0},  {QECMC_ROTATED, 7, 0, 7, 0}, {QECMC_ROTATED, 9, 0, 8, 0},
        {QECMC_PLANAR, 5, 8, 5, -1},  {QECMC_XZZX, 5, 6, 4, -1}};
    for (const auto &s : shapes) {
        rc |= check_shape(s.code, s.L, s.hbm_width, s.tile_width, s.cut);
        ++shapes_run;
    }
    rc |= shapes_run < 12;
    std::printf(rc ? "class minplus tiled trace selftest FAILED\n" : "class minplus tiled trace selftest OK\n");
    return rc;
}
