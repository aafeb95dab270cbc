// Stand-alone check of class_minplus_tiled.hpp for the sanitizers (make minplus_tiled_asan: -fsanitize=address,undefined): tiled plans of the small
// shapes under several widths of state vector and tile -- nothing held, holds forced by a narrow hbm_width -- with the tiled plan's refusals behind
// this entry point's prefixes; the twin minplus_tiled_host, threaded and not, over outputs of their exact size, against minplus_cut_host where the
// cut plans take the shape and at rank <= 16 against a brute force over every subset of the generator table; minplus_one_wide over POISONED scratch;
// the site twin over tables of exactly rows * nq * 4 bytes, constant rows against the uniform twin and one row per syndrome against that row alone;
// the cost-range checks at their limits.  Exit status 0: all held.
#include "class_minplus_tiled.hpp"

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

// over every subset of the generator table: the least cost over the qubits a generator touches, and the number of subsets that reach it
void brute_force(const sweep::Plan &p, const uint8_t *chain, const uint32_t *cost4, uint32_t *cost, uint64_t *count)
{
    const correct::Table ct = correct::build_table(p.code, p.L);
    std::vector<std::vector<uint8_t>> gen((size_t)p.n_gen, std::vector<uint8_t>((size_t)p.nq, 0));
    std::vector<char> touched((size_t)p.nq, 0);
    for (int g = 0; g < p.n_gen; ++g)
        for (int i = 0; i < 4; ++i) {
            const uint32_t e = (ct.gen[(size_t)(2 * g + (i >> 1))] >> ((i & 1) * 16)) & 0xFFFFu, pauli = e & 3u, site = e >> 2;
            if (pauli) { gen[(size_t)g][site] ^= (uint8_t)pauli; touched[site] = 1; }
        }
    std::vector<uint8_t> cur(chain, chain + p.nq);
    *cost = 0xFFFFFFFFu; *count = 0;
    for (uint64_t k = 0; k < (1ull << p.n_gen); ++k) {
        if (k) {                                                                // Gray code: one generator per step
            const int g = __builtin_ctzll(k);
            for (int q = 0; q < p.nq; ++q) cur[(size_t)q] ^= gen[(size_t)g][(size_t)q];
        }
        uint32_t c = 0;
        for (int q = 0; q < p.nq; ++q)
            if (touched[(size_t)q]) c += cost4[cur[(size_t)q] & 3u];
        if (c < *cost) { *cost = c; *count = 1; }
        else if (c == *cost) ++*count;
    }
}

// buffers of exactly n elements on the heap, so that one element too far is seen
template <class T> std::unique_ptr<T[]> exact(size_t n, int fill)
{
    std::unique_ptr<T[]> p(new T[n ? n : 1]);
    std::memset(p.get(), fill, (n ? n : 1) * sizeof(T));
    return p;
}

int check_twin(const sweep::TiledPlan &tp, bool cut_takes_it)
{
    const sweep::Plan &p = tp.plan;
    const uint64_t N = 3;
    const int shift = p.n_gen - p.rank;
    const size_t n_out = (size_t)N * p.ncls, row = (size_t)p.nq * 4u;
    int fails = 0;
    auto chains = exact<uint8_t>(N * p.nq, 0);
    for (uint64_t s = 1; s < N; ++s)
        for (int q = 0; q < p.nq; ++q) {
            const bool idle = p.code == QECMC_PLANAR && q >= p.L * p.L && ((q - p.L * p.L) / p.L == p.L - 1 || (q - p.L * p.L) % p.L == p.L - 1);
            if (!idle && draw() < 0x40000000u) chains[s * p.nq + q] = (uint8_t)(1 + draw() % 3);
        }
    auto cost = exact<uint32_t>(n_out, 0xEE), cost1 = exact<uint32_t>(n_out, 0xEE), costc = exact<uint32_t>(n_out, 0xEE);
    auto count = exact<uint64_t>(n_out, 0xEE), count1 = exact<uint64_t>(n_out, 0xEE), countc = exact<uint64_t>(n_out, 0xEE);
    auto cls = exact<int32_t>(N, 0xEE), cls2 = exact<int32_t>(N, 0xEE);
    const auto same = [&](const uint32_t *a, const uint64_t *b) { return !std::memcmp(a, cost.get(), n_out * 4) && !std::memcmp(b, count.get(), n_out * 8); };
    const uint32_t costs[3][4] = {{0, 1, 1, 1}, {0, 1, 2, 1}, {1, 0, 2, 3}};
    for (const auto &c4 : costs) {
        minplus::minplus_tiled_host(tp, N, chains.get(), c4, cost.get(), count.get(), cls.get(), 4);
        minplus::minplus_tiled_host(tp, N, chains.get(), c4, cost1.get(), count1.get(), nullptr, 1);
        fails += !same(cost1.get(), count1.get());
        for (size_t i = 0; i < n_out; ++i) fails += count[i] == 0;
        if (cut_takes_it) {
            const sweep::CutPlan cp = minplus::build_minplus_plan(p.code, p.L, 0);
            if (cp.plan.refusal.code) return 1;
            minplus::minplus_cut_host(cp, N, chains.get(), c4, costc.get(), countc.get(), cls2.get());
            fails += !same(costc.get(), countc.get()) || std::memcmp(cls.get(), cls2.get(), N * 4) != 0;
        }
        // one unit's twin over poisoned scratch: only A[0] is set up
        if (tp.n_held == 0) {
            std::vector<uint64_t> A((size_t)1 << p.width, 0xDEADBEEFDEADBEEFull);
            std::vector<uint32_t> reps((size_t)p.ncls * p.W);
            uint32_t cxz[4];
            minplus::costs_xz(c4, cxz);
            for (uint64_t s = 0; s < N; ++s) {
                sweep::class_representatives(p, chains.get() + s * p.nq, reps.data());
                for (int c = 0; c < p.ncls; ++c) {
                    uint32_t c1; uint64_t n1;
                    minplus::mp_unpack(minplus::minplus_one_wide(tp, &reps[(size_t)c * p.W], cxz, A.data()), shift, &c1, &n1);
                    fails += c1 != cost[s * p.ncls + c] || n1 != count[s * p.ncls + c];
                }
            }
        }
        if (p.rank <= 16)
            for (uint64_t s = 0; s < N; ++s) {
                uint32_t c1; uint64_t n1;
                brute_force(p, chains.get() + s * p.nq, c4, &c1, &n1);
                const size_t own = s * p.ncls + (size_t)cls[s];
                fails += c1 != cost[own] || (n1 >> shift) != count[own] || (n1 & ((1ull << shift) - 1ull)) != 0;
            }
        // constant rows, one table and one per syndrome: the uniform twin
        for (const uint64_t rows : {(uint64_t)1, N}) {
            auto cq = exact<uint8_t>(rows * row, 0);
            for (size_t i = 0; i < rows * row; ++i) cq[i] = (uint8_t)c4[i & 3u];
            minplus::minplus_tiled_site_host(tp, N, chains.get(), cq.get(), rows, cost1.get(), count1.get(), cls2.get(), 2);
            fails += !same(cost1.get(), count1.get()) || std::memcmp(cls.get(), cls2.get(), N * 4) != 0;
        }
    }
    // random bytes, a row per syndrome: every syndrome as the one table of a call of its own
    auto cq = exact<uint8_t>(N * row, 0);
    for (size_t i = 0; i < N * row; ++i) cq[i] = (uint8_t)draw();
    minplus::minplus_tiled_site_host(tp, N, chains.get(), cq.get(), N, cost.get(), count.get(), cls.get());
    for (uint64_t s = 0; s < N; ++s) {
        auto c1 = exact<uint32_t>((size_t)p.ncls, 0xEE);
        auto n1 = exact<uint64_t>((size_t)p.ncls, 0xEE);
        minplus::minplus_tiled_site_host(tp, 1, chains.get() + s * p.nq, cq.get() + s * row, 1, c1.get(), n1.get(), nullptr, 1);
        fails += std::memcmp(c1.get(), cost.get() + s * p.ncls, (size_t)p.ncls * 4) != 0 || std::memcmp(n1.get(), count.get() + s * p.ncls, (size_t)p.ncls * 8) != 0;
    }
    fails += minplus::check_tiled_cost_rows_range(cq.get(), N, p.nq, sweep::closed_qubits(tp.ops, p.nq)).code != 0;
    if (fails) std::fprintf(stderr, "code %d L %d hbm_width %d tile_width %d: %d twin checks failed\n", p.code, p.L, tp.hbm_width, tp.tile_width, fails);
    return fails != 0;
}

int check_ranges()
{
    int rc = 0;
    const sweep::TiledPlan r21 = sweep::build_tiled_plan(QECMC_ROTATED, 21, 0, 0), p12 = sweep::build_tiled_plan(QECMC_PLANAR, 12, 0, 0);
    if (r21.plan.refusal.code || p12.plan.refusal.code || r21.plan.n_qubits != 441 || p12.plan.n_qubits != 265) return 1;
    const uint32_t at[4] = {0, 148, 1, 1}, past[4] = {149, 0, 0, 0}, p_at[4] = {0, 1, 247, 1}, p_past[4] = {0, 1, 1, 248}, top[4] = {0, 1, 256, 1};
    rc |= minplus::check_tiled_cost_range(r21.plan, at).code != 0 || minplus::check_tiled_cost_range(r21.plan, past).code != QECMC_ERR_UNSUPPORTED;
    rc |= minplus::check_tiled_cost_range(p12.plan, p_at).code != 0 || minplus::check_tiled_cost_range(p12.plan, p_past).code != QECMC_ERR_UNSUPPORTED;
    rc |= minplus::check_tiled_costs(top).code != QECMC_ERR_INVALID || minplus::check_tiled_costs(top).msg.rfind("qecmc_class_minplus_tiled: cost[2]=256", 0) != 0;
    // a table of exactly 2 * nq * 4 bytes: the planar code's unused cells at 255 do not count, eleven qubits at 255 carry row 1 past the limit
    const int nq = p12.plan.nq;
    const std::vector<char> named = sweep::closed_qubits(p12.ops, nq);
    int closed = 0;
    for (const char c : named) closed += c;
    rc |= closed != 265;
    auto cq = exact<uint8_t>((size_t)2 * nq * 4, 0);
    for (int r = 0; r < 2; ++r)
        for (int q = 0; q < nq; ++q) cq[((size_t)r * nq + q) * 4 + 3] = named[(size_t)q] ? 247 : 255;
    rc |= minplus::check_tiled_cost_rows_range(cq.get(), 2, nq, named).code != 0;
    for (int q = 0, n = 0; q < nq && n < 11; ++q)
        if (named[(size_t)q]) { cq[((size_t)nq + q) * 4 + 1] = 255; ++n; }
    const Refusal r = minplus::check_tiled_cost_rows_range(cq.get(), 2, nq, named);
    rc |= r.code != QECMC_ERR_UNSUPPORTED || r.msg.rfind("qecmc_class_minplus_tiled_site: cq row 1:", 0) != 0 || r.msg.find("65543") == std::string::npos;
    rc |= minplus::check_tiled_cost_rows_range(cq.get(), 1, nq, named).code != 0;
    if (rc) std::fprintf(stderr, "the cost-range checks failed\n");
    return rc;
}

}  // namespace

int main()
{
    int rc = check_ranges(), twins = 0, held = 0;
    // (code, L, hbm_width, tile_width, the cut plans take the shape at their default)
    const struct { int code, L, hbm_width, tile_width; bool cut; } shapes[] = {
        {QECMC_XZZX, 3, 0, 4, true}, {QECMC_ROTATED, 3, 4, 4, true}, {QECMC_PLANAR, 3, 0, 0, true}, {QECMC_TORIC, 3, 0, 6, true}, {QECMC_TORIC, 3, 8, 4, true},
        {QECMC_XZZX, 5, 0, 4, true}, {QECMC_ROTATED, 5, 5, 4, true}, {QECMC_ROTATED, 7, 0, 5, true}, {QECMC_PLANAR, 4, 0, 13, true}, {QECMC_PLANAR, 5, 8, 5, true}};
    for (const auto &s : shapes) {
        const sweep::TiledPlan plain = sweep::build_tiled_plan(s.code, s.L, s.hbm_width, s.tile_width);
        const sweep::TiledPlan tp = minplus::build_minplus_tiled_plan(s.code, s.L, s.hbm_width, s.tile_width, "qecmc_class_minplus_tiled");
        if (tp.plan.refusal.code || plain.plan.refusal.code || tp.ops != plain.ops || tp.dev_ops != plain.dev_ops || tp.held_words != plain.held_words) {
            std::fprintf(stderr, "code %d L %d hbm_width %d tile_width %d: not the tiled plan (%d: %s)\n", s.code, s.L, s.hbm_width, s.tile_width, tp.plan.refusal.code,
                         tp.plan.refusal.msg.c_str());
            rc = 1;
            continue;
        }
        std::printf("code %d L %d hbm_width %d tile_width %d: %d held, width %d, rank %d, %zu segments\n", s.code, s.L, s.hbm_width, s.tile_width, tp.n_held, tp.plan.width,
                    tp.plan.rank, tp.segments.size());
        rc |= check_twin(tp, s.cut);
        ++twins;
        held += tp.n_held > 0;
    }
    // the tiled plan's refusals, prefixed
    const struct { int code, L, hbm_width, tile_width, want; } refused[] = {{QECMC_XZZX, 4, 0, 0, QECMC_ERR_INVALID}, {QECMC_TORIC, 4, 0, 0, QECMC_ERR_UNSUPPORTED},
                                                                          {QECMC_TORIC, 9, 0, 0, QECMC_ERR_UNSUPPORTED}, {QECMC_ROTATED, 23, 0, 0, QECMC_ERR_UNSUPPORTED},
                                                                          {QECMC_XZZX, 3, 0, 3, QECMC_ERR_INVALID}, {QECMC_XZZX, 3, 25, 0, QECMC_ERR_INVALID},
                                                                          {QECMC_TORIC, 7, 16, 0, QECMC_ERR_UNSUPPORTED}, {-1, 3, 0, 0, QECMC_ERR_INVALID}};
    for (const auto &s : refused)
        for (const char *entry : {"qecmc_class_minplus_tiled", "qecmc_class_minplus_tiled_site"}) {
            const sweep::TiledPlan plain = sweep::build_tiled_plan(s.code, s.L, s.hbm_width, s.tile_width);
            const sweep::TiledPlan tp = minplus::build_minplus_tiled_plan(s.code, s.L, s.hbm_width, s.tile_width, entry);
            if (tp.plan.refusal.code != s.want || plain.plan.refusal.code != s.want || tp.plan.refusal.msg != std::string(entry) + ": " + plain.plan.refusal.msg) {
                std::fprintf(stderr, "code %d L %d hbm_width %d tile_width %d: refusal %d: %s\n", s.code, s.L, s.hbm_width, s.tile_width, tp.plan.refusal.code,
                             tp.plan.refusal.msg.c_str());
                rc = 1;
            }
        }
    rc |= twins < 10 || held < 3;
    std::printf(rc ? "class minplus tiled selftest FAILED\n" : "class minplus tiled selftest OK\n");
    return rc;
}
