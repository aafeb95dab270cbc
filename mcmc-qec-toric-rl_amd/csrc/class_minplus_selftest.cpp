// Stand-alone check of class_minplus.hpp for the sanitizers (make minplus_asan: -fsanitize=address,undefined): builds the plan of every (code, L)
// with L in [1, 13] and of a few large L under lds_width 0, 13, 14 and a narrow one and checks that it is build_cut_plan's -- accepted where that
// one accepts, refused with its code and its message behind the prefix where it refuses; checks the combine's algebra (the tie rule, sticky
// saturation, associativity and commutativity over random triples, counts near kSat among them); then, for every accepted plan that is cheap enough,
// runs the twin on random chains: minplus_one over POISONED scratch against minplus_cut_host, threaded against not, the narrow plan (generators held)
// against the default plan, all-zero costs against the size of the group -- saturated where 2^n_gen passes kSat --, and at rank <= 16 against a brute
// force over every subset of the generator table.  Exit status 0: all held.
#include "class_minplus.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace qecmc;

namespace {

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t draw()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

int check_combine()
{
    using namespace minplus;
    int fails = 0;
    const auto pack = [](uint64_t cost, uint64_t count) { return (cost << kCountBits) | count; };
    fails += mp_combine(pack(3, 5), pack(4, 9)) != pack(3, 5) || mp_combine(pack(4, 9), pack(3, 5)) != pack(3, 5);
    fails += mp_combine(pack(3, 5), pack(3, 9)) != pack(3, 14);
    fails += mp_sat_add(kSat, 0) != kSat || mp_sat_add(kSat, 1) != kSat || mp_sat_add(kSat, kSat) != kSat || mp_sat_add(kSat - 1, 1) != kSat || mp_sat_add(kSat - 2, 1) != kSat - 1;
    fails += mp_combine(pack(7, kSat), pack(7, 1)) != pack(7, kSat) || mp_combine(pack(7, kSat - 1), pack(7, 5)) != pack(7, kSat);
    fails += mp_combine(pack(7, kSat), pack(6, 1)) != pack(6, 1);               // (a cheaper entry replaces a saturated one)
    fails += mp_combine(pack(0xFFFF, 1), pack(0xFFFF, 1)) != pack(0xFFFF, 2);
    for (int i = 0; i < 20000; ++i) {
        uint64_t e[3];
        for (uint64_t &x : e) {
            const uint32_t how = draw() % 4u;
            const uint64_t count = how == 0 ? 1ull + draw() % 7u : how == 1 ? kSat - draw() % 5u : how == 2 ? (kSat >> 1) + draw() % 3u : 1ull + (((uint64_t)draw() << 16) | (draw() & 0xFFFFu));
            x = pack(draw() % 3u, count > kSat ? kSat : count);
        }
        fails += mp_combine(mp_combine(e[0], e[1]), e[2]) != mp_combine(e[0], mp_combine(e[1], e[2]));
        fails += mp_combine(e[0], e[1]) != mp_combine(e[1], e[0]);
    }
    if (fails) std::fprintf(stderr, "%d combine checks failed\n", fails);
    return fails != 0;
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

int check_twin(const sweep::CutPlan &cp)
{
    const sweep::Plan &p = cp.plan;
    const sweep::CutPlan full = minplus::build_minplus_plan(p.code, p.L, 0);
    if (full.plan.refusal.code) return 1;
    const uint64_t N = 3;
    const int shift = p.n_gen - p.rank;
    int fails = 0;
    std::vector<uint8_t> chains(N * p.nq, 0);
    for (uint64_t s = 1; s < N; ++s)
        for (int q = 0; q < p.nq; ++q) {
            const bool idle = p.code == QECMC_PLANAR && q >= p.L * p.L && ((q - p.L * p.L) / p.L == p.L - 1 || (q - p.L * p.L) % p.L == p.L - 1);
            if (!idle && draw() < 0x40000000u) chains[s * p.nq + q] = (uint8_t)(1 + draw() % 3);
        }
    const size_t n_out = (size_t)N * p.ncls;
    std::vector<uint32_t> cost(n_out), cost1(n_out), costf(n_out);
    std::vector<uint64_t> count(n_out), count1(n_out), countf(n_out);
    std::vector<int32_t> cls(N), cls2(N);
    const uint32_t costs[3][4] = {{0, 1, 1, 1}, {0, 3, 3, 1}, {1, 0, 2, 3}}, zero[4] = {0, 0, 0, 0};
    for (const auto &c4 : costs) {
        minplus::minplus_cut_host(cp, N, chains.data(), c4, cost.data(), count.data(), cls.data(), 4);
        minplus::minplus_cut_host(cp, N, chains.data(), c4, cost1.data(), count1.data(), nullptr, 1);
        minplus::minplus_cut_host(full, N, chains.data(), c4, costf.data(), countf.data(), cls2.data());
        fails += cost != cost1 || count != count1 || cost != costf || count != countf || cls != cls2;
        for (size_t i = 0; i < n_out; ++i) fails += count[i] == 0;
        // one workgroup's twin over poisoned scratch: only A[0] is set up
        if (cp.n_held == 0) {
            std::vector<uint64_t> A((size_t)1 << p.width, 0xDEADBEEFDEADBEEFull);
            std::vector<uint32_t> reps((size_t)p.ncls * p.W);
            uint32_t cxz[4];
            minplus::costs_xz(c4, cxz);
            for (uint64_t s = 0; s < N; ++s) {
                sweep::class_representatives(p, chains.data() + s * p.nq, reps.data());
                for (int c = 0; c < p.ncls; ++c) {
                    uint32_t c1; uint64_t n1;
                    minplus::mp_unpack(minplus::minplus_one(p, &reps[(size_t)c * p.W], cxz, A.data()), shift, &c1, &n1);
                    fails += c1 != cost[s * p.ncls + c] || n1 != count[s * p.ncls + c];
                }
            }
        }
        if (p.rank <= 16)
            for (uint64_t s = 0; s < N; ++s) {
                uint32_t c1; uint64_t n1;
                brute_force(p, chains.data() + s * p.nq, c4, &c1, &n1);
                const size_t own = s * p.ncls + (size_t)cls[s];
                fails += c1 != cost[own] || (n1 >> shift) != count[own] || (n1 & ((1ull << shift) - 1ull)) != 0;
            }
    }
    // all-zero costs: every subset reaches cost 0, so the count is the group's size -- or saturated, where 2^n_gen subsets pass kSat
    minplus::minplus_cut_host(cp, N, chains.data(), zero, cost.data(), count.data(), nullptr);
    for (size_t i = 0; i < n_out; ++i) fails += cost[i] != 0 || count[i] != (p.n_gen >= minplus::kCountBits ? 0ull : 1ull << p.rank);
    if (fails) std::fprintf(stderr, "code %d L %d lds_width %d: %d twin checks failed\n", p.code, p.L, cp.lds_width, fails);
    return fails != 0;
}

}  // namespace

int main()
{
    int rc = check_combine(), twins = 0, saturated = 0;
    const int Ls[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 33, 64, 65};
    for (int code = -1; code <= 4; ++code)
        for (const int L : Ls)
            for (const int lds_width : {0, 13, 14, 6}) {
                if (L > 13 && lds_width != 0) continue;
                const sweep::CutPlan cut = sweep::build_cut_plan(code, L, lds_width);
                const sweep::CutPlan cp = minplus::build_minplus_plan(code, L, lds_width);
                if (cp.plan.refusal.code != cut.plan.refusal.code || (cut.plan.refusal.code && cp.plan.refusal.msg != "qecmc_class_minplus: " + cut.plan.refusal.msg) ||
                    (!cut.plan.refusal.code && (cp.plan.ops != cut.plan.ops || cp.held_words != cut.held_words || cp.n_held != cut.n_held))) {
                    std::fprintf(stderr, "code %d L %d lds_width %d: not the cut plan (%d: %s)\n", code, L, lds_width, cp.plan.refusal.code, cp.plan.refusal.msg.c_str());
                    rc = 1;
                }
                if (cp.plan.refusal.code) continue;
                rc |= minplus::check_cost_range(cp.plan).code != 0 || cp.plan.n_gen - cp.plan.rank < 0 || cp.plan.n_gen - cp.plan.rank > 2;
                // cheap enough here: the narrow plans of the small shapes (held generators), and every plan that holds nothing up to width 11
                const bool narrow = lds_width == 6 && cp.full_width <= 10, plain = lds_width == 0 && cp.n_held == 0 && cp.plan.width <= 11;
                if (narrow || plain) {
                    std::printf("code %d L %d lds_width %d: %d held, width %d, rank %d\n", code, L, lds_width, cp.n_held, cp.plan.width, cp.plan.rank);
                    rc |= check_twin(cp);
                    ++twins;
                    saturated += cp.plan.n_gen >= minplus::kCountBits;
                }
            }
    const uint32_t bad[4] = {0, 1, 256, 1}, good[4] = {255, 0, 255, 7};
    rc |= minplus::check_costs(bad).code != QECMC_ERR_INVALID || minplus::check_costs(good).code != 0;
    for (const int w : {-1, 1, 15, 99}) rc |= minplus::build_minplus_plan(QECMC_XZZX, 3, w).plan.refusal.code != QECMC_ERR_INVALID;
    rc |= twins < 12 || saturated < 2;
    std::printf(rc ? "class minplus selftest FAILED\n" : "class minplus selftest OK\n");
    return rc;
}
