// Stand-alone check of class_sweep_cut.hpp for the sanitizers (make sweep_cut_asan: -fsanitize=address,undefined): builds the cut plan of every
// (code, L) with L in [1, 13] and of a few large L under lds_width 0, 13, 14 and a narrow one, checks WHICH are accepted, that an accepted plan keeps
// width <= lds_width and n_held <= kMaxHeld, that its held words are the held generators' Paulis and that the launch group keeps a launch within
// kCutGridMax; that a plan which holds nothing is build_plan's stream word for word; then, for narrow widths at the small shapes, runs the cut twin
// on random chains -- threaded and not -- against the uncut twin: all-ones weights give exactly 2^rank, other weights agree to a relative 1e-12,
// one thread and many give the same bits.  Exit status 0: all held.
#include "class_sweep_cut.hpp"

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

int check_plan(const sweep::CutPlan &cp, int lds_width)
{
    const sweep::Plan &p = cp.plan;
    int fails = 0;
    fails += p.width > cp.lds_width || (lds_width && cp.lds_width != lds_width) || cp.n_held > sweep::kMaxHeld || cp.n_held < cp.full_width - cp.lds_width;
    fails += !sweep::cut_fits(p.width) || (int)p.ops.size() != p.n_ops * sweep::kOpWords || (int)cp.held.size() != cp.n_held;
    fails += cp.held_words.size() != (size_t)cp.n_held * p.W;
    const correct::Table ct = correct::build_table(p.code, p.L);
    for (int j = 0; j < cp.n_held && !fails; ++j) {
        std::vector<uint8_t> chain((size_t)p.nq, 0);
        const int g = cp.held[(size_t)j];
        fails += g < 0 || g >= p.n_gen || (j && cp.held[(size_t)j - 1] >= g);
        for (int i = 0; i < 4 && !fails; ++i) {
            const uint32_t e = (ct.gen[(size_t)(2 * g + (i >> 1))] >> ((i & 1) * 16)) & 0xFFFFu, pauli = e & 3u, site = e >> 2;
            if (pauli) chain[site] ^= (uint8_t)pauli;
        }
        for (int q = 0; q < p.nq; ++q) fails += ((cp.held_words[(size_t)j * p.W + (q >> 4)] >> ((q & 15) * 2)) & 3u) != chain[(size_t)q];
    }
    for (uint64_t N : {0ull, 1ull, 5ull, 100000ull}) {
        const uint32_t group = sweep::cut_launch_group(N, p.ncls, cp.n_held);
        fails += group < 1u || group > sweep::kGroupMax || ((uint64_t)group * p.ncls << cp.n_held) > sweep::kCutGridMax;
    }
    if (cp.n_held == 0 && p.width <= sweep::kMaxWidth) {
        const sweep::Plan q = sweep::build_plan(p.code, p.L);
        fails += q.refusal.code != 0 || q.ops != p.ops || q.scale != p.scale || q.width != p.width;
    }
    if (fails) std::fprintf(stderr, "code %d L %d lds_width %d: %d plan checks failed\n", p.code, p.L, lds_width, fails);
    return fails != 0;
}

int check_twin(const sweep::CutPlan &cp)
{
    const sweep::Plan &p = cp.plan;
    const sweep::Plan full = sweep::build_plan(p.code, p.L);
    if (full.refusal.code) return 1;
    const uint64_t N = 3;
    int fails = 0;
    std::vector<uint8_t> chains(N * p.nq, 0);
    for (uint64_t s = 1; s < N; ++s)
        for (int q = 0; q < p.nq; ++q) {
            const bool idle = p.code == QECMC_PLANAR && q >= p.L * p.L && ((q - p.L * p.L) / p.L == p.L - 1 || (q - p.L * p.L) % p.L == p.L - 1);
            if (!idle && draw() < 0x40000000u) chains[s * p.nq + q] = (uint8_t)(1 + draw() % 3);
        }
    std::vector<double> ones(N * p.ncls), z(N * p.ncls), z1(N * p.ncls), want(N * p.ncls);
    std::vector<int32_t> cls(N), cls2(N);
    const double w1[4] = {1.0, 1.0, 1.0, 1.0}, w[4] = {1.0, 0.031, 0.017, 0.29};
    sweep::sweep_cut_host(cp, N, chains.data(), w1, ones.data(), cls.data());
    for (size_t i = 0; i < ones.size(); ++i) fails += ones[i] != std::ldexp(1.0, p.rank);
    sweep::sweep_cut_host(cp, N, chains.data(), w, z.data(), nullptr, 4);
    sweep::sweep_cut_host(cp, N, chains.data(), w, z1.data(), nullptr, 1);
    sweep::sweep_host(full, N, chains.data(), w, want.data(), cls2.data());
    fails += std::memcmp(z.data(), z1.data(), z.size() * sizeof(double)) != 0;
    for (size_t i = 0; i < z.size(); ++i) fails += !(z[i] > 0.0) || std::fabs(z[i] - want[i]) > 1e-12 * want[i];
    for (uint64_t s = 0; s < N; ++s) fails += cls[s] != cls2[s];
    if (cp.n_held == 0) fails += std::memcmp(z.data(), want.data(), z.size() * sizeof(double)) != 0;
    if (fails) std::fprintf(stderr, "code %d L %d lds_width %d: %d twin checks failed\n", p.code, p.L, cp.lds_width, fails);
    return fails != 0;
}

}  // namespace

int main()
{
    int rc = 0, twins = 0;
    const int Ls[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 33, 64, 65};
    for (int code = -1; code <= 4; ++code)
        for (const int L : Ls)
            for (const int lds_width : {0, 13, 14, 6}) {
                if (L > 13 && lds_width != 0) continue;
                const sweep::CutPlan cp = sweep::build_cut_plan(code, L, lds_width);
                const bool odd_code = code == QECMC_XZZX || code == QECMC_ROTATED;
                int expect = QECMC_ERR_UNSUPPORTED;
                if (code < 0 || code > 3 || L < 2 || L > 64 || (odd_code && L % 2 == 0)) expect = QECMC_ERR_INVALID;
                else if (code == QECMC_TORIC && L % 2 == 0) expect = QECMC_ERR_UNSUPPORTED;
                else if (lds_width == 6) expect = (code == QECMC_TORIC && L == 3) || (code == QECMC_PLANAR && L <= 4) || (odd_code && L <= 5) ? 0 : cp.plan.refusal.code ? QECMC_ERR_UNSUPPORTED : 0;
                else if ((code == QECMC_TORIC && L <= 5) || (code == QECMC_PLANAR && L <= 7) || (odd_code && L <= 11)) expect = 0;
                if (cp.plan.refusal.code != expect) {
                    std::fprintf(stderr, "code %d L %d lds_width %d: refusal %d (%s), expected %d\n", code, L, lds_width, cp.plan.refusal.code, cp.plan.refusal.msg.c_str(), expect);
                    rc = 1;
                }
                if (cp.plan.refusal.code) continue;
                std::printf("code %d L %d lds_width %d: full width %d, %d held, width %d, %d ops\n", code, L, lds_width, cp.full_width, cp.n_held, cp.plan.width, cp.plan.n_ops);
                rc |= check_plan(cp, lds_width);
                if (lds_width == 6 && cp.full_width <= 10) { rc |= check_twin(cp); ++twins; }
                if (lds_width == 13 && cp.full_width <= 8) { rc |= check_twin(cp); ++twins; }
            }
    for (const int bad : {-1, 1, 15, 99}) rc |= sweep::build_cut_plan(QECMC_XZZX, 3, bad).plan.refusal.code != QECMC_ERR_INVALID;
    rc |= twins < 6;
    std::printf(rc ? "class sweep cut selftest FAILED\n" : "class sweep cut selftest OK\n");
    return rc;
}
