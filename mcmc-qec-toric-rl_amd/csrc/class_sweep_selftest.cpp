// Stand-alone check of class_sweep.hpp for the sanitizers (make sweep_asan: -fsanitize=address,undefined): builds the plan of every (code, L) in
// [1, 65] -- accepted or refused -- and checks WHICH are accepted and that the width of an accepted plan fits lds_carve(); then, for every accepted
// plan up to width 10, runs the twin on random chains and checks that the representative of class c lies in class c, that all-ones weights give
// exactly 2^rank in every class, that a generator away Z is the same to the last bit of a relative 1e-12, and that bad weights are refused.
// Exit status 0: all held.
#include "class_sweep.hpp"

#include <cstdio>
#include <cstdlib>

using namespace qecmc;

namespace {

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t draw()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

int check(const sweep::Plan &p)
{
    const uint64_t N = 5;
    int fails = 0;
    const correct::Table ct = correct::build_table(p.code, p.L);
    std::vector<uint8_t> chains(N * p.nq, 0);
    for (uint64_t s = 1; s < N; ++s)
        for (int q = 0; q < p.nq; ++q) {
            const bool idle = p.code == QECMC_PLANAR && q >= p.L * p.L && ((q - p.L * p.L) / p.L == p.L - 1 || (q - p.L * p.L) % p.L == p.L - 1);
            if (!idle && draw() < 0x40000000u) chains[s * p.nq + q] = (uint8_t)(1 + draw() % 3);
        }
    std::vector<uint32_t> reps((size_t)p.ncls * p.W);
    for (uint64_t s = 0; s < N; ++s) {
        const int a = sweep::class_representatives(p, &chains[s * p.nq], reps.data());
        fails += a < 0 || a >= p.ncls;
        for (int c = 0; c < p.ncls; ++c) {
            lift::HostState st{&reps[(size_t)c * p.W]};
            fails += correct::class_of(st, p.code, p.L, p.W) != c;
        }
    }
    std::vector<double> ones(N * p.ncls), z(N * p.ncls), z2(N * p.ncls);
    std::vector<int32_t> cls(N), cls2(N);
    const double w1[4] = {1.0, 1.0, 1.0, 1.0}, w[4] = {1.0, 0.031, 0.017, 0.29};
    sweep::sweep_host(p, N, chains.data(), w1, ones.data(), cls.data());
    for (size_t i = 0; i < ones.size(); ++i) fails += ones[i] != std::ldexp(1.0, p.rank);
    sweep::sweep_host(p, N, chains.data(), w, z.data(), nullptr);
    // a few generators away: the same classes, the same Z
    for (uint64_t s = 0; s < N; ++s)
        for (int k = 0; k < 5; ++k) {
            const int g = (int)(draw() % (uint32_t)p.n_gen);
            for (int i = 0; i < 4; ++i) {
                const uint32_t e = (ct.gen[(size_t)(2 * g + (i >> 1))] >> ((i & 1) * 16)) & 0xFFFFu, pauli = e & 3u, site = e >> 2;
                if (pauli) chains[s * p.nq + site] ^= (uint8_t)pauli;           // (byte values XOR as the Pauli product)
            }
        }
    sweep::sweep_host(p, N, chains.data(), w, z2.data(), cls2.data());
    for (size_t i = 0; i < z.size(); ++i) fails += !(z[i] > 0.0) || std::fabs(z2[i] - z[i]) > 1e-12 * z[i];
    for (uint64_t s = 0; s < N; ++s) fails += cls[s] != cls2[s];
    if (fails) std::fprintf(stderr, "code %d L %d: %d checks failed\n", p.code, p.L, fails);
    return fails != 0;
}

}  // namespace

int main()
{
    int rc = 0, checked = 0;
    for (int code = -1; code <= 4; ++code)
        for (int L = 1; L <= 65; ++L) {
            const sweep::Plan p = sweep::build_plan(code, L);
            const bool odd_code = code == QECMC_XZZX || code == QECMC_ROTATED;
            const int expect = code < 0 || code > 3 || L < 2 || L > 64 || (odd_code && L % 2 == 0) ? QECMC_ERR_INVALID
                               : (code == QECMC_TORIC && L == 3) || (code == QECMC_PLANAR && L <= 6) || (odd_code && L <= 9) ? 0
                               : QECMC_ERR_UNSUPPORTED;
            if (p.refusal.code != expect) { std::fprintf(stderr, "code %d L %d: refusal %d (%s), expected %d\n", code, L, p.refusal.code, p.refusal.msg.c_str(), expect); rc = 1; }
            if (p.refusal.code == 0) {
                const int want = code == QECMC_TORIC ? 2 * L * L - 2 : code == QECMC_PLANAR ? 2 * L * (L - 1) : L * L - 1;
                if (p.rank != want) { std::fprintf(stderr, "code %d L %d: rank %d, expected %d\n", code, L, p.rank, want); rc = 1; }
                if (p.width > sweep::kMaxWidth || p.carve.bytes > sweep::kLdsBudget || (int)p.ops.size() != p.n_ops * sweep::kOpWords) rc = 1;
                std::printf("code %d L %d: width %d, %d ops\n", code, L, p.width, p.n_ops);
                if (p.width <= 10) { rc |= check(p); ++checked; }
            }
        }
    const double bad[5][4] = {{1, 0, 1, 1}, {1, 1, -1, 1}, {1, 1, 1, NAN}, {INFINITY, 1, 1, 1}, {1, 1, 1, 1}};
    for (int i = 0; i < 5; ++i) rc |= (sweep::check_weights(bad[i]).code != 0) != (i < 4);
    rc |= checked < 6;
    std::printf(rc ? "class sweep selftest FAILED\n" : "class sweep selftest OK\n");
    return rc;
}
