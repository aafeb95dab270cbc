// Stand-alone check of syndrome_lift.hpp for the sanitizers (make lift_asan: -fsanitize=address,undefined): builds the lift table of every code at
// several sizes, lifts random syndromes -- and a few that are none -- with and without the greedy descent through lift_body(), the body the kernel
// runs, and checks every chain: its syndrome (formed here from the generator table: a generator's cell is set iff an odd number of its sites hold
// another non-identity Pauli) is the one that went in, the weight is the chain's error count, the descent never raises it.  Exit status 0: all held.
#include "syndrome_lift.hpp"

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

void syndrome_of(const lift::Table &t, const uint8_t *chain, uint8_t *cells)
{
    for (int c = 0; c < t.n_cells; ++c) cells[c] = 0;
    for (int g = 0; g < t.n_gen; ++g) {
        int v = 0;
        for (int u = 0; u < 4; ++u) {
            const uint32_t e = (u < 2 ? t.gen[2 * (size_t)g] >> (16 * u) : t.gen[2 * (size_t)g + 1] >> (16 * (u - 2))) & 0xFFFFu;
            if (e & 3u) v ^= chain[e >> 2] != 0 && chain[e >> 2] != (e & 3u);
        }
        cells[lift::generator_cell(t.code, t.L, g)] = (uint8_t)v;
    }
}

int check(int code, int L)
{
    const lift::Table t = lift::build_table(code, L);
    if (t.rows.empty()) { std::fprintf(stderr, "code %d L %d: no table\n", code, L); return 1; }
    const uint64_t N = 64;
    std::vector<uint8_t> err(N * t.nq, 0), defects(N * t.n_cells, 0), back((size_t)t.n_cells), status(N);
    std::vector<uint8_t> plain(N * t.nq), low(N * t.nq);
    std::vector<int32_t> w_plain(N), w_low(N);
    const uint32_t thr[3] = {0x0CCCCCCCu, 0x26666666u, 0x66666666u};          // site probabilities 0.05, 0.15, 0.4
    for (uint64_t s = 1; s < N; ++s) {                                        // (syndrome 0 stays empty)
        for (int q = 0; q < t.nq; ++q) {
            const bool idle = code == QECMC_PLANAR && q >= L * L && ((q - L * L) / L == L - 1 || (q - L * L) % L == L - 1);
            if (!idle && draw() < thr[s % 3]) err[s * t.nq + q] = (uint8_t)(1 + draw() % 3);
        }
        syndrome_of(t, &err[s * t.nq], &defects[s * t.n_cells]);
    }
    // two that are no syndromes: a single defect on the torus (odd parity), a set cell that is no check elsewhere
    int bad = -1;
    for (int c = 0; c < t.n_cells && bad < 0; ++c)
        if ((code == QECMC_TORIC) == (t.rows[(size_t)c * (t.W + 1) + t.W] != 0u)) bad = c;
    if (bad >= 0) defects[5 * (size_t)t.n_cells + bad] ^= 1;
    lift::chains_from_syndromes_host(t, N, defects.data(), 0, plain.data(), status.data(), w_plain.data());
    lift::chains_from_syndromes_host(t, N, defects.data(), 1, low.data(), nullptr, w_low.data());
    int fails = 0;
    for (uint64_t s = 0; s < N; ++s) {
        const bool refused = bad >= 0 && s == 5;
        if ((status[s] != 0) != refused) { ++fails; continue; }
        for (const std::vector<uint8_t> *ch : {&plain, &low}) {
            int n = 0;
            for (int q = 0; q < t.nq; ++q) n += (*ch)[s * t.nq + q] != 0;
            const int32_t w = ch == &plain ? w_plain[s] : w_low[s];
            if (refused) { fails += n != 0 || w != -1; continue; }
            syndrome_of(t, &(*ch)[s * t.nq], back.data());
            for (int c = 0; c < t.n_cells; ++c) fails += back[(size_t)c] != (defects[s * t.n_cells + c] != 0);
            fails += w != n;
        }
        fails += w_low[s] > w_plain[s];
    }
    if (fails) std::fprintf(stderr, "code %d L %d: %d checks failed\n", code, L, fails);
    return fails != 0;
}

}  // namespace

int main()
{
    int rc = 0;
    for (int code = 0; code < 4; ++code)
        for (int L : {3, 5, 7}) rc |= check(code, L);
    rc |= check(QECMC_TORIC, 4) | check(QECMC_TORIC, 15) | check(QECMC_ROTATED, 21) | check(QECMC_PLANAR, 4);
    std::printf(rc ? "syndrome_lift selftest FAILED\n" : "syndrome_lift selftest OK\n");
    return rc;
}
