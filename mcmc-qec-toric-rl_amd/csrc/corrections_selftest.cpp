// Stand-alone check of corrections.hpp for the sanitizers (make corrections_asan: -fsanitize=address,undefined): builds the class-move table of every
// (code, L) check_code_L() accepts and checks WHICH have none (exactly the toric code at even L); then, for the four codes at several sizes, corrects
// random candidates (K = 1 and K = 3, both settings of place and descend) towards every class -- and towards classes that do not exist -- through
// correct_body(), the body the kernel runs, and checks every chain: its syndrome (formed here from the generator table) is the candidates', its class
// is the target, the weight is its error count; an out-of-range target gives the zero chain, weight -1, and leaves its neighbours alone.
// Exit status 0: all held.
#include "corrections.hpp"
#include "plan_host.hpp"

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

// one bit per generator: set iff an odd number of its sites hold another non-identity Pauli
void syndrome_of(const correct::Table &t, const uint8_t *chain, uint8_t *bits)
{
    for (int g = 0; g < t.n_gen; ++g) {
        int v = 0;
        for (int u = 0; u < 4; ++u) {
            const uint32_t e = (u < 2 ? t.gen[2 * (size_t)g] >> (16 * u) : t.gen[2 * (size_t)g + 1] >> (16 * (u - 2))) & 0xFFFFu;
            if (e & 3u) v ^= chain[e >> 2] != 0 && chain[e >> 2] != (e & 3u);
        }
        bits[g] = (uint8_t)v;
    }
}

int class_of_bytes(const correct::Table &t, const uint8_t *chain)
{
    std::vector<uint32_t> words((size_t)t.W, 0u);
    for (int q = 0; q < t.nq; ++q) words[(size_t)(q >> 4)] |= (uint32_t)(chain[q] & 3u) << ((q & 15) * 2);
    lift::HostState st{words.data()};
    return correct::class_of(st, t.code, t.L, t.W);
}

int check(int code, int L)
{
    const correct::Table t = correct::build_table(code, L);
    if (t.need.empty()) { std::fprintf(stderr, "code %d L %d: no class-move table\n", code, L); return 1; }
    const uint64_t N = 48;
    int fails = 0;
    for (uint32_t K : {1u, 3u}) {
        std::vector<uint8_t> cand(N * K * t.nq, 0), out(N * t.nq), moved(N), status(N), s_in((size_t)t.n_gen), s_out((size_t)t.n_gen);
        std::vector<int32_t> target(N), weight(N), source(N);
        for (uint64_t s = 0; s < N; ++s) {
            uint8_t *c0 = &cand[s * K * t.nq];
            for (int q = 0; q < t.nq; ++q) {
                const bool idle = code == QECMC_PLANAR && q >= L * L && ((q - L * L) / L == L - 1 || (q - L * L) % L == L - 1);
                if (!idle && s > 0 && draw() < 0x26666666u) c0[q] = (uint8_t)(1 + draw() % 3);
            }
            for (uint32_t k = 1; k < K; ++k) {                          // the same syndrome: a few generators and logical operators on top
                uint8_t *ck = c0 + (size_t)k * t.nq;
                for (int q = 0; q < t.nq; ++q) ck[q] = c0[q];
                for (int n = 0; n < 4; ++n) {
                    const int g = (int)(draw() % (uint32_t)t.n_gen);
                    for (int u = 0; u < 4; ++u) {
                        const uint32_t e = (u < 2 ? t.gen[2 * (size_t)g] >> (16 * u) : t.gen[2 * (size_t)g + 1] >> (16 * (u - 2))) & 0xFFFFu;
                        if (e & 3u) ck[e >> 2] ^= (uint8_t)(e & 3u);
                    }
                }
                const int kind = (int)(draw() % (uint32_t)t.kinds), p = (int)(draw() % (uint32_t)L);
                for (int q = 0; q < t.nq; ++q) ck[q] ^= (uint8_t)((t.masks[((size_t)kind * (L + 1) + p) * t.W + (q >> 4)] >> ((q & 15) * 2)) & 3u);
            }
            target[s] = (int32_t)(s % (uint64_t)t.ncls);
        }
        target[5] = -1; target[17] = t.ncls; target[29] = 0x7FFFFFFF;
        for (int place = 0; place < 2; ++place)
            for (int descend = 0; descend < 2; ++descend) {
                correct::corrections_host(t, N, K, cand.data(), target.data(), place, descend, out.data(), weight.data(), source.data(), moved.data(), status.data());
                for (uint64_t s = 0; s < N; ++s) {
                    const uint8_t *o = &out[s * t.nq];
                    int n = 0;
                    for (int q = 0; q < t.nq; ++q) n += o[q] != 0;
                    const bool refused = target[s] < 0 || target[s] >= t.ncls;
                    if ((status[s] != 0) != refused) { ++fails; continue; }
                    if (refused) { fails += n != 0 || weight[s] != -1 || source[s] != -1 || moved[s] != 0; continue; }
                    fails += weight[s] != n || source[s] < 0 || source[s] >= (int)K;
                    fails += class_of_bytes(t, o) != target[s];
                    syndrome_of(t, &cand[s * K * t.nq], s_in.data());
                    syndrome_of(t, o, s_out.data());
                    for (int g = 0; g < t.n_gen; ++g) fails += s_in[(size_t)g] != s_out[(size_t)g];
                }
            }
    }
    if (fails) std::fprintf(stderr, "code %d L %d: %d checks failed\n", code, L, fails);
    return fails != 0;
}

}  // namespace

int main()
{
    int rc = 0;
    // which (code, L) have no class move: the toric code at even L, nothing else
    for (int code = 0; code < 4; ++code)
        for (int L = 2; L <= 64; ++L) {
            if (check_code_L(code, L).code) continue;
            const bool none = correct::build_table(code, L).need.empty(), expect = code == QECMC_TORIC && L % 2 == 0;
            if (none != expect) { std::fprintf(stderr, "code %d L %d: class-move table %s\n", code, L, none ? "missing" : "unexpected"); rc = 1; }
        }
    for (int code = 0; code < 4; ++code)
        for (int L : {3, 5, 7}) rc |= check(code, L);
    rc |= check(QECMC_TORIC, 15) | check(QECMC_ROTATED, 21) | check(QECMC_PLANAR, 4);
    std::printf(rc ? "corrections selftest FAILED\n" : "corrections selftest OK\n");
    return rc;
}
