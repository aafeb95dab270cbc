// Stand-alone check of enumerate.hpp for the sanitizers (make enumerate_asan: -fsanitize=address,undefined): builds the table of every (code, L) in
// [2, 64] -- accepted or refused -- and checks WHICH are accepted; then, for every accepted (code, L) up to rank 16, runs the twin on random chains and
// checks that the representative of class c lies in class c, that every class sums to 2^rank, that partial histograms over a split of the chunks (and
// over chunk widths) add up to the whole, that a stabilizer away the histogram is the same, and that a range past the last chunk is refused.
// Exit status 0: all held.
#include "enumerate.hpp"

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

int class_of_planes(const enumr::Table &t, uint32_t x, uint32_t z)
{
    uint32_t words[(enumr::kMaxQubits + 15) / 16] = {};
    for (int q = 0; q < t.nq; ++q) {
        const uint32_t xb = (x >> q) & 1u, zb = (z >> q) & 1u, f = zb ? (xb ? 2u : 3u) : xb;
        words[q >> 4] |= f << ((q & 15) * 2);
    }
    lift::HostState st{words};
    return correct::class_of(st, t.code, t.L, t.W);
}

int check(const enumr::Table &t)
{
    const uint64_t N = 6;
    const size_t per = (size_t)t.ncls * (size_t)(t.nq + 1) * (size_t)(t.nq + 1);
    int fails = 0;
    std::vector<uint8_t> chains(N * t.nq, 0);
    for (uint64_t s = 1; s < N; ++s)
        for (int q = 0; q < t.nq; ++q) {
            const bool idle = t.code == QECMC_PLANAR && q >= t.L * t.L && ((q - t.L * t.L) / t.L == t.L - 1 || (q - t.L * t.L) % t.L == t.L - 1);
            if (!idle && draw() < 0x40000000u) chains[s * t.nq + q] = (uint8_t)(1 + draw() % 3);
        }
    std::vector<uint32_t> reps((size_t)t.ncls * 2);
    for (uint64_t s = 0; s < N; ++s) {
        const int a = enumr::class_representatives(t, &chains[s * t.nq], reps.data());
        for (int c = 0; c < t.ncls; ++c) fails += class_of_planes(t, reps[(size_t)2 * c], reps[(size_t)2 * c + 1]) != c;
        fails += a < 0 || a >= t.ncls;
    }
    int bits = 0;
    uint64_t count = 0;
    fails += enumr::resolve_range(t, bits, 0, count).code != 0 || bits != t.rank || count != 1;
    std::vector<uint64_t> whole(N * per), part(N * per), sum(N * per, 0);
    std::vector<int32_t> cls(N);
    enumr::enumerate_host(t, N, chains.data(), bits, 0, count, whole.data(), cls.data());
    for (uint64_t s = 0; s < N; ++s)
        for (int c = 0; c < t.ncls; ++c) {
            uint64_t total = 0;
            for (size_t i = 0; i < per / (size_t)t.ncls; ++i) total += whole[s * per + (size_t)c * (per / (size_t)t.ncls) + i];
            fails += total != 1ull << t.rank;
        }
    // chunks of 2^8 elements, in three uneven ranges
    bits = 8; count = 0;
    fails += enumr::resolve_range(t, bits, 0, count).code != 0 || count != 1ull << (t.rank - 8);
    const uint64_t n_chunks = count, cut[4] = {0, n_chunks / 3, n_chunks / 3 + 1 < n_chunks ? n_chunks / 3 + 1 : n_chunks, n_chunks};
    for (int r = 0; r < 3; ++r) {
        if (cut[r] == cut[r + 1]) continue;
        enumr::enumerate_host(t, N, chains.data(), 8, cut[r], cut[r + 1] - cut[r], part.data(), nullptr);
        for (size_t i = 0; i < sum.size(); ++i) sum[i] += part[i];
    }
    for (size_t i = 0; i < sum.size(); ++i) fails += sum[i] != whole[i];
    int b2 = 8;
    uint64_t c2 = 1;
    fails += enumr::resolve_range(t, b2, n_chunks, c2).code != QECMC_ERR_INVALID;          // past the last chunk
    b2 = 8; c2 = 2;
    fails += enumr::resolve_range(t, b2, n_chunks - 1, c2).code != QECMC_ERR_INVALID;
    b2 = 7; c2 = 0;
    fails += enumr::resolve_range(t, b2, 0, c2).code != QECMC_ERR_INVALID;
    b2 = 31; c2 = 0;
    fails += enumr::resolve_range(t, b2, 0, c2).code != QECMC_ERR_INVALID;
    // a stabilizer away: the same histogram
    for (uint64_t s = 0; s < N; ++s) {
        uint32_t x, z;
        enumr::product_planes(t, 0, draw() & ((1ull << t.rank) - 1), x, z);
        for (int q = 0; q < t.nq; ++q) {
            const uint32_t xb = (x >> q) & 1u, zb = (z >> q) & 1u;
            chains[s * t.nq + q] ^= (uint8_t)(zb ? (xb ? 2u : 3u) : xb);
        }
    }
    enumr::enumerate_host(t, N, chains.data(), t.rank, 0, 1, part.data(), nullptr);
    for (size_t i = 0; i < whole.size(); ++i) fails += part[i] != whole[i];
    if (fails) std::fprintf(stderr, "code %d L %d: %d checks failed\n", t.code, t.L, fails);
    return fails != 0;
}

}  // namespace

int main()
{
    int rc = 0, checked = 0;
    for (int code = -1; code <= 4; ++code)
        for (int L = 1; L <= 65; ++L) {
            const enumr::Table t = enumr::build_table(code, L);
            const bool odd_code = code == QECMC_XZZX || code == QECMC_ROTATED;
            const int expect = code < 0 || code > 3 || L < 2 || L > 64 || (odd_code && L % 2 == 0) ? QECMC_ERR_INVALID
                               : (code == QECMC_TORIC && L == 3) || (code == QECMC_PLANAR && (L == 3 || L == 4)) || (odd_code && (L == 3 || L == 5)) ? 0
                               : QECMC_ERR_UNSUPPORTED;
            if (t.refusal.code != expect) { std::fprintf(stderr, "code %d L %d: refusal %d, expected %d\n", code, L, t.refusal.code, expect); rc = 1; }
            if (t.refusal.code == 0) {
                const int want = code == QECMC_TORIC ? 2 * L * L - 2 : code == QECMC_PLANAR ? 2 * L * (L - 1) : L * L - 1;
                if (t.rank != want) { std::fprintf(stderr, "code %d L %d: rank %d, expected %d\n", code, L, t.rank, want); rc = 1; }
                if (t.rank <= 16) { rc |= check(t); ++checked; }
            }
        }
    rc |= checked != 4;
    std::printf(rc ? "enumerate selftest FAILED\n" : "enumerate selftest OK\n");
    return rc;
}
