// Stand-alone check of class_sample.hpp for the sanitizers (make sample_asan: -fsanitize=address,undefined): builds the sample plan of every
// (code, L) with L in [1, 13] under lds_width 0, 13, 14 and a narrow one and checks it against build_cut_plan -- the same refusals behind the entry
// point's name, the same op stream, every generator held or retired exactly once --; the launch group against its bounds; then, for every plan that
// is cheap enough, runs the twin in both modes and under a site table with its outputs in heap blocks of their exact size, poisoned: z is
// sweep_cut_host's bits, every sample commutes with every generator exactly where the input does not (the syndrome) and lies in its class, the
// posterior's sample (s, k) is sample (s, cls[s, k], k) of the every-class mode, constant rows give the uniform form's bytes, and one job repeated by
// hand over POISONED scratch and a POISONED record of their exact size walks to f == 0 and to the twin's chain.  Exit status 0: all held.
#include "class_sample.hpp"

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

// the generator table as byte chains, and the cells that hold a qubit
void generator_bytes(const sweep::Plan &p, std::vector<std::vector<uint8_t>> &gen, std::vector<char> &touched)
{
    const correct::Table ct = correct::build_table(p.code, p.L);
    gen.assign((size_t)p.n_gen, std::vector<uint8_t>((size_t)p.nq, 0));
    touched.assign((size_t)p.nq, 0);
    for (int g = 0; g < p.n_gen; ++g)
        for (int i = 0; i < 4; ++i) {
            const uint32_t e = (ct.gen[(size_t)(2 * g + (i >> 1))] >> ((i & 1) * 16)) & 0xFFFFu, pauli = e & 3u, site = e >> 2;
            if (pauli) { gen[(size_t)g][site] ^= (uint8_t)pauli; touched[site] = 1; }
        }
}

// bit g: the chain anticommutes with generator g
std::vector<char> syndrome(const std::vector<std::vector<uint8_t>> &gen, const uint8_t *chain, int nq)
{
    std::vector<char> s(gen.size(), 0);
    for (size_t g = 0; g < gen.size(); ++g)
        for (int q = 0; q < nq; ++q) s[g] ^= (char)(gen[g][(size_t)q] && (chain[q] & 3u) && gen[g][(size_t)q] != (chain[q] & 3u));
    return s;
}

int class_of_bytes(const sweep::Plan &p, const uint8_t *chain)
{
    std::vector<uint32_t> words((size_t)p.W, 0u);
    for (int q = 0; q < p.nq; ++q) words[(size_t)(q >> 4)] |= (uint32_t)(chain[q] & 3u) << ((q & 15) * 2);
    lift::HostState st{words.data()};
    return correct::class_of(st, p.code, p.L, p.W);
}

int check_plan(int code, int L, int lds_width)
{
    const sweep::CutPlan cp = sweep::build_cut_plan(code, L, lds_width);
    const sample::SamplePlan sp = sample::build_sample_plan(code, L, lds_width, "qecmc_class_sample_site");
    const sweep::Plan &p = sp.cut.plan;
    if (p.refusal.code != cp.plan.refusal.code) return 1;
    if (cp.plan.refusal.code) return p.refusal.msg != "qecmc_class_sample_site: " + cp.plan.refusal.msg;
    int fails = p.ops != cp.plan.ops || sp.cut.held != cp.held || sp.cut.held_words != cp.held_words;
    fails += sp.n_forget != p.n_gen - cp.n_held || (int)sp.forget_gen.size() != sp.n_forget || sp.forget_words.size() != (size_t)sp.n_forget * p.W;
    std::vector<int> seen((size_t)p.n_gen, 0);
    for (const int g : cp.held) ++seen[(size_t)g];
    for (const int g : sp.forget_gen) ++seen[(size_t)g];
    for (const int n : seen) fails += n != 1;
    const uint64_t per = sample::sample_bytes_per_job(sp);
    fails += per != ((uint64_t)sp.n_forget << (p.width - 1)) * 16u;
    for (const uint64_t N : {0ull, 1ull, 7ull, 600ull, 5000ull, 1ull << 32})
        for (const uint64_t K : {1ull, 70ull, 4096ull, 0xFFFFFFFFull}) {
            const sample::LaunchGroup g = sample::sample_launch_group(N, p.ncls, cp.n_held, K, per);
            fails += g.syndromes < 1 || g.syndromes > sweep::cut_launch_group(N, p.ncls, cp.n_held) || g.k_chunk < 1 || g.k_chunk > K || g.jobs < 1;
            fails += (uint64_t)g.jobs * per > sample::kSampleWorkspaceBytes || (uint64_t)g.syndromes * p.ncls * g.k_chunk > sample::kLaunchSamples;
            fails += cp.n_held == 0 && g.jobs != g.syndromes * (uint32_t)p.ncls;
        }
    if (fails) std::fprintf(stderr, "code %d L %d lds_width %d: %d plan checks failed\n", code, L, lds_width, fails);
    return fails != 0;
}

int check_twin(const sample::SamplePlan &sp)
{
    const sweep::CutPlan &cp = sp.cut;
    const sweep::Plan &p = cp.plan;
    const uint64_t N = 3, K = 5, seed = 0xC0FFEE1234ull;
    const uint32_t first = 0xFFFFFFF0u;
    int fails = 0;
    std::vector<std::vector<uint8_t>> gen;
    std::vector<char> touched;
    generator_bytes(p, gen, touched);
    std::vector<uint8_t> chains(N * p.nq, 0);
    for (uint64_t s = 1; s < N; ++s)
        for (int q = 0; q < p.nq; ++q)
            if (touched[(size_t)q] && draw() < (s == 1 ? 0x10000000u : 0x50000000u)) chains[s * p.nq + q] = (uint8_t)(1 + draw() % 3);
    const double w4[4] = {1.0, 0.031, 0.017, 0.12};
    const size_t n_all = (size_t)N * p.ncls * K * p.nq, n_post = (size_t)N * K * p.nq;
    // outputs at their exact size, poisoned
    uint8_t *all = new uint8_t[n_all], *post = new uint8_t[n_post], *site = new uint8_t[n_post];
    int32_t *cls = new int32_t[N * K], *cls_site = new int32_t[N * K];
    double *z = new double[N * p.ncls], *z_post = new double[N * p.ncls], *z_want = new double[N * p.ncls];
    std::memset(all, 0xEE, n_all); std::memset(post, 0xEE, n_post); std::memset(site, 0xEE, n_post);
    std::memset(cls, 0xEE, N * K * sizeof(int32_t)); std::memset(cls_site, 0xEE, N * K * sizeof(int32_t));
    fails += sample::sample_host(sp, "t", N, chains.data(), w4, nullptr, 0, K, seed, first, 0, all, nullptr, z, 4).code != 0;
    fails += sample::sample_host(sp, "t", N, chains.data(), w4, nullptr, 0, K, seed, first, 1, post, cls, z_post, 1).code != 0;
    std::vector<double> rows((size_t)N * p.nq * 4);
    for (size_t i = 0; i < rows.size(); ++i) rows[i] = w4[i & 3u];
    fails += sample::sample_host(sp, "t", N, chains.data(), nullptr, rows.data(), N, K, seed, first, 1, site, cls_site, z_want, 2).code != 0;
    fails += std::memcmp(site, post, n_post) != 0 || std::memcmp(cls, cls_site, N * K * sizeof(int32_t)) != 0;            // constant rows: the uniform form's bytes
    sweep::sweep_cut_host(cp, N, chains.data(), w4, z_want, nullptr, 3);
    fails += std::memcmp(z, z_want, N * p.ncls * sizeof(double)) != 0 || std::memcmp(z_post, z_want, N * p.ncls * sizeof(double)) != 0;
    for (uint64_t s = 0; s < N; ++s) {
        const std::vector<char> syn = syndrome(gen, chains.data() + s * p.nq, p.nq);
        for (int c = 0; c < p.ncls; ++c)
            for (uint64_t k = 0; k < K; ++k) {
                const uint8_t *mine = all + ((s * p.ncls + c) * K + k) * p.nq;
                for (int q = 0; q < p.nq; ++q) fails += mine[q] > 3;
                fails += syndrome(gen, mine, p.nq) != syn || class_of_bytes(p, mine) != c;
            }
        for (uint64_t k = 0; k < K; ++k) {
            const int32_t c = cls[s * K + k];
            if (c < 0 || c >= p.ncls) { ++fails; continue; }
            fails += std::memcmp(post + (s * K + k) * p.nq, all + ((s * p.ncls + c) * K + k) * p.nq, (size_t)p.nq) != 0;
        }
    }
    // one job by hand: partials, pick, record and walk over poisoned scratch of the exact size
    double wxz[4];
    sweep::weights_xz(w4, wxz);
    const sample::Factors fc{wxz, 0u};
    std::vector<uint32_t> reps((size_t)p.ncls * p.W), rep((size_t)p.W);
    std::vector<uint8_t> bytes((size_t)p.nq);
    const uint64_t s = N - 1, k = K - 1;
    const int c = p.ncls - 1;
    sweep::class_representatives(p, chains.data() + s * p.nq, reps.data());
    sweep::Plan unscaled = p;
    unscaled.scale = 1.0;
    double *A = new double[(size_t)1 << p.width];
    sample::PairRecord *R = new sample::PairRecord[(size_t)sample::sample_pairs_per_job(sp.n_forget, p.width)];
    std::memset(A, 0xEE, ((size_t)1 << p.width) * sizeof(double));
    std::memset(R, 0xEE, (size_t)sample::sample_bytes_per_job(sp));
    std::vector<double> P((size_t)1 << cp.n_held);
    for (uint32_t h = 0; h < (1u << cp.n_held); ++h) {
        sweep::cut_representative(cp, &reps[(size_t)c * p.W], h, rep.data());
        P[h] = sweep::sweep_one(unscaled, rep.data(), wxz, A);
    }
    const uint32_t pick = cp.n_held ? sample::pick_running(P.data(), 1u << cp.n_held, sample::draw_u53(k, 0u, 0u, first + (uint32_t)s, (uint32_t)c, seed)) : 0u;
    sweep::cut_representative(cp, &reps[(size_t)c * p.W], pick, rep.data());
    fails += sample::record_one(sp, rep.data(), fc, A, R) != P[pick];
    fails += sample::sample_walk(sp, R, k, first + (uint32_t)s, (uint32_t)c, seed, rep.data()) != 0u;
    minplus::unpack_chain(rep.data(), p.nq, bytes.data());
    fails += std::memcmp(bytes.data(), all + ((s * p.ncls + c) * K + k) * p.nq, (size_t)p.nq) != 0;
    delete[] A; delete[] R;
    delete[] all; delete[] post; delete[] site; delete[] cls; delete[] cls_site; delete[] z; delete[] z_post; delete[] z_want;
    if (fails) std::fprintf(stderr, "code %d L %d lds_width %d: %d twin checks failed\n", p.code, p.L, cp.lds_width, fails);
    return fails != 0;
}

}  // namespace

int main()
{
    int rc = 0, twins = 0, held = 0;
    const int Ls[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 33, 64, 65};
    for (int code = -1; code <= 4; ++code)
        for (const int L : Ls)
            for (const int lds_width : {0, 13, 14, 6}) {
                if (L > 13 && lds_width != 0) continue;
                rc |= check_plan(code, L, lds_width);
                const sample::SamplePlan sp = sample::build_sample_plan(code, L, lds_width);
                if (sp.cut.plan.refusal.code) continue;
                // cheap enough here: the narrow plans of the small shapes (held generators), and every plan that holds nothing up to width 11
                const bool narrow = lds_width == 6 && sp.cut.full_width <= 10, plain = lds_width == 0 && sp.cut.n_held == 0 && sp.cut.plan.width <= 11;
                if (narrow || plain) {
                    std::printf("code %d L %d lds_width %d: %d held, width %d, %d FORGETs, %llu bytes per job\n", code, L, lds_width, sp.cut.n_held, sp.cut.plan.width, sp.n_forget,
                                (unsigned long long)sample::sample_bytes_per_job(sp));
                    rc |= check_twin(sp);
                    ++twins;
                    held += sp.cut.n_held > 0;
                }
            }
    const double neg[4] = {1.0, -0.1, 0.1, 0.1}, zero[4] = {0.0, 0.0, 0.0, 0.0}, ok[4] = {1.0, 0.0, 0.0, 0.5};
    rc |= sample::check_sample_weights("n", neg).code != QECMC_ERR_INVALID || sample::check_sample_weights("n", zero).code != QECMC_ERR_INVALID ||
          sample::check_sample_weights("n", ok).code != 0;
    rc |= sample::check_sample_args("n", 1, 0, 0, 0).code != QECMC_ERR_INVALID || sample::check_sample_args("n", 1, 1ull << 32, 0, 0).code != QECMC_ERR_INVALID ||
          sample::check_sample_args("n", 2, 1, 0xFFFFFFFFu, 0).code != QECMC_ERR_INVALID || sample::check_sample_args("n", 1, 1, 0xFFFFFFFFu, 1).code != 0 ||
          sample::check_sample_args("n", 1, 1, 0, 2).code != QECMC_ERR_INVALID;
    const double z_bad[4] = {1.0, 0.0, 2.0, 3.0}, z_none[4] = {0.0, 0.0, 0.0, 0.0};
    rc |= sample::check_sample_z("n", 3, z_bad, 4, 0).code != QECMC_ERR_INVALID || sample::check_sample_z("n", 3, z_bad, 4, 1).code != 0 ||
          sample::check_sample_z("n", 3, z_none, 4, 1).code != QECMC_ERR_INVALID;
    const double one[3] = {0.0, 2.0, 0.0};
    rc |= sample::pick_running(one, 3, 0.0) != 1u || sample::pick_running(one, 3, 0.999) != 1u;     // a weight of 0 is never picked
    const double tiny[3] = {0.0, 0x1p-1074, 0.0}, u_top = 1.0 - 0x1p-53;                            // ... nor at the last positive double, where u * last rounds up to last
    rc |= sample::pick_running(tiny, 3, 0.0) != 1u || sample::pick_running(tiny, 3, 0.75) != 1u || sample::pick_running(tiny, 3, u_top) != 1u;
    const double z_low[4] = {1.0, 0x1p-962, 2.0, 3.0}, z_floor[4] = {0x1p-961, 0x1p-961, 0x1p-961, 0x1p-961}, z_under[4] = {0x1p-964, 0x1p-964, 0x1p-964, 0x1p-964};
    rc |= sample::check_sample_z("n", 3, z_low, 4, 0).code != QECMC_ERR_INVALID || sample::check_sample_z("n", 3, z_low, 4, 1).code != 0 ||
          sample::check_sample_z("n", 3, z_floor, 4, 0).code != 0 || sample::check_sample_z("n", 3, z_under, 4, 1).code != QECMC_ERR_INVALID;
    rc |= sample::check_sample_z("n", 3, z_low, 4, 0).msg.find("row 3, class 1") == std::string::npos || sample::check_sample_z("n", 3, z_low, 4, 0).msg.find("below 2^-960") == std::string::npos;
    rc |= twins < 12 || held < 2;
    std::printf(rc ? "class sample selftest FAILED\n" : "class sample selftest OK\n");
    return rc;
}
