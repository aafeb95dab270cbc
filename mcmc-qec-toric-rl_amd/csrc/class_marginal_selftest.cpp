// Stand-alone check of class_marginal.hpp for the sanitizers (make marginal_asan: -fsanitize=address,undefined): builds the marginal plan of every
// (code, L) with L in [1, 13] under lds_width 0, 13, 14 and a narrow one and checks it against build_cut_plan -- the same refusals behind the entry
// point's name, the same op stream, every cell that a generator touches closed exactly once --; the launch group against its bounds; then, for every
// plan that is cheap enough, runs the twin with its outputs in heap blocks of their exact size, poisoned: z is sweep_cut_host's bits, the four
// weights of every qubit total z within the rounding of the rule, a cell no CLOSE names holds z at the input's representative byte, constant rows
// give the uniform form's bytes, the result does not depend on the number of host threads, and one job repeated by hand over POISONED scratch and a
// POISONED record of their exact size gives sums that total its partial.  Exit status 0: all held.
#include "class_marginal.hpp"

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

bool near(double a, double b, double rtol) { return std::fabs(a - b) <= rtol * (a > b ? a : b); }

int check_plan(int code, int L, int lds_width)
{
    const sweep::CutPlan cp = sweep::build_cut_plan(code, L, lds_width);
    const marginal::MarginalPlan mp = marginal::build_marginal_plan(code, L, lds_width, "qecmc_class_marginals_site");
    const sweep::Plan &p = mp.cut.plan;
    if (p.refusal.code != cp.plan.refusal.code) return 1;
    if (cp.plan.refusal.code) return p.refusal.msg != "qecmc_class_marginals_site: " + cp.plan.refusal.msg;
    int fails = p.ops != cp.plan.ops || mp.cut.held != cp.held || mp.cut.held_words != cp.held_words;
    const std::vector<char> named = sweep::closed_qubits(p.ops, p.nq);
    fails += (int)mp.close_op.size() != mp.n_close || (int)mp.close_qubit.size() != mp.n_close || (int)mp.close_of.size() != p.nq || mp.n_close != p.n_qubits;
    for (int q = 0; q < p.nq; ++q) {
        const int32_t ci = mp.close_of[(size_t)q];
        fails += (ci >= 0) != (named[(size_t)q] != 0);
        if (ci >= 0) fails += ci >= mp.n_close || mp.close_qubit[(size_t)ci] != (uint32_t)q || p.ops[(size_t)mp.close_op[(size_t)ci] * sweep::kOpWords + 3] != (uint32_t)q;
    }
    for (int ci = 1; ci < mp.n_close; ++ci) fails += mp.close_op[(size_t)ci] <= mp.close_op[(size_t)ci - 1];
    const uint64_t per = marginal::marginal_bytes_per_job(mp);
    fails += per != ((uint64_t)mp.n_close << p.width) * 8u;
    const uint64_t jobs_per_syndrome = (uint64_t)p.ncls << cp.n_held;
    for (const uint64_t N : {0ull, 1ull, 7ull, 600ull, 5000ull, 1ull << 32}) {
        const marginal::LaunchGroup g = marginal::marginal_launch_group(N, p.ncls, cp.n_held, mp.n_close, per);
        fails += g.syndromes < 1 || g.syndromes > sweep::cut_launch_group(N, p.ncls, cp.n_held) || g.jobs < 1 || g.jobs > sweep::kCutGridMax;
        fails += (uint64_t)g.jobs * per > marginal::kMarginalWorkspaceBytes || g.jobs > g.syndromes * jobs_per_syndrome;
        fails += g.syndromes > 1 && g.syndromes * jobs_per_syndrome * marginal::marginal_fold_per_job(mp.n_close) * 8u > marginal::kMarginalFoldBytes;
    }
    if (fails) std::fprintf(stderr, "code %d L %d lds_width %d: %d plan checks failed\n", code, L, lds_width, fails);
    return fails != 0;
}

int check_twin(const marginal::MarginalPlan &mp)
{
    const sweep::CutPlan &cp = mp.cut;
    const sweep::Plan &p = cp.plan;
    const uint64_t N = 3;
    int fails = 0;
    const std::vector<char> named = sweep::closed_qubits(p.ops, p.nq);
    std::vector<uint8_t> chains(N * p.nq, 0);
    for (uint64_t s = 1; s < N; ++s)
        for (int q = 0; q < p.nq; ++q)
            if (named[(size_t)q] && draw() < (s == 1 ? 0x10000000u : 0x50000000u)) chains[s * p.nq + q] = (uint8_t)(1 + draw() % 3);
    const double w4[4] = {1.0, 0.031, 0.0, 0.12};                                // (a zero weight: allowed here)
    const size_t row = (size_t)p.nq * 4u, n_out = (size_t)N * p.ncls * row, n_z = (size_t)N * p.ncls;
    double *out = new double[n_out], *again = new double[n_out], *site = new double[n_out];
    double *z = new double[n_z], *z_again = new double[n_z], *z_site = new double[n_z], *z_want = new double[n_z];
    int32_t *cls = new int32_t[N];
    std::memset(out, 0xEE, n_out * sizeof(double)); std::memset(again, 0xEE, n_out * sizeof(double)); std::memset(site, 0xEE, n_out * sizeof(double));
    std::memset(z, 0xEE, n_z * sizeof(double)); std::memset(z_again, 0xEE, n_z * sizeof(double)); std::memset(z_site, 0xEE, n_z * sizeof(double));
    marginal::marginal_host(mp, N, chains.data(), w4, nullptr, 0, out, z, cls, 4);
    marginal::marginal_host(mp, N, chains.data(), w4, nullptr, 0, again, z_again, nullptr, 1);
    std::vector<double> rows((size_t)N * row);
    for (size_t i = 0; i < rows.size(); ++i) rows[i] = w4[i & 3u];
    marginal::marginal_host(mp, N, chains.data(), nullptr, rows.data(), N, site, z_site, nullptr, 3);
    fails += std::memcmp(out, again, n_out * sizeof(double)) != 0 || std::memcmp(z, z_again, n_z * sizeof(double)) != 0;       // whatever the threads
    fails += std::memcmp(out, site, n_out * sizeof(double)) != 0 || std::memcmp(z, z_site, n_z * sizeof(double)) != 0;         // constant rows: the uniform form's bytes
    const double positive[4] = {1.0, 0.031, 0.5, 0.12};
    {   // z against sweep_cut_host, which refuses a zero weight: under positive weights
        double *o2 = new double[n_out];
        marginal::marginal_host(mp, N, chains.data(), positive, nullptr, 0, o2, z_again, nullptr, 2);
        sweep::sweep_cut_host(cp, N, chains.data(), positive, z_want, nullptr, 3);
        fails += std::memcmp(z_again, z_want, n_z * sizeof(double)) != 0;
        delete[] o2;
    }
    const double rtol = 2.0 * (2.0 * p.n_ops + (double)((1u << p.width) / 64u) + cp.n_held + 20.0) * 0x1p-53;
    std::vector<uint32_t> reps((size_t)p.ncls * p.W);
    for (uint64_t s = 0; s < N; ++s) {
        fails += cls[s] != sweep::class_representatives(p, chains.data() + s * p.nq, reps.data());
        for (int c = 0; c < p.ncls; ++c) {
            const double Zc = z[s * p.ncls + c];
            for (int q = 0; q < p.nq; ++q) {
                const double *m = out + ((s * p.ncls + c) * (size_t)p.nq + (size_t)q) * 4u;
                for (int i = 0; i < 4; ++i) fails += !(m[i] >= 0.0) || !std::isfinite(m[i]);
                if (named[(size_t)q]) { fails += !near(m[0] + m[1] + m[2] + m[3], Zc, rtol) || m[2] != 0.0; continue; }
                const uint32_t here = (reps[(size_t)c * p.W + (size_t)(q >> 4)] >> ((q & 15) * 2)) & 3u;
                for (uint32_t i = 0; i < 4u; ++i) fails += m[i] != (i == here ? Zc : 0.0);
            }
        }
    }
    // one job by hand over poisoned scratch of the exact size: the four sums of every CLOSE total the partial
    double wxz[4];
    sweep::weights_xz(w4, wxz);
    const sample::Factors fc{wxz, 0u};
    std::vector<uint32_t> rep((size_t)p.W);
    sweep::class_representatives(p, chains.data() + (N - 1) * p.nq, reps.data());
    sweep::cut_representative(cp, &reps[(size_t)(p.ncls - 1) * p.W], (1u << cp.n_held) - 1u, rep.data());
    const size_t entries = (size_t)marginal::marginal_entries_per_job(mp.n_close, p.width);
    double *A = new double[(size_t)1 << p.width], *B = new double[(size_t)1 << p.width], *fwd = new double[entries], *Mh = new double[(size_t)mp.n_close * 4u];
    std::memset(A, 0xEE, ((size_t)1 << p.width) * sizeof(double)); std::memset(B, 0xEE, ((size_t)1 << p.width) * sizeof(double));
    std::memset(fwd, 0xEE, entries * sizeof(double)); std::memset(Mh, 0xEE, (size_t)mp.n_close * 4u * sizeof(double));
    const double partial = marginal::forward_one(mp, rep.data(), fc, A, fwd);
    marginal::backward_one(mp, rep.data(), fc, B, fwd, Mh);
    for (int ci = 0; ci < mp.n_close; ++ci) fails += !near(Mh[ci * 4] + Mh[ci * 4 + 1] + Mh[ci * 4 + 2] + Mh[ci * 4 + 3], partial, rtol);
    fails += !near(B[0], partial, rtol);                                         // the backward sweep ends where the forward one does
    delete[] A; delete[] B; delete[] fwd; delete[] Mh;
    delete[] out; delete[] again; delete[] site; delete[] z; delete[] z_again; delete[] z_site; delete[] z_want; delete[] cls;
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
                const marginal::MarginalPlan mp = marginal::build_marginal_plan(code, L, lds_width);
                if (mp.cut.plan.refusal.code) continue;
                // cheap enough here: the narrow plans of the small shapes (held generators), and every plan that holds nothing up to width 10
                const bool narrow = lds_width == 6 && mp.cut.full_width <= 10, plain = lds_width == 0 && mp.cut.n_held == 0 && mp.cut.plan.width <= 10;
                if (narrow || plain) {
                    std::printf("code %d L %d lds_width %d: %d held, width %d, %d CLOSEs, %llu bytes per job\n", code, L, lds_width, mp.cut.n_held, mp.cut.plan.width, mp.n_close,
                                (unsigned long long)marginal::marginal_bytes_per_job(mp));
                    rc |= check_twin(mp);
                    ++twins;
                    held += mp.cut.n_held > 0;
                }
            }
    const double neg[4] = {1.0, -0.1, 0.1, 0.1}, zero[4] = {0.0, 0.0, 0.0, 0.0}, ok[4] = {1.0, 0.0, 0.0, 0.5};
    rc |= marginal::check_marginal_weights("n", neg).code != QECMC_ERR_INVALID || marginal::check_marginal_weights("n", zero).code != QECMC_ERR_INVALID ||
          marginal::check_marginal_weights("n", ok).code != 0;
    rc |= marginal::check_marginal_args("n", 1ull << 32).code != QECMC_ERR_INVALID || marginal::check_marginal_args("n", 0xFFFFFFFFull).code != 0;
    rc |= twins < 12 || held < 2;
    std::printf(rc ? "class marginal selftest FAILED\n" : "class marginal selftest OK\n");
    return rc;
}
