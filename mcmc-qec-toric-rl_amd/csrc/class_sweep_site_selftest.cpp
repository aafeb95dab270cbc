// Stand-alone check of class_sweep_site.hpp for the sanitizers (make sweep_site_asan: -fsanitize=address,undefined): runs the three site twins on weight
// tables allocated at exactly rows * nq * 4 doubles -- a read past a row, or of a row that is not there, faults --, with one table and with one per
// syndrome; constant rows against the uniform twins, bit for bit; three distinct tables against the calls made with each alone; zero weights (the
// pure-erasure limit: every class weight is 0 or one power of two); NaN in cells that hold no qubit; and the host checks' refusals.  Exit status 0:
// all held.
#include "class_sweep_site.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>

using namespace qecmc;

namespace {

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t draw()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}
double draw_weight() { return std::exp(-6.9 * (draw() / 4294967296.0)); }       // log-uniform in about [1e-3, 1]

// one of the three routes: the plan's header and stream, and its two twins
struct Route {
    const char *name;
    sweep::Plan head;
    std::vector<uint32_t> ops;                                                   // four-word ops: what closed_qubits() reads
    sweep::Plan plan;
    sweep::CutPlan cut;
    sweep::TiledPlan tiled;
    int kind;
    void site(uint64_t N, const uint8_t *chains, const double *wq, uint64_t rows, double *z, int32_t *cls) const
    {
        if (kind == 0) sweep::sweep_site_host(plan, N, chains, wq, rows, z, cls);
        else if (kind == 1) sweep::sweep_cut_site_host(cut, N, chains, wq, rows, z, cls);
        else sweep::sweep_tiled_site_host(tiled, N, chains, wq, rows, z, cls);
    }
    void uniform(uint64_t N, const uint8_t *chains, const double *w, double *z, int32_t *cls) const
    {
        if (kind == 0) sweep::sweep_host(plan, N, chains, w, z, cls);
        else if (kind == 1) sweep::sweep_cut_host(cut, N, chains, w, z, cls);
        else sweep::sweep_tiled_host(tiled, N, chains, w, z, cls);
    }
};

Route make_route(int kind, int code, int L, int a, int b)
{
    Route r;
    r.kind = kind;
    if (kind == 0) { r.name = "sweep"; r.plan = sweep::build_plan(code, L); r.head = r.plan; r.ops = r.plan.ops; }
    else if (kind == 1) { r.name = "cut"; r.cut = sweep::build_cut_plan(code, L, a); r.head = r.cut.plan; r.ops = r.cut.plan.ops; }
    else { r.name = "tiled"; r.tiled = sweep::build_tiled_plan(code, L, a, b); r.head = r.tiled.plan; r.ops = r.tiled.ops; }
    return r;
}

// a heap block of exactly n doubles: AddressSanitizer guards either end
std::unique_ptr<double[]> exact_block(size_t n) { return std::unique_ptr<double[]>(new double[n]); }

bool idle_cell(const sweep::Plan &p, int q)
{
    return p.code == QECMC_PLANAR && q >= p.L * p.L && ((q - p.L * p.L) / p.L == p.L - 1 || (q - p.L * p.L) % p.L == p.L - 1);
}

int check_route(const Route &r)
{
    const sweep::Plan &p = r.head;
    if (p.refusal.code) { std::fprintf(stderr, "%s code %d L %d: refused (%s)\n", r.name, p.code, p.L, p.refusal.msg.c_str()); return 1; }
    const uint64_t N = 3;
    const size_t row = (size_t)p.nq * 4u, nz = N * (size_t)p.ncls;
    int fails = 0;
    std::vector<uint8_t> chains(N * p.nq, 0);
    for (uint64_t s = 0; s < N; ++s)
        for (int q = 0; q < p.nq; ++q)
            if (!idle_cell(p, q) && draw() < 0x40000000u) chains[s * p.nq + q] = (uint8_t)(1 + draw() % 3);
    const std::vector<char> named = sweep::closed_qubits(r.ops, p.nq);
    for (int q = 0; q < p.nq; ++q) fails += (named[(size_t)q] != 0) == idle_cell(p, q);
    std::vector<double> z(nz), want(nz), one(nz);
    std::vector<int32_t> cls(N), cls2(N);
    // ---- constant rows are the uniform twin, bit for bit, with one table and with N
    const double w[4] = {1.0, 0.031, 0.017, 0.29};
    r.uniform(N, chains.data(), w, want.data(), cls2.data());
    for (const uint64_t rows : {(uint64_t)1, N}) {
        auto wq = exact_block(rows * row);
        for (size_t i = 0; i < rows * row; ++i) wq[i] = w[i & 3u];
        fails += sweep::check_site_rows(N, rows).code != 0 || sweep::check_site_weights(wq.get(), rows, p.nq, named).code != 0;
        r.site(N, chains.data(), wq.get(), rows, z.data(), cls.data());
        fails += std::memcmp(z.data(), want.data(), nz * sizeof(double)) != 0 || cls != cls2;
    }
    // ---- three distinct tables: row s is the call made with table s alone
    auto wq = exact_block(N * row);
    for (size_t i = 0; i < N * row; ++i) wq[i] = draw_weight();
    for (int q = 0; q < p.nq; ++q)                                              // (a cell that holds no qubit may hold anything)
        if (idle_cell(p, q))
            for (uint64_t s = 0; s < N; ++s)
                for (int i = 0; i < 4; ++i) wq[s * row + (size_t)q * 4u + i] = std::numeric_limits<double>::quiet_NaN();
    fails += sweep::check_site_weights(wq.get(), N, p.nq, named).code != 0;
    r.site(N, chains.data(), wq.get(), N, z.data(), nullptr);
    for (uint64_t s = 0; s < N; ++s) {
        auto alone = exact_block(row);
        std::memcpy(alone.get(), wq.get() + s * row, row * sizeof(double));
        r.site(N, chains.data(), alone.get(), 1, one.data(), nullptr);
        fails += std::memcmp(&one[s * p.ncls], &z[s * p.ncls], p.ncls * sizeof(double)) != 0;
        for (int c = 0; c < p.ncls; ++c) fails += !(z[s * p.ncls + c] > 0.0) || !std::isfinite(z[s * p.ncls + c]);
    }
    // ---- zero weights: (1, 0, 0, 0) off a random set, (1, 1, 1, 1) on it, the chain I off the set -- every class weight is 0 or one power of two
    for (uint64_t s = 0; s < N; ++s)
        for (int q = 0; q < p.nq; ++q) {
            const bool erased = !idle_cell(p, q) && draw() < 0x40000000u;
            chains[s * p.nq + q] = erased ? (uint8_t)(draw() & 3u) : 0;
            for (int i = 0; i < 4; ++i) wq[s * row + (size_t)q * 4u + i] = erased || i == 0 ? 1.0 : 0.0;
        }
    fails += sweep::check_site_weights(wq.get(), N, p.nq, named).code != 0;
    r.site(N, chains.data(), wq.get(), N, z.data(), cls.data());
    for (uint64_t s = 0; s < N; ++s) {
        double common = 0.0;
        for (int c = 0; c < p.ncls; ++c) {
            const double v = z[s * p.ncls + c];
            int e = 0;
            if (v == 0.0) continue;
            fails += std::frexp(v, &e) != 0.5 || (common != 0.0 && v != common);
            common = v;
        }
        fails += z[s * p.ncls + cls[s]] == 0.0;                                 // the class of the true error has support on the erased set
    }
    // ---- the refusals, on blocks of the exact size
    fails += sweep::check_site_rows(N, 2).code != QECMC_ERR_INVALID || sweep::check_site_rows(N, 0).code != QECMC_ERR_INVALID || sweep::check_site_rows(0, 7).code != 0;
    int q0 = 0;
    while (!named[(size_t)q0]) ++q0;
    const double bad[] = {-1e-300, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()};
    for (const double b : bad) {
        const double keep = wq[(N - 1) * row + (size_t)q0 * 4u + 2];
        wq[(N - 1) * row + (size_t)q0 * 4u + 2] = b;
        const Refusal rf = sweep::check_site_weights(wq.get(), N, p.nq, named);
        char frag[64];
        std::snprintf(frag, sizeof frag, "wq[row %llu][qubit %d][Y]", (unsigned long long)(N - 1), q0);
        fails += rf.code != QECMC_ERR_INVALID || rf.msg.find(frag) == std::string::npos;
        wq[(N - 1) * row + (size_t)q0 * 4u + 2] = keep;
    }
    for (int i = 0; i < 4; ++i) wq[row + (size_t)q0 * 4u + i] = 0.0;
    const Refusal all_zero = sweep::check_site_weights(wq.get(), N, p.nq, named);
    fails += all_zero.code != QECMC_ERR_INVALID || all_zero.msg.find("all zero") == std::string::npos || all_zero.msg.find("wq[row 1]") == std::string::npos;
    if (fails) std::fprintf(stderr, "%s code %d L %d: %d checks failed\n", r.name, p.code, p.L, fails);
    else std::printf("%s code %d L %d: width %d, %d ops\n", r.name, p.code, p.L, p.width, p.n_ops);
    return fails != 0;
}

}  // namespace

int main()
{
    int rc = 0;
    rc |= check_route(make_route(0, QECMC_TORIC, 3, 0, 0));
    rc |= check_route(make_route(0, QECMC_PLANAR, 4, 0, 0));
    rc |= check_route(make_route(0, QECMC_XZZX, 5, 0, 0));
    rc |= check_route(make_route(0, QECMC_ROTATED, 7, 0, 0));
    rc |= check_route(make_route(1, QECMC_TORIC, 3, 4, 0));
    rc |= check_route(make_route(1, QECMC_PLANAR, 3, 3, 0));
    rc |= check_route(make_route(1, QECMC_XZZX, 5, 6, 0));
    rc |= check_route(make_route(2, QECMC_XZZX, 5, 0, 4));
    rc |= check_route(make_route(2, QECMC_TORIC, 3, 8, 4));
    rc |= check_route(make_route(2, QECMC_PLANAR, 4, 6, 5));
    rc |= check_route(make_route(2, QECMC_ROTATED, 7, 0, 5));
    // a refused plan stays refused: the site twins are never reached
    rc |= sweep::build_plan(QECMC_TORIC, 5).refusal.code != QECMC_ERR_UNSUPPORTED || sweep::build_cut_plan(QECMC_TORIC, 4, 0).plan.refusal.code != QECMC_ERR_UNSUPPORTED;
    std::printf(rc ? "class sweep site selftest FAILED\n" : "class sweep site selftest OK\n");
    return rc;
}
