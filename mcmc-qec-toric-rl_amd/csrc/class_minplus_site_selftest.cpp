// Stand-alone check of class_minplus_site.hpp for the sanitizers (make minplus_site_asan: -fsanitize=address,undefined): the site plans of every
// (code, L) against the uniform plans -- the same refusals behind the entry points' own prefixes --; the row check; the packed words; then, for every
// plan that is cheap enough, the two twins on random chains with the cost table in a heap block of exactly rows * nq * 4 bytes (one table, and one
// per syndrome), outputs of their exact size, poisoned: cost, count and class of the sweep twin equal the trace twin's; every chain has the input's
// syndrome, lies in its class and has the site cost the sweep reports; constant rows give the uniform twins, chains included; one table equals N
// copies of it; a pair repeated by hand over POISONED scratch and decision words agrees.  Exit status 0: all held.
#include "class_minplus_site.hpp"

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

int check_plan(int code, int L, int lds_width)
{
    const sweep::CutPlan u = minplus::build_minplus_plan(code, L, lds_width), s = minplus::build_minplus_site_plan(code, L, lds_width);
    const minplus::TracePlan ut = minplus::build_trace_plan(code, L, lds_width), st = minplus::build_trace_site_plan(code, L, lds_width);
    int fails = u.plan.refusal.code != s.plan.refusal.code || ut.cut.plan.refusal.code != st.cut.plan.refusal.code;
    if (u.plan.refusal.code) fails += s.plan.refusal.msg != "qecmc_class_minplus_site:" + u.plan.refusal.msg.substr(std::strlen("qecmc_class_minplus:"));
    else fails += s.plan.ops != u.plan.ops || s.held_words != u.held_words;
    if (ut.cut.plan.refusal.code)
        fails += st.cut.plan.refusal.msg != "qecmc_class_minplus_chains_site:" + ut.cut.plan.refusal.msg.substr(std::strlen("qecmc_class_minplus_chains:"));
    else fails += st.cut.plan.ops != ut.cut.plan.ops || st.forget_words != ut.forget_words;
    if (fails) std::fprintf(stderr, "code %d L %d lds_width %d: %d plan checks failed\n", code, L, lds_width, fails);
    return fails != 0;
}

int check_twin(const minplus::TracePlan &tp)
{
    const sweep::CutPlan &cp = tp.cut;
    const sweep::Plan &p = cp.plan;
    const uint64_t N = 3;
    int fails = 0;
    std::vector<std::vector<uint8_t>> gen;
    std::vector<char> touched;
    generator_bytes(p, gen, touched);
    const std::vector<char> named = sweep::closed_qubits(p.ops, p.nq);
    for (int q = 0; q < p.nq; ++q) fails += (named[(size_t)q] != 0) != (touched[(size_t)q] != 0);       // a CLOSE per qubit, none for a cell without one
    std::vector<uint8_t> chains(N * p.nq, 0);
    for (uint64_t s = 1; s < N; ++s)
        for (int q = 0; q < p.nq; ++q)
            if (touched[(size_t)q] && draw() < (s == 1 ? 0x10000000u : 0x50000000u)) chains[s * p.nq + q] = (uint8_t)(1 + draw() % 3);
    const size_t n_out = (size_t)N * p.ncls, row = (size_t)p.nq * 4u;
    for (int variant = 0; variant < 4; ++variant) {
        // 0: random bytes, a row per syndrome; 1: random bytes, one table; 2: {0, 1}, a row per syndrome; 3: extreme bytes, a row per syndrome
        const uint64_t rows = variant == 1 ? 1 : N;
        uint8_t *cq = new uint8_t[rows * row];                                  // exactly rows * nq * 4 bytes
        for (size_t i = 0; i < rows * row; ++i) cq[i] = variant == 2 ? (uint8_t)(draw() & 1u) : variant == 3 ? (uint8_t)((draw() & 1u) ? 255 : 0) : (uint8_t)draw();
        uint8_t *out = new uint8_t[n_out * p.nq];
        uint32_t *cost = new uint32_t[n_out], *cost2 = new uint32_t[n_out];
        uint64_t *count = new uint64_t[n_out], *count2 = new uint64_t[n_out];
        int32_t *cls = new int32_t[N], *cls2 = new int32_t[N];
        std::memset(out, 0xEE, n_out * p.nq);
        std::memset(cost, 0xEE, n_out * sizeof(uint32_t));
        std::memset(count, 0xEE, n_out * sizeof(uint64_t));
        minplus::minplus_trace_site_host(tp, N, chains.data(), cq, rows, out, cost, count, cls, 4);
        minplus::minplus_cut_site_host(cp, N, chains.data(), cq, rows, cost2, count2, cls2, 1);
        fails += std::memcmp(cost, cost2, n_out * sizeof(uint32_t)) != 0 || std::memcmp(count, count2, n_out * sizeof(uint64_t)) != 0 ||
                 std::memcmp(cls, cls2, N * sizeof(int32_t)) != 0;
        uint8_t *again = new uint8_t[n_out * p.nq];
        minplus::minplus_trace_site_host(tp, N, chains.data(), cq, rows, again, nullptr, nullptr, nullptr, 1);     // (one thread, and the nullable outputs)
        fails += std::memcmp(out, again, n_out * p.nq) != 0;
        if (rows == 1) {                                                        // one table is N copies of it
            uint8_t *copies = new uint8_t[N * row];
            for (uint64_t s = 0; s < N; ++s) std::memcpy(copies + s * row, cq, row);
            minplus::minplus_trace_site_host(tp, N, chains.data(), copies, N, again, cost2, count2, cls2, 2);
            fails += std::memcmp(out, again, n_out * p.nq) != 0 || std::memcmp(cost, cost2, n_out * sizeof(uint32_t)) != 0 ||
                     std::memcmp(count, count2, n_out * sizeof(uint64_t)) != 0;
            delete[] copies;
        }
        delete[] again;
        std::vector<uint32_t> reps((size_t)p.ncls * p.W), rep((size_t)p.W), words((size_t)p.W), cw((size_t)p.nq);
        std::vector<uint8_t> bytes((size_t)p.nq);
        for (uint64_t s = 0; s < N; ++s) {
            const uint8_t *mine_cq = cq + (rows == 1 ? 0u : s) * row;
            minplus::site_cost_words(mine_cq, 1, p.nq, cw.data());
            const std::vector<char> syn = syndrome(gen, chains.data() + s * p.nq, p.nq);
            sweep::class_representatives(p, chains.data() + s * p.nq, reps.data());
            for (int c = 0; c < p.ncls; ++c) {
                const uint8_t *mine = out + (s * p.ncls + c) * p.nq;
                uint32_t sum = 0;
                for (int q = 0; q < p.nq; ++q) {
                    fails += mine[q] > 3;
                    if (touched[(size_t)q]) {
                        sum += mine_cq[(size_t)q * 4u + (mine[q] & 3u)];
                        fails += minplus::site_cost(cw[(size_t)q], sweep::pauli_to_xz(mine[q] & 3u)) != mine_cq[(size_t)q * 4u + (mine[q] & 3u)];
                    }
                }
                fails += sum != cost[s * p.ncls + c];
                fails += syndrome(gen, mine, p.nq) != syn;
                std::fill(words.begin(), words.end(), 0u);
                for (int q = 0; q < p.nq; ++q) words[(size_t)(q >> 4)] |= (uint32_t)(mine[q] & 3u) << ((q & 15) * 2);
                lift::HostState st{words.data()};
                fails += correct::class_of(st, p.code, p.L, p.W) != c;
                // the pair by hand: partials, pick, forward pass and walk over poisoned scratch of the exact size
                std::vector<uint64_t> A((size_t)1 << p.width, 0xDEADBEEFDEADBEEFull), D((size_t)tp.n_forget * tp.words_per_forget, 0xFFFFFFFFFFFFFFFFull),
                    P((size_t)1 << cp.n_held);
                for (uint32_t h = 0; h < (1u << cp.n_held); ++h) {
                    sweep::cut_representative(cp, &reps[(size_t)c * p.W], h, rep.data());
                    P[h] = minplus::minplus_one_site(p, rep.data(), cw.data(), A.data());
                }
                const uint32_t pick = minplus::pick_assignment(P.data(), cp.n_held);
                sweep::cut_representative(cp, &reps[(size_t)c * p.W], pick, rep.data());
                fails += minplus::minplus_one_traced_site(tp, rep.data(), cw.data(), A.data(), D.data()) != P[pick];
                fails += minplus::trace_walk(tp, D.data(), rep.data()) != 0u;
                minplus::unpack_chain(rep.data(), p.nq, bytes.data());
                fails += std::memcmp(bytes.data(), mine, (size_t)p.nq) != 0;
            }
        }
        delete[] cq; delete[] out; delete[] cost; delete[] cost2; delete[] count; delete[] count2; delete[] cls; delete[] cls2;
    }
    // constant rows are the uniform twins, chains included
    const uint32_t costs[3][4] = {{0, 1, 1, 1}, {0, 3, 3, 1}, {1, 0, 2, 255}};
    for (const auto &c4 : costs) {
        uint8_t *cq = new uint8_t[row];
        for (size_t i = 0; i < row; ++i) cq[i] = (uint8_t)c4[i & 3u];
        std::vector<uint8_t> a(n_out * p.nq), b(n_out * p.nq);
        std::vector<uint32_t> ca(n_out), cb(n_out);
        std::vector<uint64_t> na(n_out), nb(n_out);
        minplus::minplus_trace_site_host(tp, N, chains.data(), cq, 1, a.data(), ca.data(), na.data(), nullptr, 3);
        minplus::minplus_trace_host(tp, N, chains.data(), c4, b.data(), cb.data(), nb.data(), nullptr, 3);
        fails += a != b || ca != cb || na != nb;
        delete[] cq;
    }
    if (fails) std::fprintf(stderr, "code %d L %d lds_width %d: %d twin checks failed\n", p.code, p.L, cp.lds_width, fails);
    return fails != 0;
}

}  // namespace

int main()
{
    int rc = 0, twins = 0, held = 0;
    const int Ls[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 33, 65};
    for (int code = -1; code <= 4; ++code)
        for (const int L : Ls)
            for (const int lds_width : {0, 14, 6, 99}) {
                if (L > 13 && lds_width != 0) continue;
                rc |= check_plan(code, L, lds_width);
                const minplus::TracePlan tp = minplus::build_trace_site_plan(code, L, lds_width);
                if (tp.cut.plan.refusal.code) continue;
                const bool narrow = lds_width == 6 && tp.cut.full_width <= 10, plain = lds_width == 0 && tp.cut.n_held == 0 && tp.cut.plan.width <= 10;
                if (narrow || plain) {
                    std::printf("code %d L %d lds_width %d: %d held, width %d\n", code, L, lds_width, tp.cut.n_held, tp.cut.plan.width);
                    rc |= check_twin(tp);
                    ++twins;
                    held += tp.cut.n_held > 0;
                }
            }
    const Refusal r = minplus::check_cost_rows("qecmc_class_minplus_site", 5, 2);
    rc |= r.code != QECMC_ERR_INVALID || r.msg.compare(0, 25, "qecmc_class_minplus_site:") != 0;
    rc |= minplus::check_cost_rows("x", 5, 1).code != 0 || minplus::check_cost_rows("x", 5, 5).code != 0 || minplus::check_cost_rows("x", 0, 7).code != 0;
    const uint8_t one[4] = {1, 2, 3, 4};
    uint32_t word = 0;
    minplus::site_cost_words(one, 1, 1, &word);
    rc |= word != 0x03040201u || minplus::site_cost(word, 0) != 1 || minplus::site_cost(word, 1) != 2 || minplus::site_cost(word, 2) != 4 || minplus::site_cost(word, 3) != 3;
    rc |= twins < 10 || held < 2;
    std::printf(rc ? "class minplus site selftest FAILED\n" : "class minplus site selftest OK\n");
    return rc;
}
