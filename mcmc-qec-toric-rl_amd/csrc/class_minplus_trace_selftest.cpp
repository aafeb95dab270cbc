// Stand-alone check of class_minplus_trace.hpp for the sanitizers (make minplus_trace_asan: -fsanitize=address,undefined): builds the trace plan of
// every (code, L) with L in [1, 13] under lds_width 0, 13, 14 and a narrow one and checks it against build_minplus_plan -- the same refusals behind
// the entry point's own prefix, the same op stream, every generator held or retired exactly once, forget_words against the generator table --; the
// launch group against its bound; then, for every plan that is cheap enough, runs the twin on random chains with its outputs in heap blocks of their
// exact size, poisoned, and repeats every pair by hand over POISONED scratch and decision words of their exact size: the chains agree byte for
// byte, commute with every generator exactly where the input does not (the syndrome), lie in their class, cost what the sweep reports, and the walk
// ends at f == 0.  cost and count are minplus_cut_host's.  Exit status 0: all held.
#include "class_minplus_trace.hpp"

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

// bit g: the chain anticommutes with generator g (two Paulis anticommute where both are set and differ)
std::vector<char> syndrome(const std::vector<std::vector<uint8_t>> &gen, const uint8_t *chain, int nq)
{
    std::vector<char> s(gen.size(), 0);
    for (size_t g = 0; g < gen.size(); ++g)
        for (int q = 0; q < nq; ++q) s[g] ^= (char)(gen[g][(size_t)q] && (chain[q] & 3u) && gen[g][(size_t)q] != (chain[q] & 3u));
    return s;
}

int check_plan(int code, int L, int lds_width)
{
    const sweep::CutPlan cp = minplus::build_minplus_plan(code, L, lds_width);
    const minplus::TracePlan tp = minplus::build_trace_plan(code, L, lds_width);
    const sweep::Plan &p = tp.cut.plan;
    if (p.refusal.code != cp.plan.refusal.code) return 1;
    if (cp.plan.refusal.code) {
        const std::string want = "qecmc_class_minplus_chains:" + cp.plan.refusal.msg.substr(std::strlen("qecmc_class_minplus:"));
        return p.refusal.msg != want;
    }
    int fails = p.ops != cp.plan.ops || tp.cut.held != cp.held || tp.cut.held_words != cp.held_words;
    fails += tp.n_forget != p.n_gen - cp.n_held || (int)tp.forget_gen.size() != tp.n_forget || tp.forget_words.size() != (size_t)tp.n_forget * p.W;
    fails += tp.words_per_forget != (p.width - 1 > 6 ? 1 << (p.width - 7) : 1);
    std::vector<int> seen((size_t)p.n_gen, 0);
    for (const int g : cp.held) ++seen[(size_t)g];
    for (const int g : tp.forget_gen) ++seen[(size_t)g];
    for (const int n : seen) fails += n != 1;
    std::vector<std::vector<uint8_t>> gen;
    std::vector<char> touched;
    generator_bytes(p, gen, touched);
    std::vector<uint8_t> bytes((size_t)p.nq);
    for (int i = 0; i < tp.n_forget && !fails; ++i) {
        minplus::unpack_chain(&tp.forget_words[(size_t)i * p.W], p.nq, bytes.data());
        fails += bytes != gen[(size_t)tp.forget_gen[(size_t)i]];
    }
    const uint64_t per = minplus::trace_bytes_per_pair(tp);
    for (const uint64_t N : {0ull, 1ull, 7ull, 600ull, 5000ull, 1ull << 32}) {
        const uint32_t group = minplus::trace_launch_group(N, p.ncls, cp.n_held, per);
        fails += group < 1 || group > sweep::cut_launch_group(N, p.ncls, cp.n_held) || (uint64_t)group * p.ncls * per > minplus::kTraceWorkspaceBytes;
    }
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
    std::vector<uint8_t> chains(N * p.nq, 0);
    for (uint64_t s = 1; s < N; ++s)
        for (int q = 0; q < p.nq; ++q)
            if (touched[(size_t)q] && draw() < (s == 1 ? 0x10000000u : 0x50000000u)) chains[s * p.nq + q] = (uint8_t)(1 + draw() % 3);
    const size_t n_out = (size_t)N * p.ncls;
    std::vector<uint32_t> cost_want(n_out);
    std::vector<uint64_t> count_want(n_out);
    std::vector<int32_t> cls_want(N);
    const uint32_t costs[4][4] = {{0, 1, 1, 1}, {0, 3, 3, 1}, {1, 0, 2, 3}, {0, 0, 0, 0}};
    for (const auto &c4 : costs) {
        // outputs at their exact size, poisoned
        uint8_t *out = new uint8_t[n_out * p.nq];
        uint32_t *cost = new uint32_t[n_out];
        uint64_t *count = new uint64_t[n_out];
        int32_t *cls = new int32_t[N];
        std::memset(out, 0xEE, n_out * p.nq);
        std::memset(cost, 0xEE, n_out * sizeof(uint32_t));
        std::memset(count, 0xEE, n_out * sizeof(uint64_t));
        minplus::minplus_trace_host(tp, N, chains.data(), c4, out, cost, count, cls, 4);
        minplus::minplus_cut_host(cp, N, chains.data(), c4, cost_want.data(), count_want.data(), cls_want.data());
        fails += std::memcmp(cost, cost_want.data(), n_out * sizeof(uint32_t)) != 0 || std::memcmp(count, count_want.data(), n_out * sizeof(uint64_t)) != 0 ||
                 std::memcmp(cls, cls_want.data(), N * sizeof(int32_t)) != 0;
        uint8_t *again = new uint8_t[n_out * p.nq];
        minplus::minplus_trace_host(tp, N, chains.data(), c4, again, nullptr, nullptr, nullptr, 1);       // (one thread, and the nullable outputs)
        fails += std::memcmp(out, again, n_out * p.nq) != 0;
        delete[] again;
        uint32_t cxz[4];
        minplus::costs_xz(c4, cxz);
        std::vector<uint32_t> reps((size_t)p.ncls * p.W), rep((size_t)p.W), words((size_t)p.W);
        std::vector<uint8_t> bytes((size_t)p.nq);
        for (uint64_t s = 0; s < N; ++s) {
            const std::vector<char> syn = syndrome(gen, chains.data() + s * p.nq, p.nq);
            sweep::class_representatives(p, chains.data() + s * p.nq, reps.data());
            for (int c = 0; c < p.ncls; ++c) {
                const uint8_t *mine = out + (s * p.ncls + c) * p.nq;
                uint32_t sum = 0;
                for (int q = 0; q < p.nq; ++q) {
                    fails += mine[q] > 3;
                    if (touched[(size_t)q]) sum += c4[mine[q] & 3u];
                }
                fails += sum != cost[s * p.ncls + c];
                fails += syndrome(gen, mine, p.nq) != syn;
                std::fill(words.begin(), words.end(), 0u);
                for (int q = 0; q < p.nq; ++q) words[(size_t)(q >> 4)] |= (uint32_t)(mine[q] & 3u) << ((q & 15) * 2);
                lift::HostState st{words.data()};
                fails += correct::class_of(st, p.code, p.L, p.W) != c;
                if (c4[1] == 0 && c4[3] == 0) {                                 // all-zero costs: every decision ties, the representative itself comes back
                    minplus::unpack_chain(&reps[(size_t)c * p.W], p.nq, bytes.data());
                    fails += std::memcmp(bytes.data(), mine, (size_t)p.nq) != 0;
                }
                // the pair by hand: partials, pick, forward pass and walk over poisoned scratch of the exact size
                std::vector<uint64_t> A((size_t)1 << p.width, 0xDEADBEEFDEADBEEFull), D((size_t)tp.n_forget * tp.words_per_forget, 0xFFFFFFFFFFFFFFFFull),
                    P((size_t)1 << cp.n_held);
                for (uint32_t h = 0; h < (1u << cp.n_held); ++h) {
                    sweep::cut_representative(cp, &reps[(size_t)c * p.W], h, rep.data());
                    P[h] = minplus::minplus_one(p, rep.data(), cxz, A.data());
                }
                const uint32_t pick = minplus::pick_assignment(P.data(), cp.n_held);
                for (uint32_t h = 0; h < pick; ++h) fails += (P[h] >> minplus::kCountBits) <= (P[pick] >> minplus::kCountBits);
                for (uint32_t h = pick; h < (1u << cp.n_held); ++h) fails += (P[h] >> minplus::kCountBits) < (P[pick] >> minplus::kCountBits);
                sweep::cut_representative(cp, &reps[(size_t)c * p.W], pick, rep.data());
                fails += minplus::minplus_one_traced(tp, rep.data(), cxz, A.data(), D.data()) != P[pick];
                fails += minplus::trace_walk(tp, D.data(), rep.data()) != 0u;
                minplus::unpack_chain(rep.data(), p.nq, bytes.data());
                fails += std::memcmp(bytes.data(), mine, (size_t)p.nq) != 0;
            }
        }
        delete[] out; delete[] cost; delete[] count; delete[] cls;
    }
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
                const minplus::TracePlan tp = minplus::build_trace_plan(code, L, lds_width);
                if (tp.cut.plan.refusal.code) continue;
                // cheap enough here: the narrow plans of the small shapes (held generators), and every plan that holds nothing up to width 11
                const bool narrow = lds_width == 6 && tp.cut.full_width <= 10, plain = lds_width == 0 && tp.cut.n_held == 0 && tp.cut.plan.width <= 11;
                if (narrow || plain) {
                    std::printf("code %d L %d lds_width %d: %d held, width %d, %d FORGETs of %d words\n", code, L, lds_width, tp.cut.n_held, tp.cut.plan.width, tp.n_forget,
                                tp.words_per_forget);
                    rc |= check_twin(tp);
                    ++twins;
                    held += tp.cut.n_held > 0;
                }
            }
    const uint32_t bad[4] = {0, 1, 256, 1}, good[4] = {255, 0, 255, 7};
    const Refusal r = minplus::check_chain_costs(bad);
    rc |= r.code != QECMC_ERR_INVALID || r.msg.compare(0, 27, "qecmc_class_minplus_chains:") != 0 || minplus::check_chain_costs(good).code != 0;
    for (const int w : {-1, 1, 15, 99}) rc |= minplus::build_trace_plan(QECMC_XZZX, 3, w).cut.plan.refusal.code != QECMC_ERR_INVALID;
    rc |= minplus::trace_launch_group(9, 16, 0, 1ull << 40) != 1u || minplus::trace_launch_group(0, 4, 0, 8) != 1u;
    rc |= minplus::remove_bit(sweep::insert_zero(0x2B5u, 4), 4) != 0x2B5u;
    rc |= twins < 12 || held < 2;
    std::printf(rc ? "class minplus trace selftest FAILED\n" : "class minplus trace selftest OK\n");
    return rc;
}
