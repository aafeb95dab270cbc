// Stand-alone check of class_sweep_tiled.hpp for the sanitizers (make sweep_tiled_asan: -fsanitize=address,undefined): builds the tiled plan of every
// (code, L) with L in [1, 13] and of a few large L under several (hbm_width, tile_width), checks WHICH are accepted, that an accepted plan keeps
// width <= hbm_width and n_held <= kMaxHeld, that its segments partition the ops with every INTRO / FORGET slot in the segment's tile, and that a plan
// with the cut plan's holds is the cut plan's stream op for op; then, at the small shapes, runs the twin against the cut twin (bit for bit where the
// holds agree) and walks the segment table the way the kernel does -- tile by tile through a small buffer, over a workspace and a tile filled with
// NaNs -- against the twin, bit for bit.  Exit status 0: all held.
#include "class_sweep_tiled.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

using namespace qecmc;

namespace {

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t draw()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

int check_plan(const sweep::TiledPlan &tp)
{
    const sweep::Plan &p = tp.plan;
    int fails = 0;
    fails += p.width > tp.hbm_width || tp.n_held > sweep::kMaxHeld || tp.n_held < tp.full_width - tp.hbm_width || (tp.n_held == 0) != (tp.full_width <= tp.hbm_width);
    fails += (int)tp.ops.size() != p.n_ops * sweep::kTiledOpWords || (int)tp.dev_ops.size() != p.n_ops * sweep::kTiledDevOpWords || !p.ops.empty();
    fails += (int)tp.held.size() != tp.n_held || tp.held_words.size() != (size_t)tp.n_held * p.W || tp.state_bits != (p.width > tp.tile_width ? p.width : tp.tile_width);
    uint32_t next = 0, live = 0;
    for (const sweep::Segment &sg : tp.segments) {
        fails += sg.op_first != next || sg.op_count == 0 || (int)sweep::popcount32(sg.tile) != tp.tile_width || (sg.tile >> tp.state_bits) != 0u || sg.live_in != live;
        fails += sg.n_tiles != 1u << sweep::popcount32(sg.live & ~sg.tile) || (sg.live >> p.width) != 0u;
        for (uint32_t o = sg.op_first; o < sg.op_first + sg.op_count && o < (uint32_t)p.n_ops; ++o) {
            const uint32_t *op = &tp.ops[(size_t)o * sweep::kTiledOpWords];
            const uint32_t kind = op[0] & 15u, slot = (op[0] >> 4) & 31u;
            fails += sweep::wide_before(op) != live || (kind != sweep::kClose && !((sg.tile >> slot) & 1u));
            live = sweep::wide_after(op);
            fails += (live & ~sg.live) != 0u;
        }
        fails += sg.live_out != live;
        next = sg.op_first + sg.op_count;
    }
    fails += next != (uint32_t)p.n_ops || live != 0u;
    const sweep::CutPlan cp = tp.hbm_width <= sweep::kCutMaxWidth ? sweep::build_cut_plan(p.code, p.L, tp.hbm_width) : sweep::CutPlan{};
    if (tp.hbm_width <= sweep::kCutMaxWidth && cp.plan.refusal.code == 0) {     // the cut plan of the same width: the same holds, the same stream
        fails += cp.held != tp.held || cp.held_words != tp.held_words || cp.plan.n_ops != p.n_ops || cp.plan.width != p.width || cp.plan.scale != p.scale;
        for (int o = 0; o < p.n_ops && o < cp.plan.n_ops; ++o) {
            const uint32_t *a = &cp.plan.ops[(size_t)o * sweep::kOpWords], *b = &tp.ops[(size_t)o * sweep::kTiledOpWords];
            fails += (a[0] & 15u) != (b[0] & 15u) || ((a[0] >> 4) & 15u) != ((b[0] >> 4) & 31u) || ((a[0] >> 8) & 15u) != ((b[0] >> 9) & 7u) || ((a[0] >> 12) & 31u) != ((b[0] >> 12) & 31u);
            fails += a[1] != b[1] || a[3] != b[3];
            for (int j = 0; j < 4; ++j) {
                const uint32_t x = (a[2] >> (8 * j)) & 0xFFu, y = (b[2] >> (8 * j)) & 0xFFu;
                fails += (x & 15u) != (y & 31u) || (x >> 4) != (y >> 5);
            }
        }
    }
    if (fails) std::fprintf(stderr, "code %d L %d hbm_width %d tile_width %d: %d plan checks failed\n", p.code, p.L, tp.hbm_width, tp.tile_width, fails);
    return fails != 0;
}

// one unit through the segment table as k_class_sweep_tiled walks it: every live tile gathered into `tile`, the segment's device ops, the tile stored
double walk_tiles(const sweep::TiledPlan &tp, const uint32_t *rep, const double *wxz, std::vector<double> &work, std::vector<double> &tile)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    work.assign((size_t)1 << tp.state_bits, nan);
    double partial = nan;
    for (size_t s = 0; s < tp.segments.size(); ++s) {
        const sweep::Segment &sg = tp.segments[s];
        const uint32_t fixed_live = sg.live & ~sg.tile, local_in = sweep::bits_extract(sg.live_in, sg.tile), local_out = sweep::bits_extract(sg.live_out, sg.tile);
        for (uint32_t t = 0; t < sg.n_tiles; ++t) {
            const uint32_t base = sweep::bits_deposit(t, fixed_live);
            tile.assign((size_t)1 << tp.tile_width, nan);
            if (s == 0) tile[0] = 1.0;
            else
                for (uint32_t l = 0; l < (1u << tp.tile_width); ++l)
                    if (!(l & ~local_in)) tile[l] = work[base + sweep::bits_deposit(l, sg.tile)];
            for (uint32_t o = sg.op_first; o < sg.op_first + sg.op_count; ++o) {
                const uint32_t *op = &tp.dev_ops[(size_t)o * sweep::kTiledDevOpWords];
                const uint32_t kind = op[0] & 15u, slot = (op[0] >> 4) & 15u, top = (op[0] >> 8) & 31u, mask = op[1], bit = 1u << slot;
                if (kind == sweep::kClose) {
                    const uint32_t q = op[3];
                    uint32_t cq = sweep::pauli_to_xz((rep[q >> 4] >> ((q & 15u) * 2u)) & 3u);
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t pr = (op[4] >> (8 * j)) & 0xFFu;
                        cq ^= (0u - ((base >> (pr & 31u)) & 1u)) & (pr >> 5);
                    }
                    for (uint32_t f = 0; f < (1u << top); ++f) {
                        if (f & ~mask) continue;
                        uint32_t idx = cq;
                        for (int j = 0; j < 4; ++j) {
                            const uint32_t pr = (op[2] >> (8 * j)) & 0xFFu;
                            idx ^= (0u - ((f >> (pr & 15u)) & 1u)) & (pr >> 4);
                        }
                        tile[f] = tile[f] * wxz[idx];
                    }
                } else {
                    for (uint32_t h = 0; h < (1u << (top - 1u)); ++h) {
                        const uint32_t f = sweep::insert_zero(h, slot);
                        if (f & ~mask) continue;
                        if (kind == sweep::kIntro) tile[f | bit] = tile[f];
                        else tile[f] = tile[f] + tile[f | bit];
                    }
                }
            }
            if (s + 1 == tp.segments.size()) partial = tile[0];
            else
                for (uint32_t l = 0; l < (1u << tp.tile_width); ++l)
                    if (!(l & ~local_out)) work[base + sweep::bits_deposit(l, sg.tile)] = tile[l];
        }
    }
    return partial;
}

int check_twin(const sweep::TiledPlan &tp)
{
    const sweep::Plan &p = tp.plan;
    const uint64_t N = 2;
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
    sweep::sweep_tiled_host(tp, N, chains.data(), w1, ones.data(), cls.data());
    for (size_t i = 0; i < ones.size(); ++i) fails += ones[i] != std::ldexp(1.0, p.rank);
    sweep::sweep_tiled_host(tp, N, chains.data(), w, z.data(), nullptr, 4);
    sweep::sweep_tiled_host(tp, N, chains.data(), w, z1.data(), nullptr, 1);
    fails += std::memcmp(z.data(), z1.data(), z.size() * sizeof(double)) != 0;
    // the cut twin: the same holds, and so the same bits, where it takes hbm_width as its lds_width; else its default plan to 1e-12
    const bool same = tp.hbm_width <= sweep::kCutMaxWidth;
    const sweep::CutPlan cp = sweep::build_cut_plan(p.code, p.L, same ? tp.hbm_width : 0);
    if (cp.plan.refusal.code == 0) {
        sweep::sweep_cut_host(cp, N, chains.data(), w, want.data(), cls2.data());
        for (size_t i = 0; i < z.size(); ++i) fails += !(z[i] > 0.0) || std::fabs(z[i] - want[i]) > 1e-12 * want[i];
        for (uint64_t s = 0; s < N; ++s) fails += cls[s] != cls2[s];
        if (same || (tp.n_held == 0 && cp.n_held == 0)) fails += std::memcmp(z.data(), want.data(), z.size() * sizeof(double)) != 0;
    }
    // the kernel's walk, unit by unit
    double wxz[4];
    sweep::weights_xz(w, wxz);
    std::vector<uint32_t> reps((size_t)p.ncls * p.W), rep((size_t)p.W);
    std::vector<double> work, tile, P((size_t)1 << tp.n_held);
    for (uint64_t s = 0; s < N; ++s) {
        sweep::class_representatives(p, chains.data() + s * p.nq, reps.data());
        for (int c = 0; c < p.ncls; ++c) {
            for (uint32_t h = 0; h < (1u << tp.n_held); ++h) {
                sweep::tiled_representative(tp, &reps[(size_t)c * p.W], h, rep.data());
                P[h] = walk_tiles(tp, rep.data(), wxz, work, tile);
            }
            const double got = sweep::cut_reduce(P.data(), tp.n_held, p.scale);
            fails += std::memcmp(&got, &z[s * p.ncls + c], sizeof got) != 0;
        }
    }
    if (fails) std::fprintf(stderr, "code %d L %d hbm_width %d tile_width %d: %d twin checks failed\n", p.code, p.L, tp.hbm_width, tp.tile_width, fails);
    return fails != 0;
}

}  // namespace

int main()
{
    int rc = 0, twins = 0;
    const int Ls[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 21, 23, 33, 64, 65};
    const int shapes[][2] = {{0, 0}, {13, 13}, {16, 8}, {8, 4}, {6, 5}};          // (hbm_width, tile_width)
    for (int code = -1; code <= 4; ++code)
        for (const int L : Ls)
            for (const auto &sh : shapes) {
                if (L > 13 && sh[0] != 0) continue;
                const sweep::TiledPlan tp = sweep::build_tiled_plan(code, L, sh[0], sh[1]);
                const bool odd_code = code == QECMC_XZZX || code == QECMC_ROTATED;
                const int hbm = sh[0] ? sh[0] : sweep::kTiledMaxWidth;
                int expect = 0;
                if (code < 0 || code > 3 || L < 2 || L > 64 || (odd_code && L % 2 == 0)) expect = QECMC_ERR_INVALID;
                else if (code == QECMC_TORIC && L % 2 == 0) expect = QECMC_ERR_UNSUPPORTED;
                else if (tp.full_width - sweep::kMaxHeld > hbm) expect = QECMC_ERR_UNSUPPORTED;
                else if (tp.plan.refusal.code == QECMC_ERR_UNSUPPORTED && tp.n_held == sweep::kMaxHeld) expect = QECMC_ERR_UNSUPPORTED;     // (a hold that does not narrow the peak)
                if (tp.plan.refusal.code != expect) {
                    std::fprintf(stderr, "code %d L %d (%d, %d): refusal %d (%s), expected %d\n", code, L, sh[0], sh[1], tp.plan.refusal.code, tp.plan.refusal.msg.c_str(), expect);
                    rc = 1;
                }
                if (tp.plan.refusal.code) continue;
                std::printf("code %d L %d hbm_width %d tile_width %d: full width %d, %d held, width %d, %d ops, %zu segments\n", code, L, tp.hbm_width, tp.tile_width,
                            tp.full_width, tp.n_held, tp.plan.width, tp.plan.n_ops, tp.segments.size());
                rc |= check_plan(tp);
                if (sh[0] != 0 && sh[0] <= 8 && tp.full_width <= 11) { rc |= check_twin(tp); ++twins; }
                if (sh[0] >= 13 && tp.full_width <= 13 && L <= 5) { rc |= check_twin(tp); ++twins; }
            }
    // the shapes the default plan is for, and the first it refuses
    const sweep::TiledPlan r21 = sweep::build_tiled_plan(QECMC_ROTATED, 21, 0, 0), t7 = sweep::build_tiled_plan(QECMC_TORIC, 7, 0, 0), t9 = sweep::build_tiled_plan(QECMC_TORIC, 9, 0, 0);
    rc |= r21.plan.refusal.code != 0 || r21.full_width != 24 || r21.n_held != 0 || t7.plan.refusal.code != 0 || t7.full_width != 29 || t7.n_held != 5 || t7.plan.width != 24;
    rc |= t9.plan.refusal.code != QECMC_ERR_UNSUPPORTED || t9.full_width != 37;
    for (const int bad : {-1, 3, 14, 99}) rc |= sweep::build_tiled_plan(QECMC_XZZX, 3, 0, bad).plan.refusal.code != QECMC_ERR_INVALID;
    for (const int bad : {-1, 12, 25, 99}) rc |= sweep::build_tiled_plan(QECMC_XZZX, 3, bad, 13).plan.refusal.code != QECMC_ERR_INVALID;
    rc |= twins < 8;
    std::printf(rc ? "class sweep tiled selftest FAILED\n" : "class sweep tiled selftest OK\n");
    return rc;
}
