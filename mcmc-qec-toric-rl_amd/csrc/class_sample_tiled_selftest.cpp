// Stand-alone check of class_sample_tiled.hpp for the sanitizers (make sample_tiled_asan: -fsanitize=address,undefined): the sample plans of the small
// shapes under several widths of state vector and tile -- nothing held, holds forced by a narrow hbm_width --, their refusals under this entry
// point's names, the cap on one job's record and the jobs of a pass; the twin sample_tiled_host over POISONED buffers of their exact size, in both
// modes, uniform and site; and a host walk of the DEVICE layout: the sweep run segment by segment and tile by tile in the tile's own coordinates (the
// device ops), every FORGET's pairs stored where the kernels store them -- R[pair_off[fi] + x * 2^(tile_width - 1) + h] over a dirty block of exactly
// bytes_per_job bytes -- and read back through forget_tile from the global f, which must give the twin's chains byte for byte.  Exit status 0: all held.
#include "class_sample_tiled.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

using namespace qecmc;

namespace {

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t draw()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

int g_failed = 0;
#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while (0)

// buffers of exactly n elements on the heap, so that one element too far is seen
template <class T> std::unique_ptr<T[]> exact(size_t n, int fill)
{
    std::unique_ptr<T[]> p(new T[n ? n : 1]);
    std::memset(p.get(), fill, (n ? n : 1) * sizeof(T));
    return p;
}

// One job in the device's layout.  A: 2^state_bits entries, R: pairs_per_job pairs, both dirty; rep: the representative under h*; tab, stride: the
// factors.  The segments in order; within a segment every live tile alone: gather, the segment's device ops over a dirty tile, write back.
void device_layout_record(const sample::TiledSamplePlan &tsp, const uint32_t *rep, const double *tab, size_t stride, double *A, sample::PairRecord *R)
{
    const sweep::TiledPlan &tp = tsp.tiled;
    const uint32_t entries = 1u << tp.tile_width;
    for (size_t s = 0; s < tp.segments.size(); ++s) {
        const sweep::Segment &sg = tp.segments[s];
        const uint32_t fixed_live = sg.live & ~sg.tile, local_in = sweep::bits_extract(sg.live_in, sg.tile), local_out = sweep::bits_extract(sg.live_out, sg.tile);
        for (uint32_t x = 0; x < sg.n_tiles; ++x) {
            const uint32_t base = sweep::bits_deposit(x, fixed_live);
            auto lds = exact<double>(entries, 0xA5);
            if (s == 0) lds[0] = 1.0;
            else
                for (uint32_t l = 0; l < entries; ++l)
                    if (!(l & ~local_in)) lds[l] = A[base + sweep::bits_deposit(l, sg.tile)];
            uint32_t fi = tsp.seg_forget[s];
            for (uint32_t o = sg.op_first; o < sg.op_first + sg.op_count; ++o) {
                const uint32_t *op = &tp.dev_ops[(size_t)o * sweep::kTiledDevOpWords];
                const uint32_t kind = op[0] & 15u, slot = (op[0] >> 4) & 15u, top = (op[0] >> 8) & 31u, mask = op[1], bit = 1u << slot;
                if (kind == sweep::kClose) {
                    const uint32_t q = op[3];
                    uint32_t cq = sweep::pauli_to_xz((rep[q >> 4] >> ((q & 15u) * 2u)) & 3u);
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t pr = (op[4] >> (8 * j)) & 0xFFu;
                        if ((base >> (pr & 31u)) & 1u) cq ^= pr >> 5;
                    }
                    for (uint32_t l = 0; l < (1u << top); ++l) {
                        if (l & ~mask) continue;
                        uint32_t idx = cq;
                        for (int j = 0; j < 4; ++j) {
                            const uint32_t pr = (op[2] >> (8 * j)) & 0xFFu;
                            if ((l >> (pr & 15u)) & 1u) idx ^= pr >> 4;
                        }
                        lds[l] = lds[l] * tab[(size_t)q * stride + idx];
                    }
                } else if (kind == sweep::kIntro) {
                    for (uint32_t h = 0; h < (1u << (top - 1u)); ++h) {
                        const uint32_t f = sweep::insert_zero(h, slot);
                        if (!(f & ~mask)) lds[f | bit] = lds[f];
                    }
                } else {
                    const uint32_t *ft = &tsp.forget_tile[(size_t)fi * sample::kTiledForgetWords];
                    CHECK(ft[0] == sg.tile && ft[1] == fixed_live && ft[2] == slot && (uint64_t)ft[3] == tsp.pair_off[fi]);
                    sample::PairRecord *rows = R + ft[3] + ((size_t)x << (tp.tile_width - 1));
                    for (uint32_t h = 0; h < (1u << (top - 1u)); ++h) {
                        const uint32_t f = sweep::insert_zero(h, slot);
                        if (f & ~mask) continue;
                        const double off = lds[f], on = lds[f | bit], sum = off + on;
                        rows[h] = sample::PairRecord{on, sum};                    // (within the job's pairs_per_job pairs, or the sanitizer says so)
                        lds[f] = sum;
                    }
                    ++fi;
                }
            }
            if (s + 1 < tp.segments.size())
                for (uint32_t l = 0; l < entries; ++l)
                    if (!(l & ~local_out)) A[base + sweep::bits_deposit(l, sg.tile)] = lds[l];
        }
    }
}

// the walk as the kernel addresses it: x, l and h from the global f through forget_tile
void device_layout_walk(const sample::TiledSamplePlan &tsp, const sample::PairRecord *R, uint64_t k, uint32_t syndrome, uint32_t stream, uint64_t seed, uint32_t *chain)
{
    const sweep::TiledPlan &tp = tsp.tiled;
    uint32_t f = 0;
    int fi = tsp.n_forget;
    for (int o = tp.plan.n_ops - 1; o >= 0; --o) {
        const uint32_t w0 = tp.ops[(size_t)o * sweep::kTiledOpWords], kind = w0 & 15u, bit = 1u << ((w0 >> 4) & 31u);
        if (kind == sweep::kIntro) f &= ~bit;
        else if (kind == sweep::kForget) {
            --fi;
            const uint32_t *ft = &tsp.forget_tile[(size_t)fi * sample::kTiledForgetWords];
            const uint32_t x = sweep::bits_extract(f, ft[1]), h = minplus::remove_bit(sweep::bits_extract(f, ft[0]), ft[2]);
            const sample::PairRecord r = R[(size_t)ft[3] + ((size_t)x << (tp.tile_width - 1)) + h];
            if (sample::take_branch(sample::draw_u53(k, 1u + ((uint32_t)fi >> 1), (uint32_t)fi & 1u, syndrome, stream, seed), r.on, r.s)) {
                f |= bit;
                for (int w = 0; w < tp.plan.W; ++w) chain[w] ^= tsp.forget_words[(size_t)fi * tp.plan.W + w];
            }
        }
    }
    CHECK(f == 0);
}

void random_chains(int nq, uint64_t N, uint8_t *out)
{
    for (uint64_t i = 0; i < N * (uint64_t)nq; ++i) out[i] = (draw() % 10u == 0u) ? (uint8_t)(1u + draw() % 3u) : 0u;
}

struct Shape { int code, L, hbm_width, tile_width; };

// the twin over poisoned buffers of exact size in both modes, then every sample of mode 0 again through the device's layout
void check_shape(const Shape &sh, bool site)
{
    const char *name = site ? "qecmc_class_sample_tiled_site" : "qecmc_class_sample_tiled";
    const sample::TiledSamplePlan tsp = sample::build_tiled_sample_plan(sh.code, sh.L, sh.hbm_width, sh.tile_width, name);
    const sweep::TiledPlan &tp = tsp.tiled;
    const sweep::Plan &p = tp.plan;
    CHECK(p.refusal.code == 0);
    if (p.refusal.code) { std::printf("  %s\n", p.refusal.msg.c_str()); return; }
    CHECK(tsp.n_forget == p.n_gen - tp.n_held && tsp.pair_off.size() == (size_t)tsp.n_forget + 1u && tsp.pair_off.back() == tsp.pairs_per_job);
    const uint64_t N = 2, K = 3, seed = 0x5EED5EEDull + (uint64_t)sh.L;
    const uint32_t first = 40;
    const size_t nq = (size_t)p.nq, ncls = (size_t)p.ncls, row = nq * 4u;
    auto chains = exact<uint8_t>(N * nq, 0);
    random_chains(p.nq, N, chains.get());
    const double w4[4] = {0.9, 0.05, 0.02, 0.03};
    auto wq = exact<double>(N * row, 0);
    for (size_t i = 0; i < N * row; ++i) wq[i] = 0.05 + (double)(draw() % 1000u) / 1000.0;
    auto out0 = exact<uint8_t>(N * ncls * K * nq, 0xEE);
    auto out1 = exact<uint8_t>(N * K * nq, 0xEE);
    auto cls = exact<int32_t>(N * K, 0x7F);
    auto z0 = exact<double>(N * ncls, 0xFF), z1 = exact<double>(N * ncls, 0xFF);
    Refusal r = sample::sample_tiled_host(tsp, name, N, chains.get(), site ? nullptr : w4, site ? wq.get() : nullptr, site ? N : 0, K, seed, first, 0, out0.get(), nullptr,
                                          z0.get(), 2);
    CHECK(r.code == 0);
    r = sample::sample_tiled_host(tsp, name, N, chains.get(), site ? nullptr : w4, site ? wq.get() : nullptr, site ? N : 0, K, seed, first, 1, out1.get(), cls.get(), z1.get(), 1);
    CHECK(r.code == 0);
    CHECK(std::memcmp(z0.get(), z1.get(), N * ncls * sizeof(double)) == 0);
    for (uint64_t s = 0; s < N; ++s)
        for (uint64_t k = 0; k < K; ++k) {
            const int32_t c = cls[s * K + k];
            CHECK(c >= 0 && c < p.ncls);
            if (c >= 0 && c < p.ncls) CHECK(std::memcmp(&out1[(s * K + k) * nq], &out0[((s * ncls + (size_t)c) * K + k) * nq], nq) == 0);
        }
    // ---- the device's layout, job by job: a dirty state vector of 2^state_bits entries and a dirty record of exactly bytes_per_job bytes
    std::vector<double> wxz(site ? row : 4u), P(ncls << tp.n_held), A((size_t)1 << p.width);
    std::vector<uint32_t> reps(ncls * (size_t)p.W), rep((size_t)p.W), chain((size_t)p.W);
    auto bytes = exact<uint8_t>(nq, 0);
    if (!site) sweep::weights_xz(w4, wxz.data());
    const size_t stride = site ? 4u : 0u;
    for (uint64_t s = 0; s < N; ++s) {
        if (site) sweep::site_rows_xz(wq.get() + s * row, 1, p.nq, wxz.data());
        sweep::class_representatives(p, chains.get() + s * nq, reps.data());
        for (size_t i = 0; i < P.size(); ++i) {
            sweep::tiled_representative(tp, &reps[(i >> tp.n_held) * (size_t)p.W], (uint32_t)(i & ((1u << tp.n_held) - 1u)), rep.data());
            P[i] = site ? sweep::sweep_one_wide_site(tp, rep.data(), wxz.data(), A.data()) : sweep::sweep_one_wide(tp, rep.data(), wxz.data(), A.data());
        }
        for (size_t c = 0; c < ncls; ++c)
            for (uint64_t k = 0; k < K; ++k) {
                const uint32_t pick = tp.n_held ? sample::pick_running(&P[c << tp.n_held], 1u << tp.n_held, sample::draw_u53(k, 0u, 0u, first + (uint32_t)s, (uint32_t)c, seed)) : 0u;
                sweep::tiled_representative(tp, &reps[c * (size_t)p.W], pick, rep.data());
                auto work = exact<double>((size_t)1 << tp.state_bits, 0xA5);
                auto R = exact<sample::PairRecord>((size_t)tsp.pairs_per_job, 0x5A);
                device_layout_record(tsp, rep.data(), wxz.data(), stride, work.get(), R.get());
                chain = rep;
                device_layout_walk(tsp, R.get(), k, first + (uint32_t)s, (uint32_t)c, seed, chain.data());
                minplus::unpack_chain(chain.data(), p.nq, bytes.get());
                CHECK(std::memcmp(bytes.get(), &out0[((s * ncls + c) * K + k) * nq], nq) == 0);
            }
    }
    std::printf("  code %d L=%d hbm %d tile %d %s: width %d, held %d, %d FORGETs, %llu bytes per job\n", sh.code, sh.L, sh.hbm_width, sh.tile_width, site ? "site" : "uniform",
                p.width, tp.n_held, tsp.n_forget, (unsigned long long)sample::tiled_sample_bytes_per_job(tsp));
}

void check_refusals()
{
    uint64_t cap = 0;
    CHECK(sample::check_record_bytes("name", 0, &cap).code == 0 && cap == sample::kTiledSampleRecordBytes);
    CHECK(sample::check_record_bytes("name", 12345, &cap).code == 0 && cap == 12345);
    CHECK(sample::check_record_bytes("name", sample::kTiledSampleRecordBytesMax, &cap).code == 0);
    CHECK(sample::check_record_bytes("name", sample::kTiledSampleRecordBytesMax + 1, &cap).code == QECMC_ERR_INVALID);
    const sample::TiledSamplePlan a = sample::build_tiled_sample_plan(2, 13, 0, 0, "entry");
    CHECK(a.tiled.plan.refusal.code == 0 && sample::tiled_sample_bytes_per_job(a) == 128ull * 496896ull && a.n_forget == 168);
    const sample::TiledSamplePlan b = sample::build_tiled_sample_plan(2, 13, 0, 0, "entry", 128ull * 496896ull - 1ull);
    CHECK(b.tiled.plan.refusal.code == QECMC_ERR_UNSUPPORTED && b.tiled.plan.refusal.msg.rfind("entry: the record of one job", 0) == 0 && b.n_forget == 168);
    const sample::TiledSamplePlan c = sample::build_tiled_sample_plan(2, 21, 0, 0, "entry");
    CHECK(c.tiled.plan.refusal.code == QECMC_ERR_UNSUPPORTED && sample::tiled_sample_bytes_per_job(c) == 128ull * 303650944ull);
    const sample::TiledSamplePlan d = sample::build_tiled_sample_plan(2, 21, 0, 0, "entry", sample::kTiledSampleRecordBytesMax);
    CHECK(d.tiled.plan.refusal.code == 0 && d.pair_off.back() <= 0x100000000ull && d.tiled.plan.W == sample::kTiledMaxWords);
    for (int fi = 0; fi < d.n_forget; ++fi) CHECK(d.pair_off[(size_t)fi] == (uint64_t)d.forget_tile[(size_t)fi * sample::kTiledForgetWords + 3u]);
    CHECK(sample::build_tiled_sample_plan(0, 4, 0, 0, "entry").tiled.plan.refusal.code == QECMC_ERR_UNSUPPORTED);
    CHECK(sample::build_tiled_sample_plan(2, 13, 0, 3, "entry").tiled.plan.refusal.msg.rfind("entry: tile_width=3", 0) == 0);
    CHECK(sample::tiled_sample_pass_jobs(16, 128ull * 496896ull, 4096, sample::kTiledSampleRecordBytes) == 67u);
    CHECK(sample::tiled_sample_pass_jobs(16, 128ull * 496896ull, 8, 3ull * 128ull * 496896ull) == 3u);
    CHECK(sample::tiled_sample_pass_jobs(24, 1ull << 40, 5, sample::kTiledSampleRecordBytes) == 1u);
    // the floor of the law, in check_sample_z's words
    const double tiny[4] = {0x1p-962, 1.0, 1.0, 1.0};
    CHECK(sample::check_sample_z("entry", 3, tiny, 4, 0).msg.rfind("entry: row 3, class 0: the class weight is", 0) == 0);
    CHECK(sample::check_sample_z("entry", 3, tiny, 4, 1).code == 0);
}

}  // namespace

int main()
{
    check_refusals();
    const Shape shapes[] = {{1, 5, 0, 4}, {2, 7, 0, 5}, {2, 7, 0, 7}, {0, 3, 0, 6}, {0, 3, 8, 4}, {3, 4, 0, 5}, {2, 9, 0, 8}};
    for (const Shape &sh : shapes) {
        check_shape(sh, false);
        if (sh.L <= 7) check_shape(sh, true);
    }
    if (g_failed) { std::printf("%d checks failed\n", g_failed); return 1; }
    std::printf("class_sample_tiled selftest OK\n");
    return 0;
}
