// The host side of a plan: everything a ladder launch depends on -- which tables exist, every threshold, the LDS size, whether the plan takes a
// work queue and how many workgroups of its persistent grid a CU holds -- decided from a parameter block alone.  Host C++ only (like tables.hpp and
// kernel_choice.hpp; no HIP runtime call): capi.hip uploads what plan_host() built, and tables_test_api.cpp builds it alone with g++, plainly and
// under -fsanitize=address,undefined, so that tests/test_kernel_choice.py and tests/test_host_tables.py see the plans the C-ABI makes.
#pragma once
#include "../../include/qecmc.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "kernel_choice.hpp"
#include "kernels.hpp"
#include "tables.hpp"

namespace qecmc {

// a QECMC_ERR_* code with its message (code 0: accepted); capi.hip's fail() hands it to qecmc_last_error()
struct Refusal {
    int code = 0;
    std::string msg;
};
__attribute__((format(printf, 2, 3))) inline Refusal refuse_params(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return {code, buf};
}

inline Refusal check_code_L(int code, int L)
{
    if (code != QECMC_TORIC && code != QECMC_XZZX && code != QECMC_ROTATED && code != QECMC_PLANAR)
        return refuse_params(QECMC_ERR_INVALID, "code %d unknown (0 toric, 1 xzzx, 2 rotated, 3 planar)", code);
    if (L < 2 || L > 64) return refuse_params(QECMC_ERR_INVALID, "L=%d out of range [2,64]", L);
    if ((code == QECMC_XZZX || code == QECMC_ROTATED) && (L < 3 || L % 2 == 0))
        return refuse_params(QECMC_ERR_INVALID, "L=%d: the xzzx / rotated models need odd L >= 3 (their half-plaquette indexing, xzzx_model.py:444)", L);
    return {};
}

inline size_t code_nq(int code, int L) { return (size_t)code_nq_of(code, L); }

inline Refusal validate_params(const qecmc_params *p)
{
    if (!p) return refuse_params(QECMC_ERR_INVALID, "params is NULL");
    if (p->abi_size != sizeof(qecmc_params))
        return refuse_params(QECMC_ERR_INVALID, "params->abi_size=%u, this library expects %zu", p->abi_size, sizeof(qecmc_params));
    if (Refusal r = check_code_L(p->code, p->L); r.code) return r;
    if (p->Nc < 1 || p->Nc > kMaxNc) return refuse_params(QECMC_ERR_INVALID, "Nc=%d out of range [1,%d]", p->Nc, kMaxNc);
    if (p->noise != QECMC_NOISE_DEPOLARIZING && p->noise != QECMC_NOISE_BIASED && p->noise != QECMC_NOISE_ALPHA) return refuse_params(QECMC_ERR_INVALID, "noise model %d unknown", p->noise);
    if (p->noise == QECMC_NOISE_ALPHA) {
        if (!(p->alpha > 0.0)) return refuse_params(QECMC_ERR_INVALID, "alpha=%g must be positive", p->alpha);
        if (!(p->p > 0.0) || !(p->p <= 1.0)) return refuse_params(QECMC_ERR_INVALID, "pz_tilde=%g must be in (0, 1]", p->p);
        if (p->code == QECMC_TORIC || p->code == QECMC_PLANAR) return refuse_params(QECMC_ERR_UNSUPPORTED, "alpha noise is built for the xzzx and rotated codes (the reference sizes its weights for L^2 qubits, mcmc_alpha.py:27)");
    } else
    if (p->noise == QECMC_NOISE_BIASED) {
        if (!(p->eta > 0.0)) return refuse_params(QECMC_ERR_INVALID, "eta=%g must be positive", p->eta);
        if (!(p->p > 0.0) || !(p->p < (p->eta + 1) / (2 * p->eta + 1))) return refuse_params(QECMC_ERR_INVALID, "p=%g must be in (0, (eta+1)/(2 eta+1))", p->p);
        if (p->code == QECMC_TORIC || p->code == QECMC_PLANAR) return refuse_params(QECMC_ERR_UNSUPPORTED, "biased noise is built for the xzzx and rotated codes (BASELINE config 4)");
    } else if (!(p->p > 0.0) || !(p->p <= 0.75)) return refuse_params(QECMC_ERR_INVALID, "p=%g must be in (0, 0.75]", p->p);
    if (!(p->p_logical >= 0.0) || !(p->p_logical <= 1.0)) return refuse_params(QECMC_ERR_INVALID, "p_logical=%g must be in [0,1]", p->p_logical);
    if (p->scan != QECMC_SCAN_RANDOM && p->scan != QECMC_SCAN_SWEEP && p->scan != QECMC_SCAN_COLOUR && p->scan != QECMC_SCAN_WAVE) return refuse_params(QECMC_ERR_INVALID, "scan mode %d unknown", p->scan);
    if (p->scan != QECMC_SCAN_RANDOM && p->noise != QECMC_NOISE_DEPOLARIZING && !(p->scan == QECMC_SCAN_WAVE && p->noise == QECMC_NOISE_ALPHA) && p->scan != QECMC_SCAN_COLOUR)
        return refuse_params(QECMC_ERR_UNSUPPORTED, "the sweep scan is built for the depolarizing rule only, the wave scan for the depolarizing and alpha rules");
    if (p->scan == QECMC_SCAN_WAVE) {
        if (p->Nc < 2) return refuse_params(QECMC_ERR_UNSUPPORTED, "scan = wave needs a ladder whose top rung sits at p = 0.75 (Nc >= 2)");
        if (p->first_syndrome & 63u) return refuse_params(QECMC_ERR_INVALID, "scan = wave shares a generator pick among the 64 ladders of a wavefront: first_syndrome=%u must be a multiple of 64", p->first_syndrome);
    }
    if (p->scan == QECMC_SCAN_COLOUR) {
        if (p->p_logical > 0.0 && p->Nc < 2 && p->noise != QECMC_NOISE_BIASED) return refuse_params(QECMC_ERR_UNSUPPORTED, "scan = colour needs the top rung at p = 0.75 (Nc >= 2) when logical moves are on");
    }
    if (p->conv_mode != QECMC_CONV_NONE && p->conv_mode != QECMC_CONV_ERROR_BASED) return refuse_params(QECMC_ERR_INVALID, "conv_mode %d unknown", p->conv_mode);
    if (p->conv_mode == QECMC_CONV_ERROR_BASED && (p->TOPS < 0 || p->SEQ < 0 || !(p->eps >= 0))) return refuse_params(QECMC_ERR_INVALID, "TOPS, SEQ and eps must be non-negative");
    if (p->iters == 0 || p->iters > 0xFFFFFFFFull) return refuse_params(QECMC_ERR_INVALID, "iters out of range");
    if (p->tops_burn < 0) return refuse_params(QECMC_ERR_INVALID, "tops_burn must be >= 0");
    if (p->replicas < 0 || p->replicas > 65536) return refuse_params(QECMC_ERR_INVALID, "replicas=%d out of range [0, 65536]", p->replicas);
    // the R ladders of a syndrome add their class counts / samples / tops0 into uint32 outputs: at most `steps` each
    if (p->replicas > 1 && (uint64_t)p->replicas * p->steps > 0xFFFFFFFFull)
        return refuse_params(QECMC_ERR_INVALID, "replicas * steps = %llu overflows the summed 32-bit class counts: lower one of them",
                             (unsigned long long)((uint64_t)p->replicas * p->steps));
    return {};
}

// what the kernel choice reads of a launch
inline KernelShape kernel_shape(const LadderArgs &a)
{
    const uint32_t lower = (1u << (a.Nc - 1)) - 1u;      // rungs below the top
    return {a.code, a.noise, a.scan, a.L, a.Nc, a.W, a.nq, a.ncls, (int)a.n_gen, a.n_types, a.gen_type != nullptr, (int)((a.acc_all_mask >> (a.Nc - 1)) & 1u),
            (a.acc_all_mask & lower) != 0, a.thr_logical != 0, a.conv_mode != 0, a.queue != nullptr, a.uset_tab != nullptr, a.xyz_thr != nullptr,
            a.swap_acc != nullptr ? 1 : a.short_neff != nullptr ? 2 : 0, a.resume != 0, a.neff != nullptr, (a.bias_f32ok & lower) == lower, a.swap_fast_ok != 0,
            a.iters > 0x7FFFFFFFu ? 0x7FFFFFFF : (int)a.iters, (int)a.tune};
}
inline bool same_shape(const KernelShape &a, const KernelShape &b) { return std::memcmp(&a, &b, sizeof a) == 0; }   // (ints only: no padding)

// A plan before its upload: `args` with every scalar and fixed-size array set and every device pointer null, the tables a launch reads (an empty
// vector: the plan has no such table and the pointer stays null -- gen, swap_thr, lmask and acc_top are uploaded always), and what the plan says of
// its launches.  `shape` is kernel_shape() of the uploaded plan with nothing of a launch attached (capi.hip checks that after the upload).
struct HostPlan {
    LadderArgs args;
    std::vector<uint32_t> gen, xyz_lut, wu_desc, col_thr, lmask, acc_top;
    std::vector<uint8_t> gen_type;
    std::vector<uint16_t> phases;
    std::vector<double> bias, lnb;
    std::vector<uint64_t> swap_thr;
    KernelShape shape;
    size_t lds_bytes = 0;
    bool takes_queue = false;           // a criterion launch offered a work queue runs a queue kernel ...
    int queue_family = kRefused;        // ... of this family (kFamLadder: fed from a counter the plan owns) ...
    uint32_t queue_per_cu = 0;          // ... on a persistent grid of this many workgroups per CU
};

// First phase: the code's dimensions, the launch scalars, the generator table and its Pauli patterns -- the static fields of the plan's shape
// (W, nq, ncls, n_gen, n_types, gen_type).  Refuses what no kernel path can stage in LDS.
inline Refusal plan_dims(const qecmc_params &p, HostPlan &hp)
{
    hp = HostPlan();
    LadderArgs &a = hp.args;
    std::memset(&a, 0, sizeof a);
    const int L = p.L, nq = (int)code_nq(p.code, L);
    a.code = p.code; a.noise = p.noise; a.scan = p.scan; a.alpha = p.alpha;
    a.replicas = p.replicas > 1 ? (uint32_t)p.replicas : 1u;
    a.tune = p.flags & 0xFFFFu;                                // developer switches (qecmc_flag): which variant runs, never what it computes
    a.L = L; a.Nc = p.Nc; a.W = (nq + 15) / 16; a.nq = nq; a.ncls = p.code == QECMC_TORIC ? 16 : 4;
    a.iters = (uint32_t)p.iters;
    a.seed_lo = (uint32_t)p.seed; a.seed_hi = (uint32_t)(p.seed >> 32);
    a.tops_burn = (uint32_t)p.tops_burn;
    a.conv_mode = p.conv_mode; a.TOPS = (uint32_t)p.TOPS; a.SEQ = (uint32_t)p.SEQ; a.eps = p.eps;
    a.thr_logical = p.p_logical > 0 ? tables::thr64(p.p_logical) : 0;
    a.n_gen = p.code == QECMC_TORIC ? 2u * L * L : (uint32_t)surf_ngen(p.code, L);
    if (a.n_gen > kMaxGenLds)   // every kernel path stages the generator table in LDS
        return refuse_params(QECMC_ERR_UNSUPPORTED, "L=%d: %u generators exceed the LDS table of %u (needed by scan=1 and by the xzzx / rotated codes)", L, a.n_gen, kMaxGenLds);
    hp.gen = p.code == QECMC_TORIC ? tables::toric_generator_table(L) : tables::surf_generator_table(p.code, L);
    // the generators' Pauli patterns: the biased rules' count-change table, the plaquette codes' dE table (ladder_kernel.hpp, DELUT)
    if (p.noise != QECMC_NOISE_DEPOLARIZING || (p.code != QECMC_TORIC && !p.scan)) {
        std::vector<uint32_t> patterns;
        tables::generator_patterns(hp.gen, hp.gen_type, patterns);
        if (patterns.size() > 16) return refuse_params(QECMC_ERR_UNSUPPORTED, "%zu distinct generator Pauli patterns (> 16)", patterns.size());
        a.n_types = (int)patterns.size();
        for (size_t t = 0; t < patterns.size(); ++t) a.type_ops[t] = (uint8_t)patterns[t];
    }
    return {};
}

// The whole host plan of a parameter block validate_params() accepts.  Each refusal comes before any that could also apply further down.
inline Refusal plan_host(const qecmc_params &p, HostPlan &hp)
{
    using namespace tables;
    if (Refusal r = plan_dims(p, hp); r.code) return r;
    LadderArgs &a = hp.args;
    const int L = a.L, Nc = a.Nc, nq = a.nq, W = a.W, ncls = a.ncls;
    const bool alpha = p.noise == QECMC_NOISE_ALPHA;
    const bool biased = p.noise == QECMC_NOISE_BIASED || alpha;     // table-driven acceptance pn / pb
    if (biased) {
        // the biased / alpha rules' table of count changes (tables.hpp)
        if (nq > 511) return refuse_params(QECMC_ERR_UNSUPPORTED, "biased / alpha noise packs the error counts in 10-bit fields: nq=%d", nq);
        std::vector<uint32_t> patterns(a.type_ops, a.type_ops + a.n_types);
        hp.xyz_lut = count_change_table(patterns);
    }
    if (p.scan != QECMC_SCAN_COLOUR) {     // (scan = colour: its LDS holds the swap thresholds, known further down)
        hp.lds_bytes = p.scan == QECMC_SCAN_WAVE ? wu_plan_lds_bytes(Nc, W, ncls, L, p.conv_mode != 0, alpha, p.iters)
                                                 : ladder_lds_bytes(Nc, W, ncls, ladder_gen_dwords(p.code, p.noise, p.scan, a.n_gen, Nc, nq, a.n_types));
        if (hp.lds_bytes > 160 * 1024)
            return refuse_params(QECMC_ERR_UNSUPPORTED, "L=%d Nc=%d needs %zu B of LDS per workgroup (> 160 KiB)", L, Nc, hp.lds_bytes);
    }

    std::vector<double> pladder, pdiff;
    // p_top = 0.75 (mcmc.py:62) or (eta+1)/(2 eta+1) (mcmc_biased.py:81)
    // ... or pz_tilde_top = 1 (mcmc_alpha.py:94)
    ladder_probabilities(p.p, alpha ? 1.0 : biased ? (p.eta + 1) / (2 * p.eta + 1) : 0.75, Nc, pladder, pdiff);   // mcmc.py:62-69
    if (alpha) pdiff.assign(pdiff.size(), 0.0);      // the depolarizing tables below are unused by the table-driven rules
    hp.acc_top.assign(nq + 1, 0u);                                         // mcmc.py:34 for a top chain below p = 0.75
    if (!biased) {
        for (int c = 0; c < Nc; ++c) {
            const double f = chain_factor(pladder[c]);
            if (f >= 1.0) a.acc_all_mask |= 1u << c;
            for (int d = 1; d <= 4; ++d) {
                a.acc_thr[c][d - 1] = thr32(std::pow(f, (double)d));                     // mcmc.py:42
                a.acc_thr44[c][d - 1] = thr44(std::pow(f, (double)d));
            }
        }
        for (int d = 1; d <= nq; ++d) hp.acc_top[d] = thr32(std::pow(chain_factor(pladder[Nc - 1]), (double)d));
        // scan = sweep and scan = colour test x <= ceil(f^dE 2^32) - 1 (ladder_kernel.hpp thrT, ladder_colour_body.inc thr1 .. thr4), which has no
        // word for "never": a threshold of 0 -- f^dE underflows to 0 in double precision, f^4 first, at p below about 3.7e-81 -- would wrap to
        // "always".  (scan = random and scan = wave test x < threshold and serve every p.)
        if (p.scan == QECMC_SCAN_SWEEP || p.scan == QECMC_SCAN_COLOUR)
            for (int c = 0; c < Nc; ++c)
                if (!((a.acc_all_mask >> c) & 1u) && a.acc_thr[c][3] == 0)
                    return refuse_params(QECMC_ERR_UNSUPPORTED, "scan = %s: the acceptance ratio f^4 of rung %d underflows to 0 at p=%g (f = (p / 3) / (1 - p); every p >= 1e-80 "
                                         "is served, and scan = random / scan = wave serve every p)", p.scan == QECMC_SCAN_SWEEP ? "sweep" : "colour", c, pladder[c]);
    }
    hp.swap_thr = swap_thresholds(pdiff, nq);                                // mcmc.py:149
    a.swap_fast_ok = 1;
    for (int i = 0; i + 1 < Nc; ++i) {
        const double l2 = std::log2(pdiff[i]);
        a.swap_inv_log2[i] = (std::isfinite(l2) && l2 < 0) ? (float)(1.0 / l2) : 0.0f;
        if (nq >= 1 && hp.swap_thr[(size_t)i * (nq + 1) + 1] > 0xFFFFFFFFull) a.swap_fast_ok = 0;
    }
    hp.lmask = p.code == QECMC_TORIC ? toric_logical_masks(L, W) : surf_logical_masks(p.code, L, W);
    if (p.scan == QECMC_SCAN_COLOUR) {
        // the colour phases: groups of mutually disjoint generators, one wavefront pass each (tables.hpp)
        int n_phases = 0;
        hp.phases = colour_phases(hp.gen, n_phases);
        a.n_phases = (uint32_t)n_phases;
        // Ladder_alpha's top rung sits at pz_tilde = 1 (mcmc_alpha.py:94): every weight ratio is 1, it takes the coin like the depolarizing top rung
        if (alpha && Nc >= 2) a.acc_all_mask |= 1u << (Nc - 1);
        hp.lds_bytes = sizeof(uint32_t) * colour_lds_dwords(Nc, W, ncls, a.n_phases, a.n_gen, L, nq, a.swap_fast_ok != 0, p.noise);
        if (hp.lds_bytes > 160 * 1024)
            return refuse_params(QECMC_ERR_UNSUPPORTED, "scan = colour: L=%d Nc=%d needs %zu B of LDS per workgroup (> 160 KiB)", L, Nc, hp.lds_bytes);
        if (p.p_logical > 0.0 && p.noise != QECMC_NOISE_BIASED && !((a.acc_all_mask >> (Nc - 1)) & 1u))
            return refuse_params(QECMC_ERR_UNSUPPORTED, "scan = colour needs a top rung that accepts every move (p_top = 0.75) when logical moves are on");
    }
    if (p.scan == QECMC_SCAN_WAVE) {
        // the wave-uniform random scan (ladder_wu.hpp): one scalar-loadable descriptor per generator; states in registers
        // (a wave plan launches ladder_wu kernels only -- choose_kernel: scan = 3 is choose_wave or a refusal --, so the toric code's tables are in
        // the wave layout, tables.hpp: the other kernel families read lmask in the flat one)
        const bool cells = p.code == QECMC_TORIC;
        hp.wu_desc = cells ? toric_wave_descriptors(hp.gen) : wave_descriptors(hp.gen);
        if (cells) hp.lmask = wave_layout_rows(p.code, L, nq, W, hp.lmask);
        if (hp.wu_desc.empty()) return refuse_params(QECMC_ERR_UNSUPPORTED, "scan = wave: a generator with three different Paulis");
    }
    if (biased) {
        for (int c = 0; c < Nc; ++c) {
            const std::vector<double> t = alpha ? alpha_tables(pladder[c], p.alpha, (size_t)nq) : bias_tables(pladder[c], p.eta, (size_t)nq);
            hp.bias.insert(hp.bias.end(), t.begin(), t.end());
        }
        if (p.scan == QECMC_SCAN_COLOUR) hp.col_thr.resize((size_t)Nc * 81);
        for (int c = 0; c < Nc; ++c) {
            // px / pI, pz / pI of rung c (px = py in both models: bias_tables / alpha_tables); their log2 are the fast test's slopes
            const double *t = &hp.bias[(size_t)c * 4 * (nq + 1)];
            const double fxy = t[1] / t[3 * (nq + 1) + 1], fz = t[2 * (nq + 1) + 1] / t[3 * (nq + 1) + 1];
            a.bias_l2[c][0] = std::log2(fxy);
            a.bias_l2[c][1] = std::log2(fz);
            a.bias_l2f[c][0] = (float)a.bias_l2[c][0];
            a.bias_l2f[c][1] = (float)a.bias_l2[c][1];
            // the fast test may run in single precision / fp16 count changes on this rung (ladder_kernel.hpp: a count changes by at
            // most 4 per proposal since loop entry; fp16 holds integers up to 2048; |l d| <= 2000 keeps the exponent's error below a unit)
            if (a.iters <= 512u && 4.0 * (double)a.iters * std::max(std::fabs(a.bias_l2[c][0]), std::fabs(a.bias_l2[c][1])) <= 2000.0)
                a.bias_f32ok |= 1u << c;
            if (p.scan != QECMC_SCAN_COLOUR) continue;
            // scan = 2 under these rules (ladder_colour.hpp): a generator is a Metropolis move for the model's own weight, accepted iff
            // u < (px / pI)^dxy (pz / pI)^dz -- as integers, u <= ceil(ratio 2^32) - 1 -- for its changes (dz, dxy) of n_z and n_x + n_y
            for (int dz = -4; dz <= 4; ++dz)
                for (int dxy = -4; dxy <= 4; ++dxy) {
                    const uint64_t th = thr64(std::pow(fxy, (double)dxy) * std::pow(fz, (double)dz));
                    if (th == 0) return refuse_params(QECMC_ERR_UNSUPPORTED, "scan = colour: an acceptance ratio of rung %d underflows", c);
                    hp.col_thr[(size_t)c * 81 + 9 * (dz + 4) + (dxy + 4)] = (uint32_t)(th - 1);
                }
        }
    }
    if (alpha) {
        hp.lnb.assign(Nc > 1 ? Nc - 1 : 1, 0.0);
        for (int i = 0; i + 1 < Nc; ++i) hp.lnb[i] = std::log(pladder[i] / pladder[i + 1]);   // mcmc_alpha.py:123
    }
    hp.shape = kernel_shape(a);
    hp.shape.gen_type = !hp.gen_type.empty();      // (the upload sets the pointer kernel_shape() reads)
    if (p.scan == QECMC_SCAN_WAVE && !choose_kernel(hp.shape).ok())
        return refuse_params(QECMC_ERR_UNSUPPORTED, "scan = wave: L=%d Nc=%d p=%g is outside what it is built for (depolarizing rule: a top rung that accepts every move, at most "
                             "16 packed state words per rung -- toric / planar L <= 11, xzzx / rotated L <= 16 --, fixed-length runs of up to 8 rungs 32 words -- toric L <= 16, xzzx / rotated L <= 22; alpha rule: xzzx / rotated L <= 11, "
                             "4 iters max|log2 ratio| <= 2000 --, %zu B of LDS)", L, Nc, p.p, hp.lds_bytes);
    // runs that stop by the convergence criterion, where the kernel takes a work queue: a persistent grid (what one launch keeps resident) fed
    // from a counter (scan = wave: the workgroups' own shares of the batch), of as many workgroups as the LDS and the kernel's occupancy let a CU hold
    KernelShape offered = hp.shape;
    offered.queue = 1;
    const KernelKey queue_kernel = choose_kernel(offered);
    if (queue_kernel.takes_queue()) {
        const size_t per_cu_lds = (160 * 1024) / hp.lds_bytes, per_cu_waves = (size_t)(4 * queue_kernel.minw) / (size_t)Nc;
        hp.takes_queue = true;
        hp.queue_family = queue_kernel.family;
        hp.queue_per_cu = (uint32_t)std::max<size_t>(1, std::min(per_cu_lds, per_cu_waves));
    }
    return {};
}

// the persistent grid of a plan on a device of cu_count CUs (0: not a queue plan); bits 16-31 of qecmc_params.flags override it (tests: force
// refills on small batches)
inline uint32_t queue_grid(const HostPlan &hp, int cu_count, uint32_t flags)
{
    if (!hp.takes_queue) return 0;
    const uint32_t grid = flags >> 16 ? flags >> 16 : (uint32_t)((size_t)hp.queue_per_cu * (size_t)cu_count);
    return grid ? grid : 1;
}

// The key of a plan: exactly the fields plan_host() reads (and the device the tables are uploaded to), in a zeroed struct -- not the caller's block
// with its padding, first_syndrome and step count.  The seed is left out on purpose: plan_host() copies it into args.seed_lo / seed_hi and nothing
// else depends on it, and the step entry points, the only users of the key, patch those two words per call -- a key with the seed would make a
// cache miss of every ladder with its own seed.
inline qecmc_params plan_key(const qecmc_params &p)
{
    qecmc_params k;
    std::memset(&k, 0, sizeof k);
    k.abi_size = p.abi_size; k.code = p.code; k.L = p.L; k.Nc = p.Nc; k.noise = p.noise; k.scan = p.scan; k.conv_mode = p.conv_mode; k.device = p.device;
    k.iters = p.iters; k.tops_burn = p.tops_burn; k.TOPS = p.TOPS; k.SEQ = p.SEQ; k.replicas = p.replicas; k.eps = p.eps; k.p = p.p; k.eta = p.eta;
    k.alpha = p.alpha; k.p_logical = p.p_logical; k.flags = p.flags;
    return k;
}

// The shortest-chain statistics (qecmc_plan_set_shortest): slots of a ladder's set of `set_capacity` distinct keys -- the smallest power of two that is at
// least twice as many --, THE formula of the set workspace, and what the statistics refuse of a plan before they look at a buffer (the chooser's text).
inline uint64_t shortest_set_slots(uint64_t set_capacity) { uint64_t s = 2; while (s < 2 * set_capacity) s <<= 1; return s; }
constexpr uint64_t kShortMaxCapacity = uint64_t(1) << 26;
inline uint64_t shortest_set_need(uint64_t N, uint64_t set_capacity) { return N * shortest_set_slots(set_capacity) * sizeof(uint64_t); }
inline Refusal shortest_check(const qecmc_params &prm, const KernelShape &plan_shape)
{
    KernelShape s = plan_shape;
    s.stats = 2;
    if (const KernelKey k = choose_kernel(s); !k.ok()) return refuse_params(QECMC_ERR_UNSUPPORTED, "qecmc_plan_set_shortest: %s", k.why);
    if (prm.replicas > 1) return refuse_params(QECMC_ERR_UNSUPPORTED, "qecmc_plan_set_shortest: the statistics are per ladder: not with replicas > 1");
    return {};
}

// LDS bytes of a workgroup of the shortest-chain kernels (the plan's args: scan = wave or colour under the alpha rule): what launch_ladder asks for, what
// qecmc_plan_set_shortest holds against the 160 KiB of a workgroup and qecmc_plan_info reports while the statistics are set
inline size_t shortest_lds_bytes(const LadderArgs &a)
{
    if (a.scan == QECMC_SCAN_WAVE) return wu_lds_bytes(a.Nc, a.W, a.ncls, a.L, true, true, true);
    return sizeof(uint32_t) * colour_lds_dwords(a.Nc, a.W, a.ncls, a.n_phases, a.n_gen, a.L, a.nq, a.swap_fast_ok != 0, a.noise, true);
}

// a criterion launch of `steps` ladder steps runs on the plan's persistent grid unless it asks for final states or statistics
inline bool launch_takes_queue(uint32_t queue_grid, uint64_t steps, bool wants_states_or_stats) { return queue_grid != 0 && !wants_states_or_stats && steps > 0; }
// the persistent grid a scan = wave criterion launch of M ladders runs on, and the ladders each of its workgroups owns
inline void wave_queue_shape(uint32_t queue_grid, uint64_t M, uint32_t *grid, uint32_t *chunk)
{
    // (whole groups of 64 per workgroup: a batch that gives every ladder a lane of its own is laid out like a launch without the queue,
    // ladder l in lane l & 63 of workgroup l >> 6, and gives the same results whatever the grid)
    const uint64_t groups = (M + 63) / 64, g = std::max<uint64_t>(1, std::min<uint64_t>(queue_grid, groups)), c = ((M + g - 1) / g + 63) / 64 * 64;
    *chunk = (uint32_t)c;
    *grid = (uint32_t)((M + c - 1) / c);
}
// THE workspace formula of the criterion runs (the one place it lives): one log entry per (ladder step, column) -- the bottom chain's
// error count (u16), or for alpha noise the two counts behind n_eff (2 x u16) -- with one column per ladder (rounded up to whole
// 64-lane groups), or, when the launch runs on the plan's persistent grid with a work queue, one per lane of that grid.
inline uint64_t workspace_need(const qecmc_params &prm, uint32_t queue_grid, uint64_t N, bool queue)
{
    if (prm.conv_mode != QECMC_CONV_ERROR_BASED) return 0;
    const uint64_t M = N * (prm.replicas > 1 ? (uint64_t)prm.replicas : 1u);
    uint64_t cols = (M + 63) / 64 * 64;
    if (queue && prm.scan == QECMC_SCAN_WAVE) {
        uint32_t grid, chunk;
        wave_queue_shape(queue_grid, M, &grid, &chunk);
        cols = (uint64_t)grid * 64u;
    } else if (queue) {
        cols = std::min<uint64_t>(cols, (uint64_t)queue_grid * 64u);
    }
    return (prm.noise == QECMC_NOISE_ALPHA ? 4ull : 2ull) * cols * prm.steps;
}

// THE sizes of a criterion run continued from device state (qecmc_pteq_resume_conv_dev): the per-ladder criterion records (kernels.hpp,
// ConvRecWord) and a log of `log_rows` rows, row = the ladder's absolute step, in the layout of workspace_need() without a queue.  Both 0
// for a plan without the criterion.
struct ResumeConvBytes { uint64_t record, log; };
inline ResumeConvBytes resume_conv_need(const qecmc_params &prm, uint64_t N, uint64_t log_rows)
{
    if (prm.conv_mode != QECMC_CONV_ERROR_BASED) return {0, 0};
    qecmc_params one = prm;
    one.replicas = 0;
    one.steps = log_rows;
    return {sizeof(uint32_t) * (uint64_t)conv_record_words(prm.noise) * N, workspace_need(one, 0, N, false)};
}
// what qecmc_pteq_resume_conv_dev refuses of a plan, before it looks at a buffer
inline Refusal resume_conv_check(const qecmc_params &prm)
{
    if (prm.conv_mode != QECMC_CONV_ERROR_BASED)
        return refuse_params(QECMC_ERR_INVALID, "qecmc_pteq_resume_conv_dev continues criterion runs: conv_mode must be error_based (fixed-length chunks: qecmc_pteq_resume_dev)");
    if (prm.scan == QECMC_SCAN_WAVE)
        return refuse_params(QECMC_ERR_UNSUPPORTED, "scan = wave runs the criterion on its persistent grid, where a ladder's lane is reused when it has stopped: no continuation from device state");
    if (prm.scan == QECMC_SCAN_COLOUR)
        return refuse_params(QECMC_ERR_UNSUPPORTED, "scan = colour starts its ladders from seed configurations: no chunked continuation");
    if (prm.replicas > 1) return refuse_params(QECMC_ERR_INVALID, "qecmc_pteq_resume_conv_dev continues single ladders: replicas must be <= 1");
    return {};
}

// THE range of the Philox addresses (philox.hpp, DESIGN.md "RNG addressing"): a counter holds a proposal index -- or a ladder-step index, swap stream --
// in 48 bits, c0 = k[31:0], c1[15:0] = k[47:32], so index 2^48 + k would draw the blocks of index k again.  The entry points that take a start
// index (step0 / prop0 / k0) refuse a call whose last index, plus kRngIndexSlack, is not below 2^48 (the slack: the colour kernels address the top
// rung's block of phase K as K + lane), or whose step0 * iters / prop0 + nsteps * iters does not fit 64 bits -- before anything is enqueued.
// The call runs ladder steps [step0, step0 + nsteps) and proposals [prop0, prop0 + nsteps * iters) (a single chain: nsteps = 1, prop0 = k0).
constexpr uint64_t kRngIndexLimit = 1ull << 48;
constexpr uint64_t kRngIndexSlack = 64;
inline Refusal rng_range_check(const char *who, uint64_t step0, uint64_t nsteps, uint64_t prop0, uint64_t iters)
{
    constexpr uint64_t kEndMax = kRngIndexLimit - kRngIndexSlack;         // the largest accepted one-past-the-last index
    uint64_t props = 0, prop_end = 0, step_end = 0;
    if (__builtin_mul_overflow(nsteps, iters, &props) || __builtin_add_overflow(prop0, props, &prop_end))
        return refuse_params(QECMC_ERR_INVALID, "%s: proposals %llu + %llu steps x %llu iters overflow 64 bits (the Philox counter holds 48: last index + %llu < 2^48)", who,
                             (unsigned long long)prop0, (unsigned long long)nsteps, (unsigned long long)iters, (unsigned long long)kRngIndexSlack);
    if (prop_end > kEndMax)
        return refuse_params(QECMC_ERR_INVALID, "%s: proposals %llu .. %llu (start %llu, %llu steps x %llu iters) leave the 48-bit Philox counter: the last index + %llu must be below 2^48 = %llu",
                             who, (unsigned long long)prop0, (unsigned long long)(prop_end - (props ? 1 : 0)), (unsigned long long)prop0, (unsigned long long)nsteps,
                             (unsigned long long)iters, (unsigned long long)kRngIndexSlack, (unsigned long long)kRngIndexLimit);
    if (__builtin_add_overflow(step0, nsteps, &step_end) || step_end > kEndMax)
        return refuse_params(QECMC_ERR_INVALID, "%s: ladder steps %llu + %llu leave the 48-bit Philox counter of the swap stream: the last index + %llu must be below 2^48 = %llu", who,
                             (unsigned long long)step0, (unsigned long long)nsteps, (unsigned long long)kRngIndexSlack, (unsigned long long)kRngIndexLimit);
    return {};
}
// ... of a run continued at ladder step step0, whose first proposal is step0 * iters (qecmc_pteq_resume_dev, qecmc_pteq_resume_conv_dev)
inline Refusal rng_range_check_resume(const char *who, uint64_t step0, uint64_t nsteps, uint64_t iters)
{
    uint64_t prop0 = 0;
    if (__builtin_mul_overflow(step0, iters, &prop0))
        return refuse_params(QECMC_ERR_INVALID, "%s: step0 * iters = %llu * %llu overflows 64 bits (the Philox counter holds 48: last proposal index + %llu < 2^48)", who,
                             (unsigned long long)step0, (unsigned long long)iters, (unsigned long long)kRngIndexSlack);
    return rng_range_check(who, step0, nsteps, prop0, iters);
}

}  // namespace qecmc
