// The one launch path of the ladder kernels: choose_kernel() (kernel_choice.hpp) names the kernel of a launch, the instantiation units
// (ladder_toric / ladder_surf / ladder_biased / ladder_uset / ladder_colour* / ladder_wu*.hip, built in parallel) hold it,
// and the launch runs it on the grid its family implies.  A key no unit holds is an error, never a neighbouring kernel.
#include "kernels.hpp"
#include "plan_host.hpp"   // kernel_shape(): what the choice reads of a launch

namespace qecmc {

namespace {

const void *kernel_of(const KernelKey &k)
{
    const void *fn = nullptr;
    for (auto unit : {ladder_toric_kernel, ladder_surf_kernel, ladder_biased_kernel, ladder_sweep_kernel, ladder_uset_kernel, colour_kernel,
                      wave_toric_kernel, wave_xzzx_kernel, wave_rotated_kernel, wave_planar_kernel, wave_alpha_kernel, wave_stats_kernel,
                      wave_stats_alpha_kernel, colour_stats_kernel, wave_shortest_kernel, colour_shortest_kernel})
        fn = fn ? fn : unit(k);
    return fn;
}

// the key of the last kernel this thread handed to the runtime (qecmc_last_kernel): one 48-byte copy per launch, nothing else
thread_local KernelKey t_last_kernel = {kRefused, 0, 0, 0, 0u, 0, 0, 0, 0, 0, nullptr};
inline void note_kernel(const KernelKey &k) { t_last_kernel = k; }

hipError_t launch_fn(const void *fn, const LadderArgs &a, hipStream_t stream, unsigned grid, size_t lds)
{
    if (lds > 64 * 1024) {   // beyond the default dynamic-LDS window (160 KiB per CU on gfx950)
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    void *kargs[] = {const_cast<LadderArgs *>(&a)};
    const hipError_t e = hipLaunchKernel(fn, dim3(grid), dim3((unsigned)a.Nc * 64u), kargs, lds, stream);
    return e != hipSuccess ? e : hipGetLastError();
}

}  // namespace

// ladder_kernel: one 64-syndrome group (Nc waves) per workgroup (two per workgroup measured slower at every batch size); `persistent`: fn is a
// QUEUE instantiation -- only those run on the capped grid, and a.queue without one is an error: a plain kernel never skips ladders
hipError_t launch_ladder_fn(const void *fn, const KernelKey &k, const LadderArgs &a, hipStream_t stream, bool persistent)
{
    unsigned grid = (unsigned)((a.N + 63) / 64);
    if ((a.queue != nullptr) != persistent) return hipErrorInvalidValue;
    if (persistent && a.grid_cap && grid > a.grid_cap) grid = a.grid_cap;
    const size_t lds = ladder_launch_lds(kernel_shape(a));
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    note_kernel(k);
    return launch_fn(fn, a, stream, grid, lds);
}

hipError_t launch_ladder(const LadderArgs &a, hipStream_t stream)
{
    if (a.N == 0) return hipSuccess;
    const KernelKey k = choose_kernel(kernel_shape(a));
    const void *fn = k.ok() ? kernel_of(k) : nullptr;
    if (!fn) return hipErrorInvalidValue;
    const bool shortest = (k.family == kFamWave || k.family == kFamColour) && k.flags == kKeyShort;   // (ladder_kernel's flags are a LadderFlag mask)
    if (shortest) {
        // qecmc_plan_set_shortest: every output and the ladders' sets (zeroed by the caller), fresh single ladders; the criterion needs its log
        if (!a.short_neff || !a.short_n || !a.short_uniq || !a.short_over || !a.short_set || a.short_cap == 0 || a.short_slots < 2u * a.short_cap ||
            (a.short_slots & (a.short_slots - 1u)) || a.replicas > 1 || a.resume || a.swap_acc || a.step0 || a.nsteps == 0 || (a.conv_mode != 0 && a.nlog == nullptr))
            return hipErrorInvalidValue;
    }
    if (shortest && k.family == kFamWave) {
        // ... on scan = 3 the queue kernel with one ladder per lane for the whole run: a workgroup owns 64 ladders, no lane is ever refilled, and the
        // layout -- ladder l in lane l & 63 of workgroup l >> 6, one log column per ladder -- is that of a launch without the queue
        if (a.wu_desc == nullptr || (a.first_syndrome & 63u) || a.bias_tbl == nullptr || a.alpha_lnb == nullptr || a.write_states) return hipErrorInvalidValue;
        LadderArgs b = a;
        b.wu_chunk = 64u; b.wu_once = 0u; b.queue = nullptr; b.grid_cap = 0u;
        note_kernel(k);
        return launch_fn(fn, b, stream, (unsigned)((a.N + 63) / 64), shortest_lds_bytes(a));
    }
    if (k.family == kFamWave) {
        // scan = 3: batches start on a multiple of 64 (a wavefront shares its generator picks); the criterion runs on a persistent grid of
        // a.grid_cap workgroups (capi.hip), each owning a.wu_chunk ladders of the batch
        if (a.wu_desc == nullptr || (a.first_syndrome & 63u) || (a.noise == 2 && (a.bias_tbl == nullptr || a.alpha_lnb == nullptr))) return hipErrorInvalidValue;
        if (k.conv && (a.nlog == nullptr || a.resume || a.write_states || a.wu_chunk < 64u || (a.wu_chunk & 63u))) return hipErrorInvalidValue;
        const uint64_t per = k.conv ? a.wu_chunk : 64u;
        LadderArgs b = a;
        b.wu_once = (uint32_t)wave_cascade_mode(kernel_shape(a));
        note_kernel(k);
        return launch_fn(fn, b, stream, (unsigned)((a.N + per - 1) / per), wu_lds_bytes(a.Nc, a.W, a.ncls, a.L, k.conv, k.alpha, false, wu_frame_steps(k.wv, k.conv, k.alpha, k.it)));
    }
    if (k.family == kFamColour) {
        // scan = 2: one ladder per workgroup
        if (a.phase_tab == nullptr || a.n_phases == 0 || (a.conv_mode != 0 && a.nlog == nullptr)) return hipErrorInvalidValue;
        if (a.noise != 0 && (a.col_thr == nullptr || a.bias_tbl == nullptr || (a.noise == 2 && a.alpha_lnb == nullptr))) return hipErrorInvalidValue;
        const size_t lds = shortest ? shortest_lds_bytes(a) : sizeof(uint32_t) * colour_lds_dwords(a.Nc, a.W, a.ncls, a.n_phases, a.n_gen, a.L, a.nq, a.swap_fast_ok != 0, a.noise);
        if (lds > 160 * 1024) return hipErrorInvalidValue;
        note_kernel(k);
        return launch_fn(fn, a, stream, (unsigned)a.N, lds);
    }
    return launch_ladder_fn(fn, k, a, stream, k.takes_queue());
}

// the key launch_ladder() last launched on this thread; false: it has launched nothing yet (an N == 0 call and a refused launch leave the key untouched)
bool last_launched_kernel(KernelKey &out)
{
    out = t_last_kernel;
    return t_last_kernel.ok();
}

}  // namespace qecmc
