// scan = 3 with the observables of qecmc_plan_set_stats under the alpha noise model (ladder_wu.hpp STATS, ALPHA): the xzzx / rotated instantiations
// of ladder_wu_stats_kernel at 4 and 8 state words per rung.
#include "ladder_wu.hpp"

namespace qecmc {

const void *wave_stats_alpha_kernel(const KernelKey &k)
{
    return find_kernel<WaveStatsSet<kCodeXzzx, 4, true>, WaveStatsSet<kCodeXzzx, 8, true>, WaveStatsSet<kCodeRotated, 4, true>,
                       WaveStatsSet<kCodeRotated, 8, true>>(k);
}

}  // namespace qecmc
