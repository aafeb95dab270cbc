// scan = 3 with the observables of qecmc_plan_set_stats (ladder_wu.hpp STATS): the instantiations of ladder_wu_stats_kernel under the depolarizing
// rule, every code at 4 .. 16 state words per rung.
#include "ladder_wu.hpp"

namespace qecmc {

template <int CODE>
using WaveStatsWords = KernelList<WaveStatsSet<CODE, 4>, WaveStatsSet<CODE, 8>, WaveStatsSet<CODE, 12>, WaveStatsSet<CODE, 16>>;

const void *wave_stats_kernel(const KernelKey &k)
{
    return find_kernel<WaveStatsWords<kCodeToric>, WaveStatsWords<kCodeXzzx>, WaveStatsWords<kCodeRotated>, WaveStatsWords<kCodePlanar>>(k);
}

}  // namespace qecmc
