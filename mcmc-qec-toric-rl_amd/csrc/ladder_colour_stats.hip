// scan = 2 with the observables of qecmc_plan_set_stats (ladder_colour.hpp): the instantiations of ladder_colour_stats_kernel, every code and rule
// the colour kernel runs.
#include "ladder_colour.hpp"

namespace qecmc {

template <int CODE, int RULE>
struct ColourStatsSet {
    static const void *find(const KernelKey &k) { return k == colour_stats_key(CODE, RULE) ? (const void *)ladder_colour_stats_kernel<CODE, RULE> : nullptr; }
};

const void *colour_stats_kernel(const KernelKey &k)
{
    return find_kernel<ColourStatsSet<kCodeToric, 0>, ColourStatsSet<kCodeXzzx, 0>, ColourStatsSet<kCodeRotated, 0>, ColourStatsSet<kCodePlanar, 0>,
                       ColourStatsSet<kCodeXzzx, 1>, ColourStatsSet<kCodeRotated, 1>, ColourStatsSet<kCodeXzzx, 2>, ColourStatsSet<kCodeRotated, 2>>(k);
}

}  // namespace qecmc
