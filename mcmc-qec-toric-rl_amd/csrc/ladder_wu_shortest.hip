// scan = 3 with the shortest-chain statistics of qecmc_plan_set_shortest (ladder_wu.hpp SHORT): the alpha rule's queue kernel on the xzzx / rotated codes
// at 4 and 8 state words per rung, the unrolled proposal loop of iters = 10 and the general one.
#include "ladder_wu.hpp"

namespace qecmc {

const void *wave_shortest_kernel(const KernelKey &k)
{
    return find_kernel<WaveShortestSet<kCodeXzzx, 4>, WaveShortestSet<kCodeXzzx, 8>, WaveShortestSet<kCodeRotated, 4>, WaveShortestSet<kCodeRotated, 8>>(k);
}

}  // namespace qecmc
