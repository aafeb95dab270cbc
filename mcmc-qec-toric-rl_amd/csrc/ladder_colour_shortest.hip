// scan = 2 with the shortest-chain statistics of qecmc_plan_set_shortest (ladder_colour.hpp): the alpha rule's criterion kernel on the xzzx / rotated codes.
#include "ladder_colour.hpp"

namespace qecmc {

template <int CODE>
struct ColourShortestSet {
    static const void *find(const KernelKey &k) { return k == colour_short_key(CODE) ? (const void *)ladder_colour_shortest_kernel<CODE> : nullptr; }
};

const void *colour_shortest_kernel(const KernelKey &k) { return find_kernel<ColourShortestSet<kCodeXzzx>, ColourShortestSet<kCodeRotated>>(k); }

}  // namespace qecmc
