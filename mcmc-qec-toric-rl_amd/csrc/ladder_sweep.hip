// scan = 1: the systematic generator sweep (depolarizing rule, every code; choose_ladder_sweep, kernel_choice.hpp).
#include "ladder_kernel.hpp"

namespace qecmc {

const void *ladder_sweep_kernel(const KernelKey &k)
{
    return find_kernel<LadderSet<1024, 4, kT, kScan, kScan | kConv, kScan | kGentop, kScan | kGentop | kConv>,
                       LadderSet<512, 8, kT, kScan, kScan | kConv, kScan | kGentop, kScan | kGentop | kConv>,
                       LadderSet<1024, 4, kX | kR | kP, kScan | kGentop, kScan | kGentop | kConv>,
                       LadderSet<512, 8, kX | kR | kP, kScan | kGentop, kScan | kGentop | kConv>>(k);
}

}  // namespace qecmc
