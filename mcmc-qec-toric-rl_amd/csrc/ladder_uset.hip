// USET instantiations: the ladder kernel with the unique-chain set insertion of PTDC / STDC / PTRC / STRC compiled in (choose_ladder_uset); and
// scan = 1: the systematic generator sweep (depolarizing rule, every code; choose_ladder_sweep, kernel_choice.hpp).  Two dispatch functions, one unit.
#include "ladder_kernel.hpp"

namespace qecmc {

const void *ladder_uset_kernel(const KernelKey &k)
{
    return find_kernel<LadderSet<1024, 4, kX | kR, kUset | kBiased | kAlpha | kGentop>,      // STDC_droplet_alpha: single Chain_alpha chains
                       LadderSet<1024, 4, kT | kX | kR | kP, kUset, kUset | kGsplit>,
                       LadderSet<512, 8, kT | kX | kR | kP, kUset, kUset | kGsplit>>(k);
}

const void *ladder_sweep_kernel(const KernelKey &k)
{
    return find_kernel<LadderSet<1024, 4, kT, kScan, kScan | kConv, kScan | kGentop, kScan | kGentop | kConv>,
                       LadderSet<512, 8, kT, kScan, kScan | kConv, kScan | kGentop, kScan | kGentop | kConv>,
                       LadderSet<1024, 4, kX | kR | kP, kScan | kGentop, kScan | kGentop | kConv>,
                       LadderSet<512, 8, kX | kR | kP, kScan | kGentop, kScan | kGentop | kConv>>(k);
}

}  // namespace qecmc
