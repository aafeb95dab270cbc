// USET instantiations: the ladder kernel with the unique-chain set insertion of PTDC / STDC / PTRC / STRC compiled in (choose_ladder_uset).
#include "ladder_kernel.hpp"

namespace qecmc {

const void *ladder_uset_kernel(const KernelKey &k)
{
    return find_kernel<LadderSet<1024, 4, kX | kR, kUset | kBiased | kAlpha | kGentop>,      // STDC_droplet_alpha: single Chain_alpha chains
                       LadderSet<1024, 4, kT | kX | kR | kP, kUset, kUset | kGsplit>,
                       LadderSet<512, 8, kT | kX | kR | kP, kUset, kUset | kGsplit>>(k);
}

}  // namespace qecmc
