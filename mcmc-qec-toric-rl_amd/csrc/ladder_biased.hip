// The biased (src/mcmc_biased.py) and alpha (src/mcmc_alpha.py) acceptance rules on the xzzx / rotated codes (choose_ladder_biased, kernel_choice.hpp).
#include "ladder_kernel.hpp"

namespace qecmc {

const void *ladder_biased_kernel(const KernelKey &k)
{
    constexpr uint32_t B = kBiased | kGentop, Q = kConv | kQueue;
    return find_kernel<LadderSet<1024, 4, kX | kR, B, B | kConv, B | kAlpha, B | kAlpha | kConv, B | Q, B | kAlpha | Q>,
                       LadderSet<512, 4, kX | kR, B | Q, B | kAlpha | Q>,
                       LadderSet<512, 8, kX | kR, B, B | kConv, B | kAlpha, B | kAlpha | kConv, B | kSsw, B | kAlpha | kSsw>>(k);
}

}  // namespace qecmc
