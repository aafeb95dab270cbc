// Toric code, depolarizing rule, the reference's random scan: the headline kernel family (choose_ladder_toric, kernel_choice.hpp).
#include "ladder_kernel.hpp"

namespace qecmc {

const void *ladder_toric_kernel(const KernelKey &k)
{
    return find_kernel<
        // 4 waves per SIMD by their LDS footprint: 128 VGPRs, the top chain's blocks drawn ahead
        LadderSet<512, 4, kT, kPre, kPre | kConv, kPre | kGsplit, kPre | kGsplit | kConv, kPre | kDelut, kPre | kDelut | kConv>,
        LadderSet<1024, 4, kT, 0u, kConv, kGsplit, kGsplit | kConv,                                                  // plain
                  kGentop, kGentop | kConv,                                                                           // general top chain
                  kDelut, kDelut | kConv, kDelut | kGsplit, kDelut | kGsplit | kConv,                                 // dE table
                  kQueue | kConv, kQueue | kConv | kGsplit>,                                                          // work queue
        LadderSet<512, 8, kT, 0u, kConv, kGsplit, kGsplit | kConv,
                  kGentop, kGentop | kConv, kGentop | kGsplit, kGentop | kGsplit | kConv,
                  kDelut, kDelut | kConv, kDelut | kGsplit, kDelut | kGsplit | kConv,
                  kSsw | kGsplit, kSsw | kGsplit | kDelut,                                                            // swap sweep by wave 0
                  kQueue | kConv, kQueue | kConv | kGsplit, kQueue | kConv | kGsplit | kDelut>>(k);
}

}  // namespace qecmc
