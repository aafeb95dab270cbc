// XZZX, rotated and planar codes, depolarizing rule, random scan (choose_ladder_surf, kernel_choice.hpp).
#include "ladder_kernel.hpp"

namespace qecmc {

const void *ladder_surf_kernel(const KernelKey &k)
{
    constexpr unsigned XRP = kX | kR | kP;
    return find_kernel<LadderSet<512, 4, XRP, kGentop | kPre, kGentop | kPre | kConv, kGentop | kPre | kDelut, kGentop | kPre | kDelut | kConv>,
                       LadderSet<1024, 4, XRP, kGentop, kGentop | kConv, kGentop | kDelut, kGentop | kDelut | kConv, kGentop | kQueue | kConv>,
                       LadderSet<512, 8, XRP, kGentop, kGentop | kConv, kGentop | kDelut, kGentop | kDelut | kConv, kGentop | kSsw, kGentop | kSsw | kDelut,
                                 kGentop | kQueue | kConv>>(k);
}

}  // namespace qecmc
