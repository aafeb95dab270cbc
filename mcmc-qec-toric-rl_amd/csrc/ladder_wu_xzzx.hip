// scan = 3 (ladder_wu.hpp): the xzzx instantiations.
#include "ladder_wu.hpp"

namespace qecmc {

const void *wave_xzzx_kernel(const KernelKey &k) { return find_kernel<WaveWords<512, kCodeXzzx>, WaveWords<1024, kCodeXzzx>, WaveSet<512, 6, kCodeXzzx, 32, false>>(k); }

}  // namespace qecmc
