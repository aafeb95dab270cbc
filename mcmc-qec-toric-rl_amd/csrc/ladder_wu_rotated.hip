// scan = 3 (ladder_wu.hpp): the rotated instantiations.
#include "ladder_wu.hpp"

namespace qecmc {

const void *wave_rotated_kernel(const KernelKey &k) { return find_kernel<WaveWords<512, kCodeRotated>, WaveWords<1024, kCodeRotated>, WaveSet<512, 6, kCodeRotated, 32, false>>(k); }

}  // namespace qecmc
