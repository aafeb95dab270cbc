// scan = 3 (ladder_wu.hpp): the planar instantiations (no 32-word kernels).
#include "ladder_wu.hpp"

namespace qecmc {

const void *wave_planar_kernel(const KernelKey &k) { return find_kernel<WaveWords<512, kCodePlanar>, WaveWords<1024, kCodePlanar>>(k); }

}  // namespace qecmc
