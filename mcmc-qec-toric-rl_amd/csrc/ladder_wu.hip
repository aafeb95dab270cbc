// scan = 3 (wave-uniform generator picks, states in registers): the toric instantiations (+ 32 words: fixed-length runs of up to 8 rungs).
#include "ladder_wu.hpp"

namespace qecmc {

const void *wave_toric_kernel(const KernelKey &k)
{
    return find_kernel<WaveWords<512, kCodeToric>, WaveWords<1024, kCodeToric>, WaveSet<512, 6, kCodeToric, 32, false>>(k);
}

}  // namespace qecmc
