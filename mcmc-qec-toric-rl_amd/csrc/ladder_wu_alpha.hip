// scan = 3 under the alpha noise model (src/mcmc_alpha.py): the xzzx / rotated instantiations of 4 and 8 state words.  The kernel: ladder_wu.hpp.
#include "ladder_wu.hpp"

namespace qecmc {

template <int MAXT, int CODE>   // fixed-length kernels at 8 waves per SIMD, criterion kernels at 6
using WaveAlpha = KernelList<WaveSet<MAXT, 8, CODE, 4, false, true>, WaveSet<MAXT, 8, CODE, 8, false, true>, WaveSet<MAXT, 6, CODE, 4, true, true>,
                             WaveSet<MAXT, 6, CODE, 8, true, true>>;

const void *wave_alpha_kernel(const KernelKey &k)
{
    return find_kernel<WaveAlpha<512, kCodeXzzx>, WaveAlpha<1024, kCodeXzzx>, WaveAlpha<512, kCodeRotated>, WaveAlpha<1024, kCodeRotated>>(k);
}

}  // namespace qecmc
