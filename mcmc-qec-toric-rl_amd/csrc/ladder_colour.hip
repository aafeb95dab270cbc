// scan = 2 (ladder_colour.hpp): the instantiations of ladder_colour_kernel.
#include "ladder_colour.hpp"

namespace qecmc {

template <int CODE, int RULE>
struct ColourSet {   // ladder_colour_kernel<CODE, CONV, RULE> for CONV = false, true
    static const void *find(const KernelKey &k)
    {
        if (!(k == colour_key(CODE, k.conv, RULE))) return nullptr;
        return k.conv ? (const void *)ladder_colour_kernel<CODE, true, RULE> : (const void *)ladder_colour_kernel<CODE, false, RULE>;
    }
};

const void *colour_kernel(const KernelKey &k)
{
    return find_kernel<ColourSet<kCodeToric, 0>, ColourSet<kCodeXzzx, 0>, ColourSet<kCodeRotated, 0>, ColourSet<kCodePlanar, 0>,
                       ColourSet<kCodeXzzx, 1>, ColourSet<kCodeRotated, 1>, ColourSet<kCodeXzzx, 2>, ColourSet<kCodeRotated, 2>>(k);
}

}  // namespace qecmc
