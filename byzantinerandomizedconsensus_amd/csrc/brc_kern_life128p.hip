// brc_kern_life128p.hip -- the NPAD = 128 wide key-lifetime kernel in its pattern form (BRC_FLAG_LIFE_PATTERN;
// brc_life_wide.h PAT), one instantiation per protocol mode that has two key variants (REFERENCE, BEB).  A unit of
// its own: the other units compile what they did.
#include "brc_life_wide.h"

namespace brc {
int launch_life_128p(int mode, uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P) {
    return launch_life_wide_pat_npad<128>(mode, blocks, lds, s, P);
}
}  // namespace brc
