// brc_kern_life256.hip -- the NPAD = 256 wide key-lifetime kernel (BRC_FLAG_WIDE_LIFE; brc_life_wide.h), one
// instantiation per protocol mode.  A unit of its own: the other units compile what they did.
#include "brc_life_wide.h"

namespace brc {
int launch_life_256(int mode, uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P) {
    return launch_life_wide_npad<256>(mode, blocks, lds, s, P);
}
}  // namespace brc
