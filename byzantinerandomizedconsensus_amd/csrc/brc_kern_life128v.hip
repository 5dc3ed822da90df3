// brc_kern_life128v.hip -- the NPAD = 128 wide key-lifetime kernel with 3-bit value ids (BRC_FLAG_LIFE_VALUES;
// brc_life_wide.h V8): REFERENCE and BEB, each with and without the pattern form.  A unit of its own: the other units
// compile what they did.
#include "brc_life_wide.h"

namespace brc {
int launch_life_128v(int mode, bool pat, uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P) {
    return launch_life_wide_val_npad<128>(mode, pat, blocks, lds, s, P);
}
}  // namespace brc
