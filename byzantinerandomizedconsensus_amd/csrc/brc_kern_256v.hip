// brc_kern_256v.hip -- the NPAD = 256 wide step kernel with 3-bit consensus value ids (BRC_FLAG_WIDE_VALUES;
// brc_step_wide.h V8, always the record form).  A unit of its own: brc_kern_256.hip / brc_kern_256x.hip compile
// what they did.
#include "brc_step_wide.h"

namespace brc {
int launch_step_256v(int dm, bool events, int mode, uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P) {
    return launch_step_wide_v8<256>(dm, events, mode, blocks, lds, s, P);
}
}  // namespace brc
