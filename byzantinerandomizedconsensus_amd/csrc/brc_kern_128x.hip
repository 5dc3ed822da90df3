// brc_kern_128x.hip -- the NPAD = 128 wide step kernel with restricted ECHO / READY records
// (BRC_FLAG_WIDE_RECORDS; brc_step_wide.h REC).  A unit of its own: brc_kern_128.hip compiles what it did.
#include "brc_step_wide.h"

namespace brc {
int launch_step_128x(int dm, bool events, int mode, uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P) {
    return launch_step_wide_rec<128>(dm, events, mode, blocks, lds, s, P);
}
}  // namespace brc
