// brc_plan_lv.h -- the planner's part for BRC_FLAG_LIFE_VALUES (3-bit value ids on the wide key-lifetime kernel,
// brc_life_wide.h V8): what the flag needs besides BRC_FLAG_WIDE_LIFE's own conditions, each with a reason that names
// it.  HIP-free, as brc_plan.h, which includes it.
#pragma once
#include "brc_layout.h"

namespace brc {

// null: the flag is not set, or the configuration may carry it (BRC_FLAG_WIDE_LIFE's checks follow in make_plan:
// with BRC_FLAG_WIDE_RECORDS / BRC_FLAG_WIDE_VALUES it stays refused there)
inline const char* life_values_why(const brc_config& c) {
    if (!(c.flags & BRC_FLAG_LIFE_VALUES)) return nullptr;
    return !(c.flags & BRC_FLAG_WIDE_LIFE) ? "BRC_FLAG_LIFE_VALUES needs BRC_FLAG_WIDE_LIFE (flags): it selects the wide "
                                             "key-lifetime kernel's 3-bit value ids"
           : c.n <= 64 ? "BRC_FLAG_LIFE_VALUES is for n > 64: at n <= 64 the key-lifetime kernel keeps 2-bit value ids"
           : c.peer_mode != BRC_PEER_SENDER ? "BRC_FLAG_LIFE_VALUES needs sender peers (peer_mode)"
           : c.mode == BRC_MODE_SPEC ? "BRC_FLAG_LIFE_VALUES: not with BRC_MODE_SPEC (mode), whose consensus is binary"
                                     : nullptr;
}

}  // namespace brc
