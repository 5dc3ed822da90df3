// brc_life_cell.h -- the body of the key-lifetime kernels' BRB cell handler, upd_cell (brc_life.h; brc_life_wide.h):
// one source for both kernels, included inside the lambda
//     auto upd_cell = [&](uint32_t& fl, uint32_t& ec, uint32_t& rc, bool opn, uint32_t sa, uint32_t ea, uint32_t ra,
//                         bool hS, bool hE, bool hR, uint32_t& es, uint32_t& rs, uint32_t& dl, uint32_t& nr) { ... };
// whose scope provides the constants CONN, BEB, SPEC (the kernel's mode) and the thresholds T_echo, T_amp, T_del.
// No include guard: it is a function body, not a set of declarations.
        auto ge = [](uint32_t x, uint32_t y) -> uint32_t { return ((x - y) >> 31) ^ 1u; };   // x >= y (< 2^31)
        if constexpr (CONN) {
            // core/brbroadcast.py:60-119 with connection-identity peers (brc_step.h brb_cell_update_conn):
            // sets count messages; the :119 amplification re-fires, nr READY copies this step.  In
            // integer form (0/1 words, VALU): the bool form's per-lane conditions became SGPR lane
            // masks combined with scalar ANDs, and this kernel is SALU-bound.
            const uint32_t o = opn ? 1u : 0u, om = 0u - o;
            es = o & sa & ~fl & 1u;                                   // :76-82 (F_EEX = bit 0)
            fl |= es | (es << 3);
            const uint32_t e = ea & om, eon = min(e, 1u);             // :84-98
            const uint32_t chk = min(e + (fl & 1u) - eon, 1u);
            fl |= eon;
            ec += e;
            const uint32_t r1 = eon & chk & ge(ec, T_echo) & (~fl >> 1) & 1u;
            fl |= r1 << 1;
            const uint32_t x = ra & om, ron = min(x, 1u);             // :100-119
            const uint32_t rexm = 0u - ((fl >> 1) & 1u);
            const uint32_t rlo = 2u + ((rc - 1u) & rexm), rhi = x + (rc & rexm);
            fl |= ron << 1;
            rc += x;
            const uint32_t any = ron & ge(rhi, rlo);
            const uint32_t alo = max(rlo, T_amp), ahi = min(rhi, T_del - 1u);
            const uint32_t fire = any & ~fl & ge(ahi, alo) & 1u;      // :118 (no F_RS test: re-fires)
            nr = r1 + ((ahi - alo + 1u) & (0u - fire));
            dl = any & ge(rhi, T_del);                                // :111-115
            fl |= dl << 2;
            rs = min(nr, 1u);
            fl |= rs << 4;
            return;
        }
        if constexpr (BEB) {
            dl = (opn && sa) ? 1u : 0u;                             // brb_cell_update_beb
            fl |= dl << 2;
        } else if constexpr (SPEC) {
            if (hS) { es = (opn ? sa : 0u) & ~(fl >> 3) & 1u; fl |= es << 3; }   // brb_cell_update_spec
            if (hE || hR) {
                ec += opn ? ea : 0u;
                rc += opn ? ra : 0u;
                rs = (opn ? 1u : 0u) & ~(fl >> 4) & (ge(ec, T_echo) | ge(rc, T_amp));
                fl |= rs << 4;
                dl = (opn ? 1u : 0u) & ge(rc, T_del);
                fl |= dl << 2;
            }
        } else {
            // brb_cell_update in integer form (brc_step.h process_pair).  F_EEX = bit 0, F_REX = 1,
            // F_DEL = 2, F_ES = 3, F_RS = 4.
            if (hS) {                                                // :76-82
                es = (opn ? sa : 0u) & ~fl & 1u;
                fl |= es | (es << 3);
            }
            if (hE) {                                                // :84-98
                const uint32_t e = opn ? ea : 0u;
                const uint32_t eon = min(e, 1u);
                const uint32_t chk = min(e + (fl & 1u) - eon, 1u);
                fl |= eon;
                ec += e;
                const uint32_t r1 = eon & chk & ge(ec, T_echo) & (~fl >> 1) & 1u;
                fl |= (r1 << 1) | (r1 << 4);
                rs = r1;
            }
            if (hR) {                                                // :100-119
                const uint32_t x = opn ? ra : 0u;
                const uint32_t ron = min(x, 1u);
                const uint32_t rexm = 0u - ((fl >> 1) & 1u);
                const uint32_t rlo = 2u + ((rc - 1u) & rexm), rhi = x + (rc & rexm);
                fl |= ron << 1;
                rc += x;
                const uint32_t any = ron & ge(rhi, rlo);
                const uint32_t alo = max(rlo, T_amp), ahi = min(rhi, T_del - 1u);
                const uint32_t r2 = any & ~fl & ~(fl >> 4) & ge(ahi, alo) & 1u;
                fl |= r2 << 4;
                dl = any & ge(rhi, T_del);
                fl |= dl << 2;
                rs |= r2;
            }
        }
        nr = rs;
