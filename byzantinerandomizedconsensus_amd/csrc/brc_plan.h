// brc_plan.h -- what brc_create decides before it touches the device: whether a brc_config can run, the engine
// geometry, the kernel family, and the size of every device buffer.  Pure arithmetic over the configuration, the
// BRC_KERNEL value and at most one number from the device (its total memory), so it needs no HIP header and a
// stand-alone host program can call it (tests/plan_dump.cpp).  brc_engine.hip executes the result.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>

#include "brc_layout.h"
#include "brc_plan_lv.h"

namespace brc {

struct PlanEnv {
    const char* kernel = nullptr;   // the BRC_KERNEL value, read once by the caller (null: unset)
    // the device's total memory; false: unknown (a failed query).  Asked at most once, and only for a lean engine
    // that is not lifetime-only already
    bool (*total_mem)(void* ctx, int device, uint64_t* bytes) = nullptr;
    void* ctx = nullptr;
};

struct Plan {
    int npad = 0, dm = 0, ipw = 0, nkw_t = 0;
    int kmode = 0;                               // the launchers' mode: BRC_MODE_* / KMODE_CONN / KMODE_XREF
    bool wide = false;                           // n > 64: one workgroup per instance (brc_step_wide.h)
    bool wide_wv4 = false;                       // wide: the 4-waves-per-SIMD instantiations (brc_step_wide.h WV)
    bool wide_rec = false;                       // wide: the record path (BRC_FLAG_WIDE_RECORDS / _VALUES; REC)
    bool wide_val = false;                       // wide: 3-bit value ids (BRC_FLAG_WIDE_VALUES; V8)
    bool regmask = false;                        // NPAD = 64 lean kernel with register delay masks (NLR = 2)
    bool compact = false;                        // lean kernels (NPAD = 64, sender peers): u32 cells (C32_*)
    bool general = false;                        // BRC_FLAG_GENERAL_KEYS at NPAD = 64 (KMODE_XREF)
    uint32_t lpi = 64;                           // replica lanes per item (64, or NPAD when wide)
    uint32_t bw = 1;                             // Byzantine-mask words per instance
    uint32_t NK = 0, nkw = 0, msize = 0, lds_bytes = 0;
    uint32_t rows = 0;                           // cell rows per item
    uint32_t rs = TS;                            // activity-ring rows: ring_steps(dm)
    uint32_t nval = 4;                           // consensus value ids the step kernel keeps (value_ids)
    uint64_t cons_bytes = 0;                     // consensus-set buffer (hmask) bytes per item
    uint64_t nitems = 0;
    bool life_cfg = false;                       // a fresh run to completion launches the key-lifetime kernel (brc_life.h)
    bool life_pl = false, life_pat = false;      // ... in its per-link delay form; the wide kernel's pattern form
    bool life_val = false;                       // ... the wide kernel's 3-bit value ids (BRC_FLAG_LIFE_VALUES; V8)
    uint32_t life_rw = LIFE_RW, life_lds = 0;    // ... its delivery-ring rows (LIFE_RW16 for delays above 8) and LDS bytes
    // false: the step kernel cannot serve this engine (its state would not fit, a lean key window above 32, or
    // BRC_FLAG_WIDE_LIFE): only the key-lifetime kernel runs, and the step kernel's key-slot arrays are not allocated
    bool step_ok = true;
    // Device buffers: which exist, and the bytes of each (8 for one the engine does not have: its pointer stays valid)
    bool cells_up_front = true;                  // brc_create allocates the step kernel's cells (else its first launch does)
    bool has_dbits = false, has_dring = false;   // lean SPEC delivery bitmaps; per-link lifetime kernel's bitmap ring
    bool has_lmeta = false;                      // two-class lifetime kernel, key windows >= 32 (life_hbm_meta)
    bool has_xsn = false;                        // a record table (xsend) with its per-item counts (xsn)
    uint64_t keys = 1, cells_n = 0;              // key-slot array entries (1: none); cells, of 4 (compact) or 8 bytes
    uint64_t step_state_bytes = 0;               // cells + key-slot arrays + activity ring (the lean engines' memory test)
    uint64_t cells_bytes = 0, meta_bytes = 0, mgen_bytes = 0, kdst_bytes = 0, act_bytes = 0, items_bytes = 0, inst_bytes = 0;
    uint64_t item_u32_bytes = 0, cons_rec_bytes = 0;   // actany, inj_off, inj_cnt each; cons0, cons1 each
    uint64_t istats_bytes = 0, hmask_bytes = 0, byz_bytes = 0;
    uint64_t dbits_bytes = 8, dring_bytes = 8, lmeta_bytes = 8, xsend_bytes = 8, xsn_bytes = 8;
};

inline int pick_npad(uint32_t n) { int p = 4; while ((uint32_t)p < n) p *= 2; return p; }
inline int pick_dm(uint32_t d) { return d <= 4 ? 4 : d <= 8 ? 8 : 16; }

// BRC_OK and *out, or BRC_E_INVALID and the reason in *why
inline int make_plan(const brc_config& c, const PlanEnv& env, Plan* out, std::string* why_out) {
    const char* why = nullptr;
    auto refuse = [&](const std::string& s) { *why_out = s; return (int)BRC_E_INVALID; };
    const bool force_step = env.kernel && strcmp(env.kernel, "step") == 0;
    const bool force_life = env.kernel && strcmp(env.kernel, "life") == 0;
    if (c.flags & BRC_FLAG_LIFE_PATTERN) {
        // the equivocation pattern on the wide key-lifetime kernel (brc_life_wide.h PAT): what the flag needs besides
        // BRC_FLAG_WIDE_LIFE's own conditions (below).  First, so that each of these gets its reason
        why =
            !(c.flags & BRC_FLAG_WIDE_LIFE) ? "BRC_FLAG_LIFE_PATTERN needs BRC_FLAG_WIDE_LIFE (flags): it selects the wide "
                                              "key-lifetime kernel's pattern form"
            : c.n <= 64 ? "BRC_FLAG_LIFE_PATTERN is for n > 64: at n <= 64 a byz_pattern runs on the step kernel"
            : c.peer_mode != BRC_PEER_SENDER ? "BRC_FLAG_LIFE_PATTERN needs sender peers (peer_mode)"
            : c.mode == BRC_MODE_SPEC ? "BRC_FLAG_LIFE_PATTERN: not with BRC_MODE_SPEC (mode), which has variants = 1 above 64 "
                                        "replicas and so cannot carry the pattern's two keys per origin"
            : c.byz_pattern != BRC_BYZ_EQUIVOCATE ? "BRC_FLAG_LIFE_PATTERN needs byz_pattern = BRC_BYZ_EQUIVOCATE: without a "
                                                    "pattern BRC_FLAG_WIDE_LIFE alone runs the same committee"
            : (c.variants != 2 && c.variants != 4) ? "BRC_FLAG_LIFE_PATTERN needs variants = 2 or 4: the pattern's keys are "
                                                     "variants 0 and 1 of a Byzantine origin"
                                                   : nullptr;
        if (why) return refuse(why);
    }
    // BRC_FLAG_LIFE_VALUES (brc_plan_lv.h): likewise
    if ((why = life_values_why(c)) != nullptr) return refuse(why);
    // every fault bound 0 .. n - 1 runs (the kernels compute n - f unsigned); f = n would leave no replica to count.
    // Named here, for a committee size in range; the range check below keeps its own f >= n
    if (c.n >= 1 && c.n <= 256 && c.f >= c.n)
        return refuse("the fault bound f = " + std::to_string(c.f) + " must be below n = " + std::to_string(c.n) +
                      " (f: 0 .. n - 1)");
    if (c.n < 1 || c.n > 256 || c.instances == 0 || c.delay_max < 1 || c.delay_max > 16 ||
        c.step_cap > STEP_LIMIT || c.peer_mode > BRC_PEER_CONNECTION ||
        (c.peer_mode == BRC_PEER_CONNECTION && c.mode != BRC_MODE_REFERENCE) ||
        (c.protocol != BRC_PROTO_BRB && c.protocol != BRC_PROTO_CONSENSUS) || c.delay_model > BRC_DELAY_GEOMETRIC ||
        (c.delay_model == BRC_DELAY_CONST && (c.delay_const < 1 || c.delay_const > c.delay_max)) ||
        !(c.key_window == 2 || c.key_window == 4 || c.key_window == 8 || c.key_window == 16 || c.key_window == 32 ||
          c.key_window == 64 || c.key_window == 128) ||
        !(c.variants == 1 || c.variants == 2 || c.variants == 4) ||
        // more than 8 live phase indices per origin: reference / best-effort protocols on the narrow kernels
        // (up to 128: the reference protocol's many-round runs; the lean kernels take <= 32 and
        // leave larger windows to the key-lifetime kernel, below)
        // ... and 16 or 32 on the wide kernels of an engine created with BRC_FLAG_WIDE_WINDOWS (validated below)
        c.key_window * c.variants > ((c.mode != BRC_MODE_SPEC && c.n <= 64) ? 128u
                                     : (c.flags & BRC_FLAG_WIDE_WINDOWS)    ? 32u : 8u) ||
        c.f >= c.n || (c.byz_pattern == BRC_BYZ_EQUIVOCATE && c.variants < 2) ||
        (c.byz_pattern != BRC_BYZ_NONE && c.byz_pattern != BRC_BYZ_EQUIVOCATE) ||
        c.proposals > BRC_PROPOSALS_LOADED || c.mode > BRC_MODE_BEB ||
        (c.flags & ~(uint32_t)(BRC_FLAG_GENERAL_KEYS | BRC_FLAG_WIDE_RECORDS | BRC_FLAG_WIDE_VALUES |
                               BRC_FLAG_WIDE_WINDOWS | BRC_FLAG_WIDE_LIFE | BRC_FLAG_LIFE_PATTERN |
                               BRC_FLAG_LIFE_VALUES)) ||
        // the general form at NPAD = 64 with sender peers is the reference protocol's (KMODE_XREF)
        ((c.flags & BRC_FLAG_GENERAL_KEYS) && c.n > 32 && c.n <= 64 && c.peer_mode == BRC_PEER_SENDER &&
         c.mode != BRC_MODE_REFERENCE) ||
        (c.n > 64 && c.mode == BRC_MODE_SPEC && c.variants != 1))
        return refuse("invalid configuration (see include/brc.h field ranges)");
    // (a backstop behind the two checks above: nothing below this line may ever see f >= n)
    if (c.f >= c.n)
        return refuse("the fault bound f = " + std::to_string(c.f) + " must be below n = " + std::to_string(c.n) +
                      " (f: 0 .. n - 1)");
    if ((c.flags & BRC_FLAG_WIDE_RECORDS) && (c.n <= 64 || c.peer_mode != BRC_PEER_SENDER))
        return refuse(c.n <= 64 ? "BRC_FLAG_WIDE_RECORDS is for the wide kernels (n > 64): the narrow kernels take restricted "
                                  "ECHO / READY records without a flag (n <= 32, or BRC_FLAG_GENERAL_KEYS at n in 33..64)"
                                : "BRC_FLAG_WIDE_RECORDS needs sender peers: with connection peers every message is a new "
                                  "peer, and the records count senders");
    if ((c.flags & BRC_FLAG_WIDE_VALUES) && (c.n <= 64 || c.peer_mode != BRC_PEER_SENDER || c.mode == BRC_MODE_SPEC))
        return refuse(c.n <= 64 ? "BRC_FLAG_WIDE_VALUES is for the wide kernels (n > 64): the narrow kernels keep 3-bit value "
                                  "ids without it (n <= 32, connection peers, or BRC_FLAG_GENERAL_KEYS at n in 33..64)"
                      : c.mode == BRC_MODE_SPEC ? "BRC_FLAG_WIDE_VALUES: not with BRC_MODE_SPEC, whose consensus is binary"
                                                : "BRC_FLAG_WIDE_VALUES needs sender peers: the connection-peer wide kernels "
                                                  "keep 2-bit value ids");
    if ((c.flags & BRC_FLAG_WIDE_WINDOWS) && (c.n <= 64 || c.peer_mode != BRC_PEER_SENDER || c.mode == BRC_MODE_SPEC))
        return refuse(c.n <= 64 ? "BRC_FLAG_WIDE_WINDOWS is for the wide kernels (n > 64): the narrow kernels take key windows "
                                  "up to 128 without it"
                      : c.mode == BRC_MODE_SPEC ? "BRC_FLAG_WIDE_WINDOWS: not with BRC_MODE_SPEC, whose per-phase windows stay <= 8"
                                                : "BRC_FLAG_WIDE_WINDOWS needs sender peers: the connection-peer wide kernels "
                                                  "(five words per cell) keep key_window * variants <= 8");
    if (c.flags & BRC_FLAG_WIDE_LIFE) {
        // the wide key-lifetime kernel (brc_life_wide.h): every field it cannot serve is named
        why =
            c.n <= 64 ? "BRC_FLAG_WIDE_LIFE is for n > 64: at n in 33..64 the key-lifetime kernel runs without a flag"
            : c.peer_mode != BRC_PEER_SENDER ? "BRC_FLAG_WIDE_LIFE needs sender peers (peer_mode): the wide key-lifetime kernel "
                                               "has no connection-peer form"
            : c.protocol != BRC_PROTO_CONSENSUS ? "BRC_FLAG_WIDE_LIFE needs the consensus protocol (protocol): the kernel takes no "
                                                  "injections, and a broadcast run is made of them"
            : c.proposals == BRC_PROPOSALS_NONE ? "BRC_FLAG_WIDE_LIFE needs Philox or loaded proposals (proposals)"
            : (c.delay_model != BRC_DELAY_CONST && c.delay_model != BRC_DELAY_SLOWSET)
                ? "BRC_FLAG_WIDE_LIFE needs constant or slow-set delays (delay_model): uniform / geometric delays have no "
                  "two-class form"
            : c.delay_max > 8 ? "BRC_FLAG_WIDE_LIFE needs delay_max <= 8 (a key's life must fit the 32-step ring)"
            : c.event_capacity != 0 ? "BRC_FLAG_WIDE_LIFE: no event log (event_capacity): the kernel visits no single message"
            : (c.byz_pattern != BRC_BYZ_NONE && !(c.flags & BRC_FLAG_LIFE_PATTERN))
                ? "BRC_FLAG_WIDE_LIFE: no byz_pattern (a pattern is made of injections); silent "
                  "Byzantine replicas go through byzantine_mask / brc_load_byzantine"
            : (c.flags & (BRC_FLAG_WIDE_RECORDS | BRC_FLAG_WIDE_VALUES))
                ? "BRC_FLAG_WIDE_LIFE: not with BRC_FLAG_WIDE_RECORDS / BRC_FLAG_WIDE_VALUES (flags), which select the step "
                  "kernel's record and 3-bit forms"
            : force_step ? "BRC_FLAG_WIDE_LIFE with BRC_KERNEL=step: a lifetime-only engine has no step state"
                         : nullptr;
        if (why) return refuse(why);
    }
    Plan p;
    p.npad = pick_npad(c.n);
    p.dm = pick_dm(c.delay_max);
    p.rs = ring_steps(p.dm);
    p.wide = p.npad > 64;
    p.ipw = p.wide ? 1 : 64 / p.npad;
    p.lpi = p.wide ? (uint32_t)p.npad : 64u;
    p.bw = p.wide ? (uint32_t)p.npad / 64 : 1u;
    p.nkw_t = p.npad / 8 < 1 ? 1 : p.npad / 8;
    // BRC_FLAG_WIDE_WINDOWS: up to 32 key slots per replica lane (NK <= 32 NPAD), as far as the LDS carve allows
    if (p.npad > 64 && (c.flags & BRC_FLAG_WIDE_WINDOWS)) p.nkw_t = p.npad / 2;
    p.NK = (uint32_t)p.npad * c.variants * c.key_window;
    // narrow kernel: + the trash row (brc_step.h); connection peers: 5 words per cell (the cell word
    // and two 16-step send-count rings, brc_step.h Ring16)
    const uint32_t cw = c.peer_mode == BRC_PEER_CONNECTION ? 5u : 1u;
    p.rows = p.wide ? p.NK * cw : (p.NK + 1) * cw;
    p.nkw = (p.NK + 63) / 64;
    p.msize = p.npad <= 8 ? 1 : (uint32_t)p.npad / 8;
    p.nitems = (c.instances + p.ipw - 1) / p.ipw;
    const bool spec = c.mode == BRC_MODE_SPEC;
    const uint32_t nL = delay_values(c.delay_model, c.delay_max);
    // BRC_FLAG_GENERAL_KEYS: NPAD = 64 with sender peers on the general form (KMODE_XREF), not the lean one
    p.general = (c.flags & BRC_FLAG_GENERAL_KEYS) && p.npad == 64 && c.peer_mode == BRC_PEER_SENDER;
    p.regmask = p.npad == 64 && c.peer_mode == BRC_PEER_SENDER && nL <= 2 && !p.general;
    p.compact = p.npad == 64 && c.peer_mode == BRC_PEER_SENDER && !p.general;   // = lean_kernel<64, mode> (brc_step.h)
    p.kmode = c.peer_mode == BRC_PEER_CONNECTION ? KMODE_CONN : p.general ? KMODE_XREF : (int)c.mode;
    // wide exchange words per (key, type): connection peers send 8 count planes per link delay
    const uint32_t xw = c.peer_mode == BRC_PEER_CONNECTION ? 8u * nL : xwords_wide(c.delay_model, c.delay_max, p.dm);
    p.lds_bytes = p.wide ? lds_bytes_wide(p.npad, p.NK, p.nkw, xw,
                                          spec, c.key_window, p.rs)
                         : lds_bytes_per_wave(p.npad, p.NK, p.nkw, p.regmask ? 0u : nL, spec, c.key_window,
                                              c.variants, p.rs, p.compact,
                                              typed_list(p.compact, c.event_capacity != 0, (int)c.mode)) * WPB;
    // wide kernel at 4 waves per SIMD (128 VGPRs): DM <= 8 without delay-code planes in registers (constant /
    // slow-set delays), sender peers, and LDS for four workgroups per CU
    // BRC_FLAG_WIDE_RECORDS: the instantiations with the record path (3 waves per SIMD, or 2 at DM = 16, only)
    // BRC_FLAG_WIDE_VALUES: 3-bit value ids (V8), instantiated in the record form only -- such an engine takes what
    // a BRC_FLAG_WIDE_RECORDS engine takes, and the two flags together select the same kernels
    p.wide_val = p.wide && (c.flags & BRC_FLAG_WIDE_VALUES);
    p.wide_rec = p.wide && (c.flags & (BRC_FLAG_WIDE_RECORDS | BRC_FLAG_WIDE_VALUES));
    p.wide_wv4 = p.wide && p.dm <= 8 && !plane_model(c.delay_model) && c.peer_mode == BRC_PEER_SENDER &&
                 p.lds_bytes <= 40u * 1024u && !p.wide_rec;
    p.nval = p.wide_val ? 8u : value_ids(!p.compact && !p.wide);
    p.cons_bytes = cons_bytes_per_item(spec, p.wide, p.lpi, p.msize, c.key_window, c.variants, p.nval);
    // the step kernel's state, as far as the configuration alone fixes it (step_ok, below, decides what is allocated)
    const uint64_t keys = (uint64_t)c.instances * p.NK;
    p.cells_n = (uint64_t)p.nitems * p.rows * p.lpi;
    p.cells_bytes = p.cells_n * (p.compact ? 4 : 8);
    const uint64_t act_bytes = (uint64_t)p.nitems * p.rs * p.nkw * act_types(p.compact, p.ipw) * 8;
    p.step_state_bytes = p.cells_bytes + keys * (8 + 4 + 8 * p.bw) + act_bytes;
    // key-lifetime kernel (brc_life.h): NPAD = 64 consensus under a two-class delay model with D <= 8
    // or per-link (uniform / geometric) delays with D <= 8, proposals from Philox or loaded, no event
    // log, no Byzantine pattern.  BRC_KERNEL=step | life | auto (default): auto runs it whenever the
    // configuration is eligible, except sender peers under per-link delays (the step kernel is faster
    // there): since round 6 its two-class form simulates a step's new keys one per lane, 1.8-7x faster than
    // the step kernel on cfg4.  A run it cannot take (injections, an event log, a stepped run)
    // falls back to the step kernel.
    // The lifetime kernel keeps no cells, so it also runs sender peers whose step-kernel cell store
    // would not fit in the free device memory (the reference protocol's many-round runs: its phase
    // leakage keeps ~1,000 keys of one instance live by round 8 at n = 64) and the key
    // windows above 32 the lean step kernel does not take.
    p.life_pl = c.delay_model == BRC_DELAY_UNIFORM || c.delay_model == BRC_DELAY_GEOMETRIC;
    p.life_lds = lds_bytes_life(p.NK, spec, c.key_window, c.variants, p.life_pl);
    p.life_rw = (p.life_pl && c.delay_max > 8) ? LIFE_RW16 : LIFE_RW;
    const bool eligible = p.npad == 64 && c.protocol == BRC_PROTO_CONSENSUS && !p.general &&
                          c.proposals != BRC_PROPOSALS_NONE && c.event_capacity == 0 && c.byz_pattern == BRC_BYZ_NONE &&
                          c.delay_max <= (p.life_pl ? 16u : 8u) && p.life_lds <= 160 * 1024 &&
                          // per-link form: its HBM delivery ring is [RW][NK] bits per instance
                          !(p.life_pl && c.key_window * c.variants > 32);
    bool big = p.compact && c.key_window * c.variants > 32;          // the lean kernels take <= 32
    // connection peers at NPAD = 64 with 8,192 key slots (Q * NV = 128): the step kernel's LDS carve
    // (186 KB) exceeds a workgroup's 160 KB, the lifetime kernel's (HBM slot metadata) does not
    const bool conn_big = !p.wide && c.peer_mode == BRC_PEER_CONNECTION && p.lds_bytes > 160 * 1024;
    if (conn_big && eligible) big = true;
    if (!big && p.compact && c.peer_mode == BRC_PEER_SENDER) {
        // the step kernel's whole per-instance state (cells, slot metadata / generations / destinations,
        // activity ring) against 90 % of the device's TOTAL memory: the choice depends on the
        // configuration and the device model only, never on what else holds memory at the time (an
        // engine whose state fits but cannot be allocated now fails brc_create with BRC_E_NOMEM)
        uint64_t tot = 0;
        if (env.total_mem && env.total_mem(env.ctx, c.device, &tot) && p.step_state_bytes > tot / 10 * 9) big = true;
    }
    const bool prefer_life = c.peer_mode == BRC_PEER_CONNECTION || !p.life_pl;
    p.life_cfg = eligible && !force_step && (force_life || prefer_life || big);
    p.step_ok = !big;
    if (big && !p.life_cfg)
        return refuse(c.key_window * c.variants > 32
            ? "key windows above 32 at n in 33..64 with sender peers (128 with connection peers) run on the "
              "key-lifetime kernel only "
              "(consensus, Philox / loaded proposals, delay_max <= 8, constant or slow-set delays, no event log)"
            : "the step kernel's cells do not fit in free device memory and the key-lifetime kernel cannot run "
              "this configuration");
    if (c.flags & BRC_FLAG_WIDE_LIFE) {
        // lifetime-only, as the "big" engines above: no cells, key-slot arrays or activity ring
        p.life_pl = false;
        p.life_rw = LIFE_RW;
        p.life_pat = (c.flags & BRC_FLAG_LIFE_PATTERN) != 0;
        p.life_val = (c.flags & BRC_FLAG_LIFE_VALUES) != 0;
        p.life_lds = lds_bytes_life_wide(p.npad, p.NK, p.nkw, spec, c.key_window, p.life_pat, p.life_val);
        p.life_cfg = true;
        p.step_ok = false;
        p.cons_bytes = 0;                               // the host masks / phase counters live in LDS for the whole run
        if (p.life_val) {
            // 3-bit value ids: host-mask planes 4..7 live in HBM, in the wide step kernel's eight-plane layout (planes
            // 0..3 of the buffer are allocated and unused: one index formula for both kernels); wide_val / wide_rec
            // stay false, they select step-kernel launchers
            p.nval = 8;
            p.cons_bytes = cons_bytes_per_item(false, true, p.lpi, p.msize, c.key_window, c.variants, p.nval);
        }
        if (p.life_lds > 160 * 1024)
            return refuse("BRC_FLAG_WIDE_LIFE: key_window * variants = " + std::to_string(c.key_window * c.variants) +
                          " exceeds the wide key-lifetime kernel's LDS (lds " + std::to_string(p.life_lds) + " B of 163840)");
    }
    if ((p.step_ok && ((p.wide && p.nkw > (uint32_t)p.nkw_t) ||
                       p.lds_bytes > 160 * 1024)) || p.nitems > 0x7FFFFFFFull * WPB)
        return refuse("configuration exceeds the kernel's LDS / key-slot limits (lds " + std::to_string(p.lds_bytes) + " B)");
    // the device buffers
    p.cells_up_front = !p.life_cfg;
    p.keys = p.step_ok ? keys : 1;                       // the step kernel's key-slot arrays
    p.meta_bytes = p.keys * 8;
    p.mgen_bytes = p.keys * 4;
    p.kdst_bytes = p.keys * 8 * p.bw;
    p.act_bytes = p.step_ok ? act_bytes : 8;
    p.item_u32_bytes = p.nitems * 4;
    p.items_bytes = p.nitems * sizeof(ItemState);
    p.inst_bytes = c.instances * sizeof(InstState);
    p.istats_bytes = c.instances * 32;
    p.cons_rec_bytes = p.nitems * p.lpi * 8;
    p.hmask_bytes = p.nitems * p.cons_bytes;
    p.byz_bytes = c.instances * p.bw * 8;
    p.has_dbits = p.compact && spec && p.step_ok;
    if (p.has_dbits) p.dbits_bytes = p.nitems * p.nkw * 64 * 8;
    p.has_dring = p.life_cfg && p.life_pl;                // (the lifetime kernel leaves its bitmap ring zero at exit)
    if (p.has_dring) p.dring_bytes = p.nitems * p.life_rw * p.nkw * 64 * 8;
    p.has_lmeta = p.life_cfg && life_hbm_meta(c.key_window, p.life_pl);
    if (p.has_lmeta) p.lmeta_bytes = p.nitems * p.NK * 8;
    // extra-SEND and restricted ECHO / READY records: the non-lean narrow kernels (the lean and wide kernels refuse
    // them), and the wide kernels of an engine created with BRC_FLAG_WIDE_RECORDS / BRC_FLAG_WIDE_VALUES
    p.has_xsn = p.wide_rec || !(p.compact || p.wide);
    if (p.has_xsn) {
        p.xsend_bytes = p.nitems * XSEND_MAX * (p.wide_rec ? WREC_W * 8 : 24);
        p.xsn_bytes = p.nitems * 4;
    }
    *out = p;
    return BRC_OK;
}

// Why an engine that runs on the key-lifetime kernel only (step_ok == false) refuses injections (run == false) or
// a run its kernel cannot take (run == true)
inline const char* life_only_why(const Plan& p, bool run) {
    if (p.wide)
        return run ? "this engine runs on the wide key-lifetime kernel only (BRC_FLAG_WIDE_LIFE): a fresh run to completion, "
                     "no injections, max_steps = 0 (brc_reset first)"
                   : "this engine runs on the wide key-lifetime kernel only (BRC_FLAG_WIDE_LIFE): no injections";
    return run ? "this engine runs on the key-lifetime kernel only (its step-kernel state does not fit, or a key "
                 "window above 32 at n in 33..64 with sender peers, of 128 with connection peers): a fresh run to "
                 "completion, no injections, "
                 "max_steps = 0, value ids < 4 (brc_reset first)"
               : "this engine runs on the key-lifetime kernel only (its step-kernel state does not fit the device, "
                 "or a key window above 32 at n in 33..64 with sender peers, of 128 with connection peers): no injections";
}

}  // namespace brc
