// brc_layout.h -- the HIP-free part of brc_internal.h: the constants and size formulas that the host's planner
// (brc_plan.h), the engine (brc_engine.hip) and the kernels share.  Includes only <stdint.h> and the public ABI, so a
// plain C++ compiler can read it; under hipcc every function is __host__ __device__ as before.
#pragma once
#include <stdint.h>

#include "../../include/brc.h"

#ifdef __HIPCC__
#define BRC_HD __host__ __device__
#else
#define BRC_HD
#endif

namespace brc {

constexpr int TS = 32;            // activity ring (steps) at the largest DM; > max delay (ring_steps(dm) per kernel)
#ifndef BRC_WPB
#define BRC_WPB 1
#endif
constexpr int WPB = BRC_WPB;      // independent waves per workgroup (narrow kernel); 1 measured best:
                                  // LDS-bound SPEC runs pack more waves per CU (exp/ab.sh, r1)
// activity-ring rows of the narrow kernel: a power of two above the largest delay (D <= DM)
BRC_HD constexpr uint32_t ring_steps(int dm) { return dm <= 8 ? 16u : 32u; }
constexpr uint32_t STEP_LIMIT = 60000;
#ifndef BRC_CHUNK_W
#define BRC_CHUNK_W 4
#endif
constexpr int CHUNK_W = BRC_CHUNK_W;                // wide kernel: keys whose ballots are exchanged per barrier
#ifndef BRC_WIDE_DCW
#define BRC_WIDE_DCW 2     // 128 key-list positions per pass: keeps cfg5 at <= 40 KB (4 workgroups per CU)
#endif
// wide kernel: delivery-bitmap words per receiver = key-list positions per pass / 64
BRC_HD inline uint32_t dpos_words_wide(uint32_t nkw) { return nkw < BRC_WIDE_DCW ? nkw : BRC_WIDE_DCW; }
constexpr int KMODE_CONN = 3;               // kernel mode: reference protocol, connection-identity peers
constexpr int KMODE_XREF = 4;               // ... reference protocol, sender peers, NPAD = 64 in the general
                                            // (non-lean) form: BRC_FLAG_GENERAL_KEYS
#ifndef BRC_CHUNK
#define BRC_CHUNK 4
#endif
constexpr int CHUNK = BRC_CHUNK;            // narrow kernel: key slots whose cell loads are in flight together
#ifndef BRC_LCHUNK
#define BRC_LCHUNK 8
#endif
constexpr int LCHUNK = BRC_LCHUNK;          // ... on the lean kernels (4 or 8; A/B round 4: 8 is 0.9 % faster)
constexpr int KPAD = CHUNK > LCHUNK ? CHUNK : LCHUNK;   // key-list padding entries: 2 KPAD
#ifndef BRC_TYPED
#define BRC_TYPED 1          // lean kernels without an event log (not BEB): the step's key list sorted by the message
#endif                       // types landing on a key, one straight-line pair body per class (0: one mixed list)
#ifndef BRC_TYPED_ER
#define BRC_TYPED_ER 1       // ... with a class of its own for keys receiving ECHO and READY in one step (0: general body)
#endif
// the kernels with the type-sorted list (brc_step.h TYPED); mode: a BRC_MODE_* / KMODE_* value of a lean kernel
BRC_HD constexpr bool typed_list(bool lean, bool events, int mode) {
    return BRC_TYPED && lean && !events && mode != BRC_MODE_BEB;
}
// ... their key-list entries beyond NK + 2 KPAD: each of the list's segments (brc_step.h TCLS <= 5 classes) is padded
// to a whole chunk, fewer than KPAD entries each
constexpr uint32_t KL_TYPED_PAD = 5 * (KPAD - 1) + 1;
#ifndef BRC_KL32_SPEC
#define BRC_KL32_SPEC 0     // lean SPEC with u32 key-list entries too (1 KB more LDS per wave at Q = 8)
#endif

// epoch: the lean kernels' send-step base (compact cells, brc_internal.h C32_*); 0 elsewhere
struct ItemState { uint32_t t, inj_pos, initialized, epoch; };

struct InstState { uint16_t status, t_stop, q_until, flags; uint32_t pad0, pad1; };

// Distinct link delays a delay model can produce (bounds the compact delay-mask table in LDS).
BRC_HD inline uint32_t delay_values(uint32_t model, uint32_t dmax) {
    return model == BRC_DELAY_CONST ? 1u : model == BRC_DELAY_SLOWSET ? (dmax > 1 ? 2u : 1u) : dmax;
}

// Extra-SEND records per item (a payload SENT by several origins; brc_step.h): live at once.  The table is
// shared with the restricted ECHO / READY records of Byzantine replicas (one bound for both kinds).
constexpr uint32_t XSEND_MAX = 16;
// Wide kernels under BRC_FLAG_WIDE_RECORDS (brc_step_wide.h REC): the same table per instance holds restricted
// ECHO / READY records and extra SENDs (type 0: a SEND of a key SENT before), WREC_W words each -- the first word as
// on the narrow kernels (XS_TYPE_SH below) with the one sender at WREC_NODE_SH (no segment: one instance per
// workgroup), then the destination set's four words (words past NPAD / 64 are zero)
constexpr uint32_t WREC_W = 5;

// Slot generation tags of the non-lean narrow step kernels (brc_internal.h gen16 / gen32): 13 bits; the host forces a
// full clear before they can wrap (brc_inject.h InjectBook)
constexpr uint32_t GEN_MASK = 0x1FFF;
constexpr uint32_t GEN_FULL_CLEAR = 6000;

struct InjDev {       // 48 B, per item CSR, sorted by t
    uint32_t t;
    uint16_t slot, s;
    uint8_t kind, type, seg, node;
    int8_t value;
    uint8_t restricted;   // SEND to a strict subset of the peers (set by the host for n > 64); MSG: bit 0 = an
                          // ECHO / READY on the links node -> dst only (a record of the item's table lands it),
                          // bit 1 = the first link (node, type, key) ever used: a SEND event (brc_step.h)
    uint8_t pad[2];
    uint64_t dst;         // destinations 0..63 (the narrow kernel reads the first 24 B only)
    uint64_t dst_hi[3];   // destinations 64..255 (wide kernel)
};

// an extra-SEND record's first word (XSEND_MAX): key slot | step << 16 | instance segment << 40 |
// message type << XS_TYPE_SH (0: an extra SEND; BRC_ECHO / BRC_READY: a restricted message)
constexpr uint32_t XS_TYPE_SH = 48;
// ... on the wide kernels under BRC_FLAG_WIDE_RECORDS (WREC_W): the one sender
constexpr uint32_t WREC_NODE_SH = 56;

// Consensus value ids (core/byzantinerandomizedconsensus.py:57-60 keys its tables by payload string;
// id 0 is str(NONE) == "-1"): 2 bits (3 strings + "-1") on the lean, wide and key-lifetime kernels,
// 3 bits (7 strings + "-1") on the other narrow kernels (NPAD <= 32, and connection peers) and on the wide
// kernels of an engine created with BRC_FLAG_WIDE_VALUES (brc_step_wide.h V8: the planner sets nval itself) and on the
// wide key-lifetime kernel of one created with BRC_FLAG_LIFE_VALUES (brc_life_wide.h V8).
BRC_HD constexpr uint32_t value_ids(bool narrow_full) { return narrow_full ? 8u : 4u; }

// u64 words of a wave's consensus LDS area: REFERENCE hm[nval][64] T; SPEC [seen[Q][64] T +] cnt[Q][64] u32
BRC_HD inline uint32_t cons_words(bool spec, uint32_t msize, uint32_t Q, uint32_t nv, uint32_t nval = 4) {
    // SPEC with one key variant per origin: a replica delivers each (origin, phase) key at most
    // once, so the origin count needs no host set (seen masks only when nv > 1)
    return spec ? (Q * 64 * (nv > 1 ? msize : 0u) + Q * 64 * 4 + 7) / 8 : (nval * 64 * msize + 7) / 8;
}

// Activity-ring words per (row, key word): the lean kernels keep one ECHO and one READY row (typed
// marks: a key step evaluates only the message types that can land; SEND arrivals are found from the
// key metadata), the others one untyped row for the wave item.  BRC_PSEG=1 (experimental) gives the
// non-lean kernels one row and key list per instance of the item (IPW = 64 / NPAD of them), so a key
// step loads only the instances with arrivals on it: measured SLOWER on cfg2 / cfg3 / cfg3-spec /
// cfg2-spec (per-lane key ids turn the key dispatch into vector work; round-5 A/B), so off by default.
#ifndef BRC_PSEG
#define BRC_PSEG 0
#endif
BRC_HD constexpr uint32_t act_types(bool lean, uint32_t ipw = 1) { return lean ? 2u : BRC_PSEG ? ipw : 1u; }

// Injection records the non-lean narrow kernels stage in LDS at a time (one memory round trip per
// INJ_CACHE records instead of one per record: cfg3's equivocation pattern is 120 records per wave)
constexpr uint32_t INJ_CACHE = 16;

// Bytes of dynamic LDS one wave of the step kernel needs (must match the kernel's carve):
// meta[IPW*NK] u64 | act[RS][act_types][nkw] u64 | dbits[nkw][64] u64 (not on lean SPEC) | consensus area | L[nL][64] T |
// mgen[IPW*NK] u16 (not on the lean kernels) | klist[NK + 2 KPAD] u16 (tail padded with the trash row NK;
// u32 entries on the lean REFERENCE / BEB kernels; BRC_PSEG: one list per instance on the others) |
// injc[INJ_CACHE][3] u64 (not on the lean kernels)
BRC_HD inline uint32_t lds_bytes_per_wave(int npad, uint32_t NK, uint32_t nkw, uint32_t nL, bool spec,
                                          uint32_t Q, uint32_t nv, uint32_t rs, bool lean, bool typed) {
    const uint32_t ipw = 64 / (uint32_t)npad;
    const uint32_t msize = npad <= 8 ? 1 : (uint32_t)npad / 8;
    const uint32_t h_words = cons_words(spec, msize, Q, nv, value_ids(!lean));
    const uint32_t l_words = (nL * 64 * msize + 7) / 8;
    // (lean REFERENCE / BEB kernels: u32 entries, brc_step.h KL_*)
    // (typed: + KL_TYPED_PAD entries, the chunk padding of the type-sorted list's segments, typed_list())
    const uint32_t klist_u16 = (NK + 2 * KPAD + (typed ? KL_TYPED_PAD : 0u)) *
                               ((lean && (!spec || BRC_KL32_SPEC)) ? 2u : lean ? 1u : act_types(false, ipw));
    const uint32_t gen_words = lean ? 0u : (ipw * NK + 3) / 4;   // lean kernels keep no slot generations
    const uint32_t dbits_words = (lean && spec) ? 0u : 64 * nkw;   // lean SPEC keeps them in HBM
    const uint32_t injc_words = lean ? 0u : 3 * INJ_CACHE;
    return 8 * (ipw * NK + rs * nkw * act_types(lean, ipw) + dbits_words + h_words + l_words + gen_words + (klist_u16 + 3) / 4 +
                injc_words);
}

// Bytes of dynamic LDS one workgroup of the wide kernel needs (brc_step_wide.h carve):
// meta[NK] u64 | act[rs][nkw] u64 (rs = ring_steps(dm)) | dpos[DCW][NPAD] u64 | consensus area |
// xb[2][CHUNK_W][nL][2][NW] u64 | outm[16][NW] u64 | sq[Q][NPAD] u8 | fresh[nkw] u64 | klist[NK] u16 |
// red[12] u32 | pmw[2][CHUNK_W][NW] u32
// consensus area: REFERENCE hm[4][NW][NPAD] u64;  SPEC cnt[Q][NPAD] u32 (one key variant per origin)
// (3-bit value ids, BRC_FLAG_WIDE_VALUES: the same carve -- host-mask planes 4..7 stay in the HBM buffer)
BRC_HD inline uint32_t cons_words_wide(bool spec, uint32_t npad, uint32_t Q) {
    const uint32_t nw = npad / 64;
    return spec ? (Q * npad + 1) / 2 : 4 * nw * npad;
}
// Wide kernel: link-delay code bit planes per DM (delay - 1 in NPL bits), and the u64 words one
// wave publishes per (key, message type) in the ballot exchange: one per link delay present
// (constant, slow-set), or -- uniform / geometric delays -- the NPL bit planes of "steps since
// this lane sent, minus one" plus the mask of lanes whose send lies inside the 2^NPL window.
BRC_HD constexpr int npl_of(int dm) { return dm == 4 ? 2 : dm == 8 ? 3 : 4; }
BRC_HD inline bool plane_model(uint32_t model) {
    return model == BRC_DELAY_UNIFORM || model == BRC_DELAY_GEOMETRIC;
}
BRC_HD inline uint32_t xwords_wide(uint32_t model, uint32_t dmax, int dm) {
    return plane_model(model) ? (uint32_t)npl_of(dm) + 1u : delay_values(model, dmax);
}

BRC_HD inline uint32_t lds_bytes_wide(int npad, uint32_t NK, uint32_t nkw, uint32_t nL, bool spec, uint32_t Q,
                                      uint32_t rs) {
    const uint32_t nw = (uint32_t)npad / 64;
    return 8 * (NK + rs * nkw + dpos_words_wide(nkw) * (uint32_t)npad + cons_words_wide(spec, (uint32_t)npad, Q) +
                2 * CHUNK_W * nL * 2 * nw + 16 * nw) +
           Q * (uint32_t)npad + 8 * nkw + 2 * NK + 4 * (12 + 2 * CHUNK_W * nw);
}

// Bytes of the global consensus-set buffer (hmask) per item: REFERENCE host masks [4][lanes] of
// n bits; SPEC phase windows seen[Q][lanes] (n bits; narrow kernel only) + cnt[Q][lanes] u32.
inline uint64_t cons_bytes_per_item(bool spec, bool wide, uint32_t lanes, uint32_t msize, uint32_t Q, uint32_t nv,
                                    uint32_t nval = 4) {
    return spec ? (uint64_t)Q * lanes * ((wide || nv == 1 ? 0 : msize) + 4) : (uint64_t)nval * lanes * msize;
}

// Key-lifetime kernel (brc_life.h): ring steps (> 4 Dd - 1 for Dd <= 8) and LDS bytes of one wave
// (must match the kernel's carve):
//   meta[NK] u32 | two-class form: dA[NK], dB[NK] u8 (each receiver class's delivery step of the key,
//   0x80 | step mod 128) | (8-B aligned) consensus area (cons_words at NPAD = 64)
constexpr uint32_t LIFE_RW = 32;
// Key windows >= 32 in the two-class form (life_hbm_meta): the slot metadata lives in HBM (P.lmeta) and
// LDS keeps only the class delivery steps plus a 128-word snapshot of the metadata of the key words a
// consensus pass reads (their own instantiations, brc_life<..., HMT>).
#ifndef BRC_LIFE_HM_Q
#define BRC_LIFE_HM_Q 32
#endif
BRC_HD inline bool life_hbm_meta(uint32_t Q, bool perlink) { return !perlink && Q >= BRC_LIFE_HM_Q; }
// Their class delivery steps live in HBM too (one u32 per slot beside the metadata: 8 B per slot in
// P.lmeta); LDS keeps, per ring step, the key words with a delivery then (LIFE_RW rows x 128 bits) and the
// consumed words' class bitmaps (16 B per key word).
BRC_HD inline uint32_t lds_bytes_life(uint32_t NK, bool spec, uint32_t Q, uint32_t nv, bool perlink) {
    if (life_hbm_meta(Q, perlink))
        return 4u * 128u + 16u * 32u + 16u * ((NK + 63) / 64) + 8 * cons_words(spec, 8, Q, nv);
    return ((4u * NK + (perlink ? 0u : 2 * NK) + 7) & ~7u) + 8 * cons_words(spec, 8, Q, nv);
}
// the per-link form's delivery-ring rows at delays up to 16, whose keys live up to 64 steps (LIFE_RW below that)
constexpr uint32_t LIFE_RW16 = 64;

// Wide key-lifetime kernel (brc_life_wide.h, BRC_FLAG_WIDE_LIFE: n > 64, two-class delays, sender peers): bytes of
// dynamic LDS one workgroup needs (must match the kernel's carve):
//   kab[nkw][2] u64 (a step's class bitmaps per key word) | consensus area (cons_words_wide: REFERENCE / BEB host
//   masks hm[4][NW][NPAD] u64, SPEC cnt[Q][NPAD] u32) | meta[NK] u32 | rg[4][LIFE_RW] u32 (the step-statistics
//   rings) | ctl[16] u32 (rows, class sizes, reduction slots) | dA[NK], dB[NK] u8 (class delivery steps) |
//   sq[Q][NPAD] u8 (deferred SENDs)
// pat (the pattern form, BRC_FLAG_LIFE_PATTERN): four class bitmaps per key word instead of two (+ 16 nkw), and
//   pbyz[4] u64 (the Byzantine mask) | pcnt[8] u32 (class sizes per parity) | oA[2 NPAD], oB[2 NPAD] u8 (the
//   out-classes' delivery steps of the pattern keys)
// v8 (3-bit value ids, BRC_FLAG_LIFE_VALUES): val[NK] u8 (the slots' value ids) at the end; host-mask planes 4..7
//   stay in the HBM buffer, as on the wide step kernel
BRC_HD inline uint32_t lds_bytes_life_wide(int npad, uint32_t NK, uint32_t nkw, bool spec, uint32_t Q,
                                           bool pat = false, bool v8 = false) {
    return 16 * nkw + 8 * cons_words_wide(spec, (uint32_t)npad, Q) + 4 * NK + 4 * (4 * LIFE_RW + 16) + 2 * NK +
           Q * (uint32_t)npad + (pat ? 16 * nkw + 64 + 4 * (uint32_t)npad : 0u) + (v8 ? NK : 0u);
}

}  // namespace brc
