// brc_internal.h -- types shared by the engine's host code (brc_engine.hip) and the step-kernel
// translation units (brc_kern_<NPAD>.hip).  Not part of the public ABI (include/brc.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "brc_layout.h"   // the HIP-free constants and size formulas (shared with brc_plan.h)

namespace brc {

constexpr uint32_t NEVER = 0xFFFFu;
constexpr uint64_t TIMES_NEVER = 0xFFFFFFFF00000000ull;
constexpr uint32_t F_EEX = 1, F_REX = 2, F_DEL = 4, F_ES = 8, F_RS = 16;
constexpr uint32_t GEN_RESTRICTED = 0x80000000u;
constexpr uint32_t GEN16_RESTRICTED = 0x8000u;  // the narrow kernel's 16-bit LDS copy of mgen
constexpr uint32_t GEN16_XDONE = 0x4000u;       // ... key processed by this step's extra-SEND pre-pass (brc_step.h)
__host__ __device__ inline uint16_t gen16(uint32_t g) {
    return (uint16_t)((g & GEN_MASK) | ((g & GEN_RESTRICTED) ? GEN16_RESTRICTED : 0u));
}
__host__ __device__ inline uint32_t gen32(uint16_t g) {
    return (g & GEN_MASK) | ((g & GEN16_RESTRICTED) ? GEN_RESTRICTED : 0u);
}
// The consensus pass's deferred-SEND queue (brc_step.h, brc_life.h send_key): the SENDs one replica starts in
// one step's pass -- one per phase end, consecutive phase indices -- at most SENDQ_MAX of them, else
// BRC_OVERFLOW.  One bound for every kernel, so the step and key-lifetime kernels overflow at the same
// point; the queue keeps 2-bit value ids in one 64-bit word, 3-bit ones one per nibble of two.  Measured with the oracle: at
// most 17 phase ends of
// one replica in one step (cfg4, n = 64, round cap 64: bench.py's long leg, whose 2^20-instance GPU test sees
// no overflow), 12 on the reference-pinned round-cap-64 fixture (tests/test_oracle_golden.py pins it); with
// every link at delay 1 up to 27 (tests/test_gpu_life.py ref-const64-cap30-q32).
constexpr uint32_t SENDQ_MAX = 32;
template <uint32_t VB> struct SendQ {      // the queued SENDs' VB-bit value ids (VB = 3: entry i in nibble i % 16 of word i / 16)
    uint64_t w[VB == 2 ? 1 : 2];
    __device__ __forceinline__ void clear() { for (auto& x : w) x = 0; }
    __device__ __forceinline__ void put(uint32_t i, uint32_t v) {
        if constexpr (VB == 2) { w[0] |= (uint64_t)(v & 3u) << (2 * i); return; }
        const uint64_t x = (uint64_t)(v & 15u) << (4 * (i & 15u));
        if (i < 16) w[0] |= x; else w[VB == 2 ? 0 : 1] |= x;
    }
    __device__ __forceinline__ uint32_t get(uint32_t i) const {
        if constexpr (VB == 2) return (uint32_t)(w[0] >> (2 * i)) & 3u;
        return (uint32_t)((i < 16 ? w[0] : w[VB == 2 ? 0 : 1]) >> (4 * (i & 15u))) & 15u;
    }
};

// Compact cell of the lean kernels (NPAD = 64, sender peers: brc_step.h), one u32:
//   bits 0-4 flags F_EEX, F_REX, F_DEL, F_ES, F_RS
//   bits 5-10 |echo set|, 11-16 |ready set| (both saturate at 63)
//   bits 17-23 / 24-30: step this lane SENT its ECHO / READY, as an offset from the item's epoch;
//   C32_OLD = sent more than DM steps before the epoch, C32_NEVER = not sent
// No generation tag: a slot's row is rewritten fresh whenever the slot is (re)allocated.
constexpr uint32_t C32_EC_SH = 5, C32_RC_SH = 11, C32_OE_SH = 17, C32_OR_SH = 24;
constexpr uint32_t C32_NEVER = 127, C32_OLD = 126;
constexpr uint32_t C32_FRESH = (C32_NEVER << C32_OE_SH) | (C32_NEVER << C32_OR_SH);
constexpr uint32_t C32_REBASE = 100;   // a step more than this past the epoch moves the epoch first
constexpr uint32_t C32_KEEP = 17;      // ... to t - C32_KEEP: sends in the last 16 steps keep their step


struct Params {
    uint32_t n, f, D, Q, NV, NK, nkw;
    uint32_t protocol, delay_model, dconst, round_cap, step_cap, proposals;
    uint32_t T_echo, T_amp, T_del, T_cnt, bound_p1, bound_p2;
    uint64_t seed, inst_offset, instances, nitems;
    uint32_t max_steps, nL;   // nL: delay_values() of the run
    uint32_t mode;            // BRC_MODE_*
    uint32_t s_limit;         // phase indices >= s_limit overflow: the slot generation tags must not wrap
    uint64_t coin_seed;
    uint64_t event_cap;
    uint64_t* cells;
    uint64_t* meta; uint32_t* mgen; uint64_t* kdst;
    uint64_t* act; uint32_t* actany; ItemState* items; InstState* inst; uint64_t* istats;
    uint64_t* cons0; uint64_t* cons1; void* hmask;
    const InjDev* inj; const uint32_t* inj_off; const uint32_t* inj_cnt;
    const uint64_t* byz; const int8_t* prop;
    brc_event* events; unsigned long long* event_count;
    uint64_t* dbits;              // lean SPEC: per-wave delivery bitmaps [item][nkw][64] (brc_step.h DBG)
    uint64_t* dring;              // per-link key-lifetime kernel: delivery bitmap ring [item][LIFE_RW or LIFE_RW16][nkw][64] (brc_life.h)
    uint32_t* lmeta;              // key-lifetime kernel, key windows >= 32: key-slot metadata + class delivery steps
                                  // [item][2][NK] u32 in HBM (brc_life.h)
    uint64_t* xsend;              // non-lean step kernels: extra-SEND records [item][XSEND_MAX][3] (brc_step.h);
                                  // wide kernels with records: [instance][XSEND_MAX][WREC_W] (brc_step_wide.h)
    uint32_t* xsn;                // ... records in use per item
    unsigned long long* gcount;   // [0] cell_steps [1] arrivals [2] msgs [3] deliveries [4] lane loads [5] max s
                                  // [6] instances still running after the launch
};

// Consensus record word 0 (cons0): round [0,16) | phase [16,20) | nvals [20,24) | order [24,48) (the
// value ids in insertion order, 2 or 3 bits each) | value_count [48,64)
__host__ __device__ inline uint64_t cons0_pack(uint32_t round, uint32_t phase, uint32_t nvals, uint32_t order,
                                               uint32_t vcount) {
    return (uint64_t)(round & 0xFFFF) | ((uint64_t)(phase & 0xF) << 16) | ((uint64_t)(nvals & 0xF) << 20) |
           ((uint64_t)(order & 0xFFFFFF) << 24) | ((uint64_t)(vcount & 0xFFFF) << 48);
}

// Launch the key-lifetime kernel (brc_kern_life.hip): one 64-lane workgroup per instance
// (perlink: uniform / geometric delays, delivery bitmaps in P.dring; dm16: delays up to 16, whose
// keys live up to 64 steps: P.dring has LIFE_RW16 rows)
// qbig: key windows of 64 / 128 (two-class form, not SPEC)
// hm: the slot metadata in HBM (life_hbm_meta)
int launch_life(int mode, bool perlink, bool dm16, bool qbig, bool hm, uint32_t blocks, uint32_t lds, hipStream_t s,
                const Params* P);

// Wide key-lifetime kernel (brc_life_wide.h, BRC_FLAG_WIDE_LIFE; LDS carve: lds_bytes_life_wide, brc_layout.h):
// its launchers, one translation unit per NPAD (brc_kern_life128.hip / brc_kern_life256.hip); mode: BRC_MODE_*
int launch_life_128(int mode, uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P);
int launch_life_256(int mode, uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P);
// ... and of the pattern form (brc_kern_life128p.hip / brc_kern_life256p.hip); mode: BRC_MODE_REFERENCE / BRC_MODE_BEB
int launch_life_128p(int mode, uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P);
int launch_life_256p(int mode, uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P);
// ... and of the 3-bit value-id form (brc_kern_life128v.hip / brc_kern_life256v.hip; BRC_FLAG_LIFE_VALUES); mode:
// BRC_MODE_REFERENCE / BRC_MODE_BEB, pat: the pattern form
int launch_life_128v(int mode, bool pat, uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P);
int launch_life_256v(int mode, bool pat, uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P);

// Step-kernel launchers, one translation unit per replica-set width NPAD (brc_kern_<NPAD>.hip).
// Return 0 on success, BRC_E_INVALID when no instantiation matches (dm), BRC_E_HIP on a launch error.
int launch_step_4(int dm, bool events, int mode, uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P);
int launch_step_8(int dm, bool events, int mode, uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P);
int launch_step_16(int dm, bool events, int mode, uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P);
int launch_step_32(int dm, bool events, int mode, uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P);
int launch_step_64(int dm, bool events, int mode, uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P);
// NPAD = 64 lean kernels with the (at most two) link-delay masks in registers (brc_kern_64r.hip)
int launch_step_64r(int dm, bool events, int mode, uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P);
// wide kernel (brc_step_wide.h): one workgroup of NPAD threads per instance
// wv4: the 4-waves-per-SIMD instantiation (wide_waves4: DM <= 8, no link-delay planes, sender peers)
int launch_step_128(int dm, bool events, int mode, bool wv4, uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P);
int launch_step_256(int dm, bool events, int mode, bool wv4, uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P);
// ... with restricted ECHO / READY records (BRC_FLAG_WIDE_RECORDS; brc_kern_128x.hip / brc_kern_256x.hip)
int launch_step_128x(int dm, bool events, int mode, uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P);
int launch_step_256x(int dm, bool events, int mode, uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P);
// ... with 3-bit consensus value ids as well (BRC_FLAG_WIDE_VALUES; brc_kern_128v.hip / brc_kern_256v.hip)
int launch_step_128v(int dm, bool events, int mode, uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P);
int launch_step_256v(int dm, bool events, int mode, uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P);

}  // namespace brc
