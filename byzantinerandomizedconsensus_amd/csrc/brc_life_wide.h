// brc_life_wide.h -- the key-lifetime kernel for large committees: n in (64, 256], two-class delays, sender peers
// (BRC_FLAG_WIDE_LIFE).
//
// brc_life.h's two-class form does not depend on n: under the constant and slow-set delay models a key's whole life
// is two receiver-class states (honest fast receivers, honest slow ones), advanced in closed form from the class
// sizes nHF / nHS and the thresholds.  The wide step kernel (brc_step_wide.h) moves NPAD cells per key-step through
// HBM (NK * NPAD * 8 B of cells per instance); this kernel keeps no cells: a key is simulated once, by the lane of
// its origin, when it is created, and leaves (a) per class the step at which the class delivers it and (b) per-step
// statistics, both in LDS.
//
// Layout: one workgroup of NPAD threads (NW = NPAD / 64 waves) per instance, thread d = replica d = origin d, as in
// brc_step_wide.h.  What was a wave operation at n <= 64 becomes:
//   * lifetime simulation: each wave simulates the new keys of its own 64 origins (simulate_batch's per-lane code,
//     one key per lane per batch), with no barrier inside -- a batch touches its own slots, and the shared step
//     statistics only through no-return LDS atomics; nHF / nHS come from one block reduction per launch;
//   * step statistics: the ring rows rg[4][RW] (arrivals, messages, cells, deliveries) and the `rows` word live in
//     LDS; a wave adds whole-word partial sums whose terms are class sizes times ballot popcounts (brc_life.h
//     BRC_LIFE_BSTAT's arithmetic: a packed 16-bit pair would overflow, a lane's arrival count reaches 2 n + 1);
//   * class delivery steps: bytes s_dA / s_dB[NK] as in brc_life.h; a step's consensus pass first builds the two
//     class bitmaps of every key word into s_kab[nkw][2] (waves take key words round-robin, ballots over keys
//     w * 64 + lane, consumed bytes cleared there) and every replica reads its class's bitmap after a barrier;
//   * control flow around every barrier is block-uniform: the next step comes from the LDS `rows` word read after a
//     barrier, status / overflow / "an honest replica is undecided" from a block reduction (rotating LDS slots, one
//     barrier each).  A wave with nothing to simulate or deliver still reaches each barrier.
//
// Scope (brc_create): sender peers, consensus protocol, BRC_MODE_REFERENCE / SPEC (one key variant) / BEB, Philox or
// loaded proposals, constant or slow-set delays up to 8, 2-bit value ids (3-bit: V8, below), silent Byzantine replicas, no event log, no
// injections, a fresh engine run to completion.  Overflow (an origin's window full, more than min(Q, SENDQ_MAX)
// SENDs of one replica in one step), step-cap stops and t_stop behave as in brc_life.h.  Results are identical to the
// wide step kernel's (tests/test_gpu_wide_life.py checks both against the C oracle).
//
// PAT (BRC_FLAG_LIFE_PATTERN): the even / odd equivocation pattern (BRC_BYZ_EQUIVOCATE; brc_engine.hip
// expand_equivocate) as a function of the instance's Byzantine mask, with no injection.  Byzantine replica b declares
// the keys (b NV + v, s = 0) with value id 1 + v (v = 0, 1), SENDs key v at t = 0 to the replicas of parity v, and
// ECHOes and READYs both keys to everyone at t = 1.  Such a key's life is four receiver-class states -- (fast | slow)
// x (got the SEND: "in" | did not: "out") -- plus the origin's own ECHO and READY, one arrival each at
// 1 + delay(b -> class).  At t = 0 every Byzantine lane (idle otherwise) simulates its two keys with
// simulate_pattern, the four-class form of simulate_batch; honest keys keep the two-class form.  A replica's class
// for a pattern key depends on its parity, so the PAT form keeps four class bitmaps per key word (fast even, slow
// even, fast odd, slow odd) and the out-classes' delivery steps in a side table oA / oB[2 NPAD] (entry 2 b + v: only
// phase slot 0 of variants 0 / 1 of a Byzantine origin is ever a pattern key).  Step 1 is entered although nothing
// may arrive then: it is the step of the pattern's second action, as in the oracle.  The PAT = false instantiations
// compile to what they did.
//
// V8 (BRC_FLAG_LIFE_VALUES): 3-bit consensus value ids (seven proposal strings besides "-1"), as brc_step_wide.h's V8.
// A slot's metadata word has no spare bit (tend 16, s + 1 14, a 2-bit id), so the 3-bit id of a slot lives in a byte
// plane of its own, val[NK] u8 in LDS, written where the metadata is claimed and read where the consensus pass read
// the 2-bit field.  `order` packs 3-bit fields (eight of them fill cons0_pack's 24 bits).  Host-mask planes 0..3
// stay in LDS; planes 4..7 live in the HBM buffer P.hmask, [instance][8][NW][NPAD] u64 (the step kernel's V8 layout;
// planes 0..3 of it are unused here), every lane its own column, touched only by a delivery that carries such an id.
// The host zeroes the buffer before every run (clear_state).  REFERENCE and BEB only: SPEC consensus is binary.
// The V8 = false instantiations compile to what they did.
#pragma once
#include "brc_life.h"

#ifndef BRC_LIFE_WIDE_WAVES
#define BRC_LIFE_WIDE_WAVES 4   // waves per SIMD the register allocation must allow (128 VGPRs)
#endif

namespace brc {

template <int NPAD, int MODE, bool PAT = false, bool V8 = false>
__global__ __launch_bounds__(NPAD, BRC_LIFE_WIDE_WAVES) void brc_life_wide(const Params* __restrict__ pp) {
    const Params& P = *pp;
    constexpr bool SPEC = MODE == BRC_MODE_SPEC, BEB = MODE == BRC_MODE_BEB, CONN = false;   // (brc_life_cell.h reads all three)
    static_assert(NPAD == 128 || NPAD == 256, "wide committees: two or four waves");
    static_assert(MODE == BRC_MODE_REFERENCE || MODE == BRC_MODE_SPEC || MODE == BRC_MODE_BEB, "sender peers");
    static_assert(!PAT || MODE != BRC_MODE_SPEC, "the pattern needs two key variants: SPEC above 64 replicas has one");
    static_assert(!V8 || MODE != BRC_MODE_SPEC, "3-bit value ids: reference / best-effort (SPEC consensus is binary)");
    // consensus value ids: VB bits each, NVAL of them; VREP has a 1 in the low bit of every VB-bit field of `order`
    constexpr uint32_t NVAL = V8 ? 8u : 4u, VB = V8 ? 3u : 2u, VMASK = NVAL - 1u, VREP = V8 ? 0x249249u : 0x55u;
    constexpr uint32_t KC = PAT ? 4u : 2u;           // class bitmaps per key word
    constexpr uint32_t NW = NPAD / 64;
    constexpr uint32_t RW = LIFE_RW;                 // ring rows (> the longest key lifetime, 4 Dd <= 32)
    extern __shared__ __attribute__((aligned(16))) uint64_t smem[];

    const uint32_t tid = threadIdx.x, wid = tid / 64, lane = tid % 64;
    const uint64_t inst = blockIdx.x;
    if (inst >= P.instances) return;                 // whole workgroup exits
    const uint32_t n = P.n, NK = P.NK, Q = P.Q, NV = P.NV, nkw = P.nkw;
    const uint32_t T_echo = P.T_echo, T_amp = P.T_amp, T_del = P.T_del;
    const uint32_t qsh = (uint32_t)__ffs(Q) - 1u, Qm = Q - 1u, ksh = qsh + (uint32_t)__ffs(NV) - 1u;

    // ---- LDS carve (lds_bytes_life_wide): kab[nkw][2] u64 | consensus area (REFERENCE / BEB hm[4][NW][NPAD] u64,
    // SPEC cnt[Q][NPAD] u32) | meta[NK] u32 | rg[4][RW] u32 | ctl[16] u32 | dA[NK], dB[NK] u8 | sq[Q][NPAD] u8
    // PAT: kab[nkw][4], and after sq: pbyz[4] u64 | pcnt[8] u32 | oA[2 NPAD], oB[2 NPAD] u8
    // V8: val[NK] u8 (the slots' 3-bit value ids) at the end
    uint64_t* const s_kab = smem;                    // the step's consumed class bitmaps per key word: class A, class B
    uint64_t* const s_hm = s_kab + KC * nkw;
    uint32_t* const s_cnt = (uint32_t*)s_hm;
    uint32_t* const s_meta = (uint32_t*)(s_hm + cons_words_wide(SPEC, NPAD, Q));
    uint32_t* const s_rg = s_meta + NK;              // arrivals [RW] | messages [RW] | cells [RW] | deliveries [RW]
    // ctl: [0] rows (ring rows holding arrivals at honest receivers) [1] nHF [2] nHS [4..15] reduction slots
    uint32_t* const s_ctl = s_rg + 4 * RW;
    uint32_t* const s_red = s_ctl + 4;
    uint8_t* const s_dA = (uint8_t*)(s_ctl + 16);    // class delivery steps (brc_life.h: 0x80 | step mod 128, 0: none)
    uint8_t* const s_dB = s_dA + NK;
    uint8_t* const s_sq = s_dB + NK;                 // deferred SENDs: values (phase indices consecutive)
    uint64_t* const s_pbyz = (uint64_t*)(s_sq + Q * NPAD);   // PAT: the instance's Byzantine mask words
    // PAT: [0..3] honest fast even / fast odd / slow even / slow odd replicas [4] Byzantine replicas
    uint32_t* const s_pcnt = (uint32_t*)(s_pbyz + 4);
    uint8_t* const s_oA = (uint8_t*)(s_pcnt + 8);    // PAT: out-class delivery steps of pattern key 2 b + v (as dA / dB)
    uint8_t* const s_oB = s_oA + 2 * NPAD;
    uint8_t* const s_val = PAT ? s_oB + 2 * NPAD : s_sq + Q * NPAD;   // V8: value id of slot k (set with s_meta[k])

    const uint32_t d = tid;
    const uint64_t g = P.inst_offset + inst;
    const uint64_t byzw = gp(P.byz)[inst * NW + wid];
    const bool real = d < n;
    const bool honest = real && !((byzw >> lane) & 1ull);

    // ---- two delay classes: delay(j -> d) = 1 if j and d are both fast, Dd otherwise (schedule.h slow set)
    uint32_t Dd = P.delay_model == BRC_DELAY_CONST ? P.dconst : P.D;
    bool laneF = false;                              // this replica is fast (no fast class: constant delays, D = 1)
    if (P.delay_model == BRC_DELAY_SLOWSET && P.D > 1) {
        const uint32_t off = slow_offset(P.seed, g, n);
        laneF = real && !(((d + n - off) % n) < P.f);
    } else if (P.delay_model == BRC_DELAY_SLOWSET) {
        Dd = 1;                                      // D = 1: every link has delay 1
    }
    Dd = uni32(Dd);

    // ---- LDS init
    for (uint32_t i = d; i < NK; i += NPAD) { s_meta[i] = 0u; s_dA[i] = 0; s_dB[i] = 0; }
    for (uint32_t i = d; i < KC * nkw; i += NPAD) s_kab[i] = 0ull;
    for (uint32_t i = d; i < 4 * RW + 16; i += NPAD) s_rg[i] = 0u;     // the rings and ctl
    if constexpr (SPEC) {
        for (uint32_t q = 0; q < Q; ++q) s_cnt[q * NPAD + d] = 0u;
    } else {
        for (uint32_t v = 0; v < 4 * NW; ++v) s_hm[v * NPAD + d] = 0ull;
    }
    if constexpr (PAT) {
        ((uint32_t*)s_oA)[d] = 0u;                   // oA and oB: 4 NPAD bytes
        if (d < 8) s_pcnt[d] = 0u;
        if (lane == 0) s_pbyz[wid] = byzw;
    }
    __syncthreads();
    {
        // class sizes over the whole committee: one block reduction per launch
        const uint32_t cF = (uint32_t)__popcll(__ballot(honest && laneF)), cS = (uint32_t)__popcll(__ballot(honest && !laneF));
        if (lane == 0) {
            if (cF) atomicAdd(&s_ctl[1], cF);
            if (cS) atomicAdd(&s_ctl[2], cS);
        }
        if constexpr (PAT) {
            // ... and per parity (64 is even: lane parity = replica parity), with the Byzantine replicas' count
            const uint64_t bF = __ballot(honest && laneF), bS = __ballot(honest && !laneF), ev = 0x5555555555555555ull;
            const uint32_t c4[5] = {(uint32_t)__popcll(bF & ev), (uint32_t)__popcll(bF & ~ev), (uint32_t)__popcll(bS & ev),
                                    (uint32_t)__popcll(bS & ~ev), (uint32_t)__popcll(__ballot(real && !honest))};
            if (lane == 0) {
#pragma unroll
                for (int q = 0; q < 5; ++q) if (c4[q]) atomicAdd(&s_pcnt[q], c4[q]);
            }
        }
    }
    __syncthreads();
    const uint32_t nHF = uni32(s_ctl[1]), nHS = uni32(s_ctl[2]);
    uint32_t nFe = 0, nFo = 0, nSe = 0, nSo = 0;
    bool any_byz = false;                            // block-uniform
    if constexpr (PAT) {
        nFe = uni32(s_pcnt[0]); nFo = uni32(s_pcnt[1]); nSe = uni32(s_pcnt[2]); nSo = uni32(s_pcnt[3]);
        any_byz = uni32(s_pcnt[4]) != 0;
    }

    // ---- block reduction: OR of x over the workgroup (rotating LDS slots, one barrier; brc_step_wide.h block_red)
    uint32_t rctr = 0;
    auto block_or = [&](uint32_t x) -> uint32_t {
        uint32_t* const cur = s_red + 4 * (rctr % 3);
        uint32_t* const nxt = s_red + 4 * ((rctr + 1) % 3);
        ++rctr;
        const uint32_t wx = wave_or(x);
        if (lane == 0 && wx) atomicOr(&cur[0], wx);
        if (tid == 0) nxt[0] = 0;
        __syncthreads();
        return uni32(cur[0]);
    };

    uint32_t status = BRC_RUNNING, t_stop = 0, t = 0;
    bool ovf = false;
    // per-thread statistics (summed at write-back): thread 0 commits the ring rows, every thread its own SENDs
    uint64_t st_msgs = 0, st_arr = 0, st_cells = 0, st_del = 0, st_ksteps = 0;
    uint32_t st_smax = 0;

    // ---- consensus state (core/byzantinerandomizedconsensus.py:25-29)
    const bool cons_lane = honest;                   // consensus protocol (host-checked)
    uint32_t round = 0, phase = 0, nvals = 0, order = 0, vcount = 0;
    uint32_t dcount = 0, frnd = 0, ft = 0, fval = 0, lval = 0;
    uint32_t clr = 0;                                // this replica's keys created this step: bit s mod Q (Q <= 32)
    auto hm = [&](uint32_t v, uint32_t w) -> uint64_t& { return s_hm[(v * NW + w) * NPAD + d]; };
    auto cnt = [&](uint32_t q) -> uint32_t& { return s_cnt[q * NPAD + d]; };
    // V8: this lane's word w of plane v (4..7) in the HBM buffer (brc_step_wide.h ghm)
    auto ghm = [&](uint32_t v, uint32_t w) -> gptr_t<uint64_t> {
        return gp((uint64_t*)P.hmask) + ((inst * NVAL + v) * NW + w) * NPAD + d;
    };

    // honest origin d broadcasts SEND for its key (d, s) with value v: the slot is claimed now (its own thread's
    // slots only), its lifetime is simulated after the step (brc_life.h send_key_now)
    auto send_key_now = [&](uint32_t s, uint32_t v) {
        const uint32_t k = (d * NV) * Q + (s & Qm);
        const uint32_t m = s_meta[k];
        if ((lm_s1(m) != 0 && t < lm_tend(m)) || s >= 0x3FFEu) { ovf = true; return; }
        if constexpr (V8) {
            s_meta[k] = ((t + 1u) << 16) | (s + 1u);   // busy until simulated; the id in its own plane
            s_val[k] = (uint8_t)v;
        } else {
            s_meta[k] = ((t + 1u) << 16) | ((v & 3u) << 14) | (s + 1u);   // busy until simulated
        }
        clr |= 1u << (s & Qm);
        st_msgs += n;
        st_smax = max(st_smax, s);
    };
    // During the consensus pass a replica's SENDs are queued and made after it (brc_life.h send_key): every slot's
    // metadata stays as it was while other replicas read it.  Consecutive phase indices: the first and a value each
    bool defer = false;
    uint32_t sq_s = 0, sq_n = 0;
    auto send_key = [&](uint32_t s, uint32_t v) {
        if (defer) {
            if (sq_n == 0) sq_s = s;
            if (s == sq_s + sq_n && sq_n < Q && sq_n < SENDQ_MAX) s_sq[sq_n++ * NPAD + d] = (uint8_t)(v & VMASK);
            else ovf = true;                         // a (Q+1)-th would find its slot busy (brc_step_wide.h send_later)
            return;
        }
        send_key_now(s, v);
    };
    auto flush_sends = [&]() {
        for (uint32_t i = 0; i < sq_n; ++i) send_key_now(sq_s + i, s_sq[i * NPAD + d]);
        sq_n = 0;
    };
    auto popc_hm = [&](uint32_t v) -> uint32_t {
        uint32_t c = 0;
        if constexpr (V8) {
            if (v >= 4) {
                for (uint32_t w = 0; w < NW; ++w) c += (uint32_t)__popcll(*ghm(v, w));
                return c;
            }
        }
        for (uint32_t w = 0; w < NW; ++w) c += (uint32_t)__popcll(hm(v, w));
        return c;
    };
    auto get_max_val = [&](uint32_t bound2) -> uint32_t {          // :64-68
        for (uint32_t i = 0; i < nvals; ++i) {
            const uint32_t v = (order >> (VB * i)) & VMASK;
            if (2 * popc_hm(v) > bound2) return v;
        }
        return 0;                                                    // str(NONE) == "-1"
    };
    auto cons_reset = [&]() {
        if constexpr (V8) {
            // the HBM planes in use are the ids above 3 in `order` (a plane is non-zero only after an insertion)
            for (uint32_t i = 0; i < nvals; ++i) {
                const uint32_t v = (order >> (VB * i)) & VMASK;
                if (v >= 4)
                    for (uint32_t w = 0; w < NW; ++w) *ghm(v, w) = 0;
            }
        }
        vcount = 0; nvals = 0; order = 0;
        for (uint32_t v = 0; v < 4; ++v)
            for (uint32_t w = 0; w < NW; ++w) hm(v, w) = 0;
    };
    auto cons_deliver_vh = [&](uint32_t v, uint32_t host) {          // :53-106
        // v already inserted? every VB-bit field of `order` compared at once (nvals <= NVAL)
        const uint32_t x = order ^ (v * VREP);
        const uint32_t valid = (1u << (VB * nvals)) - 1u;
        bool found;
        if constexpr (V8) found = (~(x | (x >> 1) | (x >> 2)) & VREP & valid) != 0;
        else found = (~(x | (x >> 1)) & VREP & valid) != 0;
        if (!found) { order |= v << (VB * nvals); ++nvals; }        // :57-58
        if constexpr (V8) {
            if (v >= 4) *ghm(v, host >> 6) |= 1ull << (host & 63);
            else hm(v, host >> 6) |= 1ull << (host & 63);
        } else {
            hm(v, host >> 6) |= 1ull << (host & 63);                 // :60
        }
        ++vcount;                                                    // :61
        if (vcount >= P.T_cnt && phase == 1) {                       // :71
            const uint32_t prop = get_max_val(P.bound_p1);           // :73
            phase = 2; cons_reset();                                 // :75-78
            send_key(2 * (round - 1) + 1, prop);                     // :80-83
        }
        if (vcount >= P.T_cnt && phase == 2) {                       // :86
            const uint32_t dec = get_max_val(P.bound_p2);            // :88 (:89 is always False: decide runs)
            ++dcount;
            if (dcount == 1) { frnd = round; ft = t; fval = dec; }
            lval = dec;
            ++round; phase = 1; cons_reset();                        // :96-100
            send_key(2 * (round - 1), dec);                          // :102-106
        }
    };
    // SPEC consensus (oracle spec_advance / spec_deliver; one key variant per origin: no host sets)
    auto spec_advance = [&]() {
        while (round > 0) {
            const uint32_t s = 2 * (round - 1) + (phase - 1), q = s & Qm;
            const uint32_t cc = cnt(q), n0 = (cc >> 10) & 0x3FF, n1 = cc >> 20;
            if ((cc & 0x3FF) < n - P.f) return;
            cnt(q) = 0;
            if (phase == 1) {
                const uint32_t prop = (2 * n0 > n + P.f) ? 1u : (2 * n1 > n + P.f) ? 2u : 0u;
                phase = 2;
                send_key(s + 1, prop);
            } else {
                const uint32_t vmax = n1 > n0 ? 2u : 1u, cmax = max(n0, n1);
                uint32_t est;
                if (cmax > 2 * P.f) {
                    ++dcount;
                    if (dcount == 1) { frnd = round; ft = t; fval = vmax; }
                    lval = vmax;
                    est = vmax;
                } else if (cmax > P.f) {
                    est = vmax;
                } else {
                    est = coin_id(P.coin_seed, g, round);
                }
                ++round; phase = 1;
                send_key(s + 1, est);
            }
        }
    };
    auto spec_deliver = [&](uint32_t k) {
        const uint32_t sn = s_meta[k] & 0xFFFFu;
        const uint32_t s = (sn & 0x3FFFu) - 1u, v = sn >> 14;
        const uint32_t cur = round ? 2 * (round - 1) + (phase - 1) : 0u;
        if (s < cur) return;
        if (s >= cur + Q) { ovf = true; return; }
        cnt(s & Qm) += 1u + (v == 1 ? 1u << 10 : 0u) + (v == 2 ? 1u << 20 : 0u);
        spec_advance();
    };

    // the BRB cell handler of one receiver class at one relative step (core/brbroadcast.py:60-119): brc_life.h's
    // upd_cell, the same source
    auto upd_cell = [&](uint32_t& fl, uint32_t& ec, uint32_t& rc, bool opn, uint32_t sa, uint32_t ea, uint32_t ra,
                        bool hS, bool hE, bool hR, uint32_t& es, uint32_t& rs, uint32_t& dl, uint32_t& nr) {
#include "brc_life_cell.h"
    };
    // ---- the lifetimes of one batch of new keys, one per lane (lane L: key slot k of origin 64 wid + L, `has`):
    // brc_life.h simulate_batch, sender peers.  Wave-local: the loop runs to the wave's own last pending step, and
    // what it shares with the other waves -- the ring rows and `rows` -- it adds with no-return LDS atomics
    auto simulate_batch = [&](const bool has, const uint32_t k) {
        const bool vA = nHF != 0, vB = nHS != 0;
        const bool oF = laneF;                        // the origin is this lane
        const uint32_t sdlA = oF ? 1u : Dd;           // SEND arrival step at class A (class B: Dd)
        // pending message types of the next steps, a window sliding with r: bit j of field S (bits 0-9),
        // E (10-19), R (20-29) <=> step r + j (a message lands at most Dd <= 8 steps after it is sent)
        uint32_t pend = 0;
        if (has) {
            if (oF && vA) pend |= 1u;
            if (vB || (!oF && vA)) pend |= 1u << (Dd - 1u);
        }
        uint32_t flA = 0, ecA = 0, rcA = 0, flB = 0, ecB = 0, rcB = 0;
        // the relative steps the classes SENT ECHO / READY, a byte each (0xFF: not sent): A's ECHO, A's READY,
        // B's ECHO, B's READY
        uint32_t sent = 0xFFFFFFFFu;
        uint32_t last = t;
        uint32_t rstep = 1;                           // steps to the next one some lane of the wave has pending
#pragma unroll 1
        for (uint32_t r = 1; ; r += rstep) {
            if (!__ballot(pend != 0u)) break;
            const bool hS = (pend & 1u) != 0, hE = (pend & (1u << 10)) != 0, hR = (pend & (1u << 20)) != 0;
            bool act = hS || hE || hR;
            if (act && r > RW) {                      // past the ring: overflow (cannot happen for Dd <= 8)
                ovf = true; act = false;
                pend = 0;
            }
            const uint32_t ts = t + r, row = ts & (RW - 1);
            const uint32_t c1 = r - 1u, cD = r >= Dd ? r - Dd : 0x100u;   // 0x100: matches no byte
            // class arrivals: fast senders (class A) land on A after 1 step, every other pair after Dd
            uint32_t eA = 0, eB = 0, rA = 0, rB = 0;
            // which class sent now-landing messages: e1 / q1 A's ECHO / READY sent at r - 1, e3 / q3 at
            // r - Dd, e2 / q2 B's at r - Dd
            bool e1 = false, e2 = false, e3 = false, q1 = false, q2 = false, q3 = false;
            if (hE) {
                const uint32_t xA = sent & 0xFFu, xB = (sent >> 16) & 0xFFu;
                e1 = xA == c1; e2 = xB == cD; e3 = xA == cD;
                eA = (e1 ? nHF : 0u) + (e2 ? nHS : 0u);
                eB = (e3 ? nHF : 0u) + (e2 ? nHS : 0u);
            }
            if (hR) {
                const uint32_t xA = (sent >> 8) & 0xFFu, xB = sent >> 24;
                q1 = xA == c1; q2 = xB == cD; q3 = xA == cD;
                rA = (q1 ? nHF : 0u) + (q2 ? nHS : 0u);
                rB = (q3 ? nHF : 0u) + (q2 ? nHS : 0u);
            }
            const uint32_t saA = (hS && r == sdlA) ? 1u : 0u, saB = (hS && r == Dd) ? 1u : 0u;
            const uint32_t aA = act ? eA + rA + saA : 0u, aB = act ? eB + rB + saB : 0u;
            // a delivered cell ignores everything (core/brbroadcast.py:74)
            const bool opnA = vA && aA != 0 && !(flA & F_DEL), opnB = vB && aB != 0 && !(flB & F_DEL);
            uint32_t esA = 0, rsA = 0, dlA = 0, esB = 0, rsB = 0, dlB = 0, nrA = 0, nrB = 0;
            if (act) {
                upd_cell(flA, ecA, rcA, opnA, saA, eA, rA, hS, hE, hR, esA, rsA, dlA, nrA);
                upd_cell(flB, ecB, rcB, opnB, saB, eB, rB, hS, hE, hR, esB, rsB, dlB, nrB);
            }
            if (esA | rsA | esB | rsB) {
                const uint32_t sm = (esA ? 0xFFu : 0u) | (rsA ? 0xFF00u : 0u) | (esB ? 0xFF0000u : 0u) | (rsB ? 0xFF000000u : 0u);
                sent = (sent & ~sm) | ((r * 0x01010101u) & sm);
            }
            // step statistics over the wave's batch (brc_life.h BRC_LIFE_BSTAT): arrivals nHF aA + nHS aB, messages
            // n (nHF (esA + rsA) + nHS (esB + rsB)), cells nHF [aA > 0] + nHS [aB > 0], deliveries nHF dlA + nHS dlB,
            // as popcounts of ballots times class sizes -- whole words (n = 256: aA reaches 513)
            const uint64_t am = __ballot(act);
            if (am) {
                auto pc = [&](bool c) -> uint32_t { return (uint32_t)__popcll(__ballot(act && c)); };
                const uint32_t n2 = pc(e2) + pc(q2);
                const uint32_t sA = nHF * (pc(e1) + pc(q1)) + nHS * n2 + pc(saA != 0);
                const uint32_t sB = nHF * (pc(e3) + pc(q3)) + nHS * n2 + pc(saB != 0);
                const uint32_t arr = nHF * sA + nHS * sB;
                const uint32_t msgs = n * (nHF * (pc(esA != 0) + pc(rsA != 0)) + nHS * (pc(esB != 0) + pc(rsB != 0)));
                const uint32_t cells = nHF * pc(aA != 0) + nHS * pc(aB != 0);
                const uint32_t dels = nHF * pc(dlA != 0) + nHS * pc(dlB != 0);
                if (lane == 0) {
                    if (arr) atomicAdd(&s_rg[row], arr);
                    if (msgs) atomicAdd(&s_rg[RW + row], msgs);
                    if (cells) atomicAdd(&s_rg[2 * RW + row], cells);
                    if (dels) atomicAdd(&s_rg[3 * RW + row], dels);
                    atomicOr(&s_ctl[0], 1u << row);
                    st_ksteps += (uint32_t)__popcll(am);
                }
            }
            if (dlA || dlB) {
                // a class delivers the key at step ts, whole (this lane's own slot)
                const uint32_t tc = 0x80u | (ts & 0x7Fu);
                if (dlA) s_dA[k] = (uint8_t)tc;
                if (dlB) s_dB[k] = (uint8_t)tc;
            }
            // the messages sent now land on class A after 1 step (fast senders) and on every other pair
            // after Dd steps
            if (esA || esB) {
                if (esA) pend |= 1u << 11;
                if (vB || esB) pend |= 1u << (10u + Dd);
            }
            if (rsA || rsB) {
                if (rsA) pend |= 1u << 21;
                if (vB || rsB) pend |= 1u << (20u + Dd);
            }
            if (act) last = ts;
            // step r consumed; the window moves to the next step any lane of the wave's batch has pending (the
            // lowest offset over the three fields and the wave: no set bit crosses a field boundary)
            pend &= ~(1u | (1u << 10) | (1u << 20));
            const uint32_t m = uni32(wave_or_all((pend | (pend >> 10) | (pend >> 20)) & 0x3FFu));
            rstep = m ? (uint32_t)__builtin_ctz(m) : 1u;
            pend >>= rstep;
        }
        if (has) s_meta[k] = (s_meta[k] & 0xFFFFu) | (last << 16);
    };
    // the keys this wave's origins created this step, each simulated once.  No barrier inside: the batches of
    // different waves are independent, and the caller's next barrier publishes what they leave
    auto simulate_new = [&]() {
#pragma unroll 1
        for (;;) {
            const bool has = clr != 0;
            uint32_t k = 0;
            if (has) { k = (d * NV) * Q + (uint32_t)__ffs(clr) - 1u; clr &= clr - 1u; }
            if (!__ballot(has)) break;
            simulate_batch(has, k);
        }
    };

    // ---- step 0: the proposals (actions stamped 0, core/byzantinerandomizedconsensus.py:38-50)
    if (honest) {
        const uint32_t v = (P.proposals == BRC_PROPOSALS_PHILOX) ? proposal_id(P.seed, g, d)
                                                                 : (uint32_t)gp(P.prop)[inst * n + d];
        round = 1; phase = 1;
        send_key(0, v & VMASK);
        if constexpr (SPEC) spec_advance();
    }
    if (block_or(ovf ? 1u : 0u)) {
        status = BRC_OVERFLOW;
    } else {
        simulate_new();
        if constexpr (PAT) {
            // ---- the equivocation pattern: every Byzantine lane's two keys (b NV + v, s = 0), value id 1 + v.
            // simulate_batch over four receiver classes: [0] fast in [1] fast out [2] slow in [3] slow out ("in": the
            // replica's parity is v, it gets the SEND); nC their honest sizes.  The origin is this lane (t = 0).
            auto simulate_pattern = [&](const bool has, const uint32_t v) {
                const uint32_t nC[4] = {v ? nFo : nFe, v ? nFe : nFo, v ? nSo : nSe, v ? nSe : nSo};
                const uint32_t k = (d * NV + v) * Q, x = 2 * d + v;
                const bool oF = laneF;
                // bit j of field S (bits 0-9), E (10-19), R (20-29) <=> something may land at step r + j (a superset:
                // the arrivals below are exact).  The SEND lands at 1 (fast origin, fast class) or Dd; the origin's
                // ECHO and READY, stamped 1, at 2 or 1 + Dd
                uint32_t pend = 0;
                if (has) {
                    if constexpr (V8) {
                        s_meta[k] = (1u << 16) | 1u;
                        s_val[k] = (uint8_t)(1u + v);
                    } else {
                        s_meta[k] = (1u << 16) | ((1u + v) << 14) | 1u;
                    }
                    st_msgs += v ? n / 2u : (n + 1u) / 2u;          // the SEND, to every replica of parity v
                    pend = (1u << (Dd - 1u)) | (1u << (10u + Dd)) | (1u << (20u + Dd));
                    if (oF) pend |= 1u | (1u << 11) | (1u << 21);
                }
                {
                    // the origin's ECHO and READY of this key go to all n replicas at step 1
                    const uint32_t c = (uint32_t)__popcll(__ballot(has));
                    if (lane == 0 && c) atomicAdd(&s_rg[RW + 1], 2u * n * c);
                }
                uint32_t fl[4] = {0, 0, 0, 0}, ec[4] = {0, 0, 0, 0}, rc[4] = {0, 0, 0, 0};
                uint32_t sE = 0xFFFFFFFFu, sR = 0xFFFFFFFFu;        // byte c: the step class c SENT ECHO / READY (0xFF: not)
                uint32_t last = 1;
                uint32_t rstep = 1;
                auto wsum = [&](uint32_t y) -> uint32_t {
#pragma unroll
                    for (int o = 32; o; o >>= 1) y += (uint32_t)__shfl_xor((int)y, o);
                    return y;
                };
#pragma unroll 1
                for (uint32_t r = 1; ; r += rstep) {
                    if (!__ballot(pend != 0u)) break;
                    bool due = (pend & (1u | (1u << 10) | (1u << 20))) != 0;
                    if (due && r > RW) {                             // past the ring (cannot happen for Dd <= 8)
                        ovf = true; due = false;
                        pend = 0;
                    }
                    const uint32_t row = r & (RW - 1);
                    const uint32_t c1 = r - 1u, cD = r >= Dd ? r - Dd : 0x100u;
                    // ECHO / READY arrivals at a fast (F) and at a slow (S) receiver: fast senders land on fast
                    // receivers after 1 step, every other pair after Dd; the origin's own count one each
                    uint32_t eF = 0, eS = 0, rF = 0, rS = 0;
#pragma unroll
                    for (uint32_t c = 0; c < 4; ++c) {
                        const uint32_t xe = (sE >> (8 * c)) & 0xFFu, xr = (sR >> (8 * c)) & 0xFFu;
                        const uint32_t eD = xe == cD ? nC[c] : 0u, rD = xr == cD ? nC[c] : 0u;
                        eS += eD; rS += rD;
                        if (c < 2) { eF += xe == c1 ? nC[c] : 0u; rF += xr == c1 ? nC[c] : 0u; }
                        else { eF += eD; rF += rD; }
                    }
                    const uint32_t oS = r == 1u + Dd ? 1u : 0u, oFst = r == (oF ? 2u : 1u + Dd) ? 1u : 0u;
                    eF += oFst; rF += oFst; eS += oS; rS += oS;
                    const uint32_t sa[4] = {r == (oF ? 1u : Dd) ? 1u : 0u, 0u, r == Dd ? 1u : 0u, 0u};
                    const bool hS = due && (sa[0] | sa[2]) != 0, hE = due && (eF | eS) != 0, hR = due && (rF | rS) != 0;
                    uint32_t arr = 0, msgs = 0, cells = 0, dels = 0, esm = 0, rsm = 0;
#pragma unroll
                    for (uint32_t c = 0; c < 4; ++c) {
                        const uint32_t e = c < 2 ? eF : eS, q = c < 2 ? rF : rS;
                        const uint32_t a = due ? e + q + sa[c] : 0u;
                        const bool opn = nC[c] != 0 && a != 0 && !(fl[c] & F_DEL);   // a delivered cell ignores everything
                        uint32_t es = 0, rs = 0, dl = 0, nr = 0;
                        if (due) upd_cell(fl[c], ec[c], rc[c], opn, sa[c], e, q, hS, hE, hR, es, rs, dl, nr);
                        arr += nC[c] * a;
                        msgs += nC[c] * (es + rs);
                        cells += a ? nC[c] : 0u;
                        dels += dl ? nC[c] : 0u;
                        if (es) esm |= 0xFFu << (8 * c);
                        if (rs) rsm |= 0xFFu << (8 * c);
                        if (dl) {
                            // class c delivers the key at step r, whole (this lane's own slot and table entry)
                            const uint8_t tc = (uint8_t)(0x80u | (r & 0x7Fu));
                            if (c == 0) s_dA[k] = tc;
                            else if (c == 1) s_oA[x] = tc;
                            else if (c == 2) s_dB[k] = tc;
                            else s_oB[x] = tc;
                        }
                    }
                    sE = (sE & ~esm) | ((r * 0x01010101u) & esm);
                    sR = (sR & ~rsm) | ((r * 0x01010101u) & rsm);
                    // step statistics over the wave's batch: whole words, one atomic per counter; the row is marked
                    // only when a message reaches an honest receiver
                    if (__ballot(due)) {
                        const uint32_t wa = wsum(arr), wm = wsum(msgs), wc = wsum(cells), wd = wsum(dels);
                        if (lane == 0) {
                            if (wa) { atomicAdd(&s_rg[row], wa); atomicOr(&s_ctl[0], 1u << row); }
                            if (wm) atomicAdd(&s_rg[RW + row], n * wm);
                            if (wc) atomicAdd(&s_rg[2 * RW + row], wc);
                            if (wd) atomicAdd(&s_rg[3 * RW + row], wd);
                            st_ksteps += (uint32_t)__popcll(__ballot(due));
                        }
                    }
                    // what the classes sent now may land on the fast classes after 1 step, anywhere after Dd
                    if (esm) pend |= ((esm & 0xFFFFu) ? 1u << 11 : 0u) | (1u << (10u + Dd));
                    if (rsm) pend |= ((rsm & 0xFFFFu) ? 1u << 21 : 0u) | (1u << (20u + Dd));
                    if (arr) last = r;
                    pend &= ~(1u | (1u << 10) | (1u << 20));
                    const uint32_t m = uni32(wave_or_all((pend | (pend >> 10) | (pend >> 20)) & 0x3FFu));
                    rstep = m ? (uint32_t)__builtin_ctz(m) : 1u;
                    pend >>= rstep;
                }
                if (has) s_meta[k] = (s_meta[k] & 0xFFFFu) | (last << 16);
            };
            const bool byz_lane = real && !honest;
            simulate_pattern(byz_lane, 0u);
            simulate_pattern(byz_lane, 1u);
        }
    }
    __syncthreads();                                 // the new keys' ring rows, class bytes and slot stamps

    const uint64_t gm0 = (1ull << Q) - 1;            // Q <= 32
    while (status == BRC_RUNNING) {
        // next step with arrivals at an honest receiver (every thread reads the same word, after a barrier)
        const uint32_t rows = uni32(s_ctl[0]);
        const uint32_t rot = (t + 1) & (RW - 1);
        uint32_t rr = rot ? ((rows >> rot) | (rows << (RW - rot))) : rows;
        if constexpr (PAT) {
            if (t == 0 && any_byz) rr |= 1u;         // step 1: the pattern's ECHOs and READYs are sent then
        }
        if (!rr) { status = BRC_QUIESCENT; break; }
        const uint32_t next = t + 1 + (uint32_t)__builtin_ctz(rr);
        if (next > P.step_cap) { status = BRC_STEPCAP; break; }
        t = next;
        const uint32_t row = t & (RW - 1);
        // commit the step's statistics
        {
            const uint32_t a = uni32(s_rg[row]), mg = uni32(s_rg[RW + row]);
            const uint32_t ce = uni32(s_rg[2 * RW + row]), de = uni32(s_rg[3 * RW + row]);
            if (tid == 0) { st_arr += a; st_msgs += mg; st_cells += ce; st_del += de; }
            if (ce) t_stop = t;
            if constexpr (PAT) {
                if (t == 1 && any_byz) t_stop = t;   // an action step counts as active
            }
        }
        // the step's two class bitmaps per key word: the keys whose delivery step for the class is now; consumed
        // entries are freed for step t + 128 here, by the wave that ballots the word
        {
            const uint32_t tc = 0x80u | (t & 0x7Fu);
            for (uint32_t w = wid; w < nkw; w += NW) {
                const uint32_t kk = w * 64 + lane;
                const bool a = s_dA[kk] == tc, b = s_dB[kk] == tc;
                if constexpr (PAT) {
                    // a pattern key (phase slot 0 of variant v = 0 / 1 of a Byzantine origin): dA / dB hold its
                    // in-classes (replica parity v), oA / oB the out-classes; any other key: both parities alike
                    const uint32_t o = kk >> ksh, v = (kk >> qsh) & (NV - 1u);
                    const bool pat = (kk & Qm) == 0 && v < 2 && ((s_pbyz[o >> 6] >> (o & 63)) & 1ull);
                    bool ao = a, bo = b;
                    if (pat) {
                        const uint32_t x = 2 * o + v;
                        ao = s_oA[x] == tc; bo = s_oB[x] == tc;
                        if (ao) s_oA[x] = 0;
                        if (bo) s_oB[x] = 0;
                    }
                    const bool odd = pat && v == 1;  // in-class parity
                    const uint64_t kAe = __ballot(odd ? ao : a), kBe = __ballot(odd ? bo : b);
                    const uint64_t kAo = __ballot((pat && !odd) ? ao : a), kBo = __ballot((pat && !odd) ? bo : b);
                    if (lane == 0) { s_kab[4 * w] = kAe; s_kab[4 * w + 1] = kBe; s_kab[4 * w + 2] = kAo; s_kab[4 * w + 3] = kBo; }
                } else {
                    const uint64_t kA = __ballot(a), kB = __ballot(b);
                    if (lane == 0) { s_kab[2 * w] = kA; s_kab[2 * w + 1] = kB; }
                }
                if (a) s_dA[kk] = 0;
                if (b) s_dB[kk] = 0;
            }
        }
        __syncthreads();                             // bitmaps built; every thread has read `rows` and the ring row
        // the step is consumed: its ring row is free for step t + RW (nothing adds to the rings before the
        // reduction's barrier below)
        if (tid == 0) {
            s_rg[row] = 0; s_rg[RW + row] = 0; s_rg[2 * RW + row] = 0; s_rg[3 * RW + row] = 0;
            s_ctl[0] = rows & ~(1u << row);
        }
        // ================= consensus: this step's deliveries in canonical (kp, s) order, each replica its own
        defer = true;
        if (cons_lane) {
            const uint32_t cls = (laneF ? 0u : 1u) + (PAT ? 2u * (d & 1u) : 0u);
#pragma unroll 1
            for (uint32_t w = 0; w < nkw; ++w) {
                uint64_t bits = s_kab[KC * w + cls];
                // one delivery at a time, ascending slot; several phases of one key prefix: smallest s first
                while (bits) {
                    uint32_t best = (uint32_t)__ffsll((unsigned long long)bits) - 1u;
                    const uint64_t grp = bits & (gm0 << (best & ~Qm));
                    if (grp & (grp - 1)) {
                        uint32_t bs = 0xFFFFFFFFu;
                        for (uint64_t x = grp; x; x &= x - 1) {
                            const uint32_t bb = (uint32_t)__ffsll((unsigned long long)x) - 1u;
                            const uint32_t s1 = s_meta[w * 64 + bb] & 0x3FFFu;
                            if (s1 < bs) { bs = s1; best = bb; }
                        }
                    }
                    bits &= ~(1ull << best);
                    const uint32_t k = w * 64 + best;
                    if constexpr (SPEC) spec_deliver(k);
                    else if constexpr (V8) cons_deliver_vh(s_val[k], k >> ksh);
                    else cons_deliver_vh((s_meta[k] & 0xFFFFu) >> 14, k >> ksh);
                }
            }
        }
        __syncthreads();                             // every replica has read the slots' metadata
        defer = false;
        flush_sends();                               // the SENDs this step's consensus started (own slots)
        // ================= per-instance stop conditions (one workgroup reduction)
        const uint32_t flags = block_or((ovf ? 1u : 0u) | ((honest && dcount < P.round_cap) ? 2u : 0u));
        if (flags & 1u) status = BRC_OVERFLOW;
        else if (P.round_cap > 0 && !(flags & 2u)) status = BRC_DONE;
        if (status == BRC_RUNNING) simulate_new();    // the keys this step's consensus created
        __syncthreads();
    }
    if (block_or(ovf ? 1u : 0u) && status != BRC_OVERFLOW) status = BRC_OVERFLOW;

    // ---- write back (brc_step_wide.h layout: inst, istats, items, cons0 / cons1, gcount)
    if (tid == 0) {
        gp(P.actany)[inst] = 0;
        ItemState o = {t, 0u, 1u, 0u};
        P.items[inst] = o;
    }
    const size_t li = inst * NPAD + d;
    if (honest) {
        gp(P.cons0)[li] = cons0_pack(round, phase, nvals, order, vcount);
        gp(P.cons1)[li] = (uint64_t)(dcount & 0xFFFF) | ((uint64_t)(frnd & 0xFFFF) << 16) | ((uint64_t)(ft & 0xFFFF) << 32) |
                          ((uint64_t)(fval & 0xFF) << 48) | ((uint64_t)(lval & 0xFF) << 56);
    }
    // statistics: wave sums, then one atomic per wave and counter (the engine is fresh: istats start at zero)
    uint64_t w6[5] = {st_cells, st_arr, st_msgs, st_del, st_ksteps * 64ull};
#pragma unroll
    for (int q = 0; q < 5; ++q) {
#pragma unroll
        for (int o = 32; o; o >>= 1) w6[q] += (uint64_t)__shfl_xor((unsigned long long)w6[q], o);
    }
    const uint32_t smax = wave_max_all(st_smax);
    if (lane == 0) {
        // istats row: msgs, arrivals, cell-steps, deliveries
        const uint64_t row4[4] = {w6[2], w6[1], w6[0], w6[3]};
#pragma unroll
        for (int q = 0; q < 4; ++q) if (row4[q]) atomicAdd((unsigned long long*)&P.istats[inst * 4 + q], (unsigned long long)row4[q]);
#pragma unroll
        for (int q = 0; q < 5; ++q) if (w6[q]) atomicAdd(&P.gcount[q], (unsigned long long)w6[q]);
        if (smax) atomicMax(&P.gcount[5], (unsigned long long)smax);
    }
    if (tid == 0) {
        gptr_t<uint64_t> ip = (gptr_t<uint64_t>)&gp(P.inst)[inst];
        *ip = (uint64_t)(status & 0xFFFF) | ((uint64_t)(t_stop & 0xFFFF) << 16) | ((uint64_t)(t & 0xFFFF) << 32);
    }
}

template <int NPAD, int MODE, bool PAT = false, bool V8 = false>
int launch_life_wide_one(uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P) {
    auto kern = brc_life_wide<NPAD, MODE, PAT, V8>;
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return BRC_E_HIP;
    kern<<<dim3(blocks), dim3(NPAD), lds, s>>>(P);
    return hipGetLastError() == hipSuccess ? 0 : BRC_E_HIP;
}

template <int NPAD>
int launch_life_wide_npad(int mode, uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P) {
    if (mode == BRC_MODE_SPEC) return launch_life_wide_one<NPAD, BRC_MODE_SPEC>(blocks, lds, s, P);
    if (mode == BRC_MODE_BEB) return launch_life_wide_one<NPAD, BRC_MODE_BEB>(blocks, lds, s, P);
    if (mode == BRC_MODE_REFERENCE) return launch_life_wide_one<NPAD, BRC_MODE_REFERENCE>(blocks, lds, s, P);
    return BRC_E_INVALID;
}

// the pattern form (BRC_FLAG_LIFE_PATTERN): REFERENCE / BEB
template <int NPAD>
int launch_life_wide_pat_npad(int mode, uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P) {
    if (mode == BRC_MODE_BEB) return launch_life_wide_one<NPAD, BRC_MODE_BEB, true>(blocks, lds, s, P);
    if (mode == BRC_MODE_REFERENCE) return launch_life_wide_one<NPAD, BRC_MODE_REFERENCE, true>(blocks, lds, s, P);
    return BRC_E_INVALID;
}

// the V8 instantiations (BRC_FLAG_LIFE_VALUES: 3-bit value ids): REFERENCE / BEB, with and without the pattern
template <int NPAD>
int launch_life_wide_val_npad(int mode, bool pat, uint32_t blocks, uint32_t lds, hipStream_t s, const Params* P) {
    if (mode == BRC_MODE_BEB)
        return pat ? launch_life_wide_one<NPAD, BRC_MODE_BEB, true, true>(blocks, lds, s, P)
                   : launch_life_wide_one<NPAD, BRC_MODE_BEB, false, true>(blocks, lds, s, P);
    if (mode == BRC_MODE_REFERENCE)
        return pat ? launch_life_wide_one<NPAD, BRC_MODE_REFERENCE, true, true>(blocks, lds, s, P)
                   : launch_life_wide_one<NPAD, BRC_MODE_REFERENCE, false, true>(blocks, lds, s, P);
    return BRC_E_INVALID;
}

}  // namespace brc
