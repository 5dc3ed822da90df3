// brc_engine.hip -- host side of the MI355X batched consensus engine: the C-ABI of
// include/brc.h (brc_create ... brc_destroy), device memory, injection CSR upload, and the small
// helper kernels.  The step kernel itself is brc_step.h, instantiated per replica-set width in
// brc_kern_<NPAD>.hip.
//
// Reference boundary replaced (sithu/ByzantineRandomizedConsensus):
//   BRBroadcast / ByzantineRandomizedConsensus constructors  -> brc_create
//   the listener accept loop (core/brbroadcast.py:60-128)     -> brc_run (one step-kernel launch)
//   Broadcast.broadcast / Consensus.propose                   -> brc_inject / brc_load_proposals
//   deliver / decide upcalls                                  -> brc_read_events / brc_read_replicas
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "brc_internal.h"
#include "brc_inject.h"
#include "brc_plan.h"

namespace {

using namespace brc;

// Byzantine equivocation pattern expanded straight into the CSR lists.
// bw: Byzantine-mask words per instance (n > 64: one instance per item, ipw = 1)
__global__ void expand_equivocate(InjDev* inj, uint32_t* off, uint32_t* cnt, const uint64_t* byz,
                                  uint64_t instances, uint64_t nitems, uint32_t ipw, uint32_t n, uint32_t nv,
                                  uint32_t Q, uint32_t per_item, uint32_t bw) {
    const uint64_t item = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= nitems) return;
    InjDev* o = inj + item * per_item;
    uint32_t c = 0;
    uint64_t even[4] = {0, 0, 0, 0}, odd[4] = {0, 0, 0, 0};   // 64 is even: bit parity = replica parity
    for (uint32_t dd = 0; dd < n; ++dd) {
        if (dd & 1) odd[dd >> 6] |= 1ull << (dd & 63); else even[dd >> 6] |= 1ull << (dd & 63);
    }
    for (int pass = 0; pass < 2; ++pass) {
        for (uint32_t sgi = 0; sgi < ipw; ++sgi) {
            const uint64_t in = item * ipw + sgi;
            if (in >= instances) break;
            for (uint32_t b = 0; b < n; ++b) {
                if (!((byz[in * bw + (b >> 6)] >> (b & 63)) & 1ull)) continue;
                for (uint32_t v = 0; v < 2; ++v) {
                    const uint32_t kp = b * nv + v;
                    InjDev r = {};
                    r.slot = (uint16_t)(kp * Q + 0); r.s = 0; r.seg = (uint8_t)sgi; r.node = (uint8_t)b;
                    r.value = (int8_t)(1 + v);
                    if (pass == 0) {
                        r.t = 0; r.kind = BRC_INJ_SEND; r.type = BRC_SEND; r.restricted = 1;
                        const uint64_t* dm = v ? odd : even;
                        r.dst = dm[0]; r.dst_hi[0] = dm[1]; r.dst_hi[1] = dm[2]; r.dst_hi[2] = dm[3];
                        o[c++] = r;
                    } else {
                        r.t = 1; r.kind = BRC_INJ_MSG; r.dst = ~0ull;
                        r.type = BRC_ECHO; o[c++] = r;
                        r.type = BRC_READY; o[c++] = r;
                    }
                }
            }
        }
    }
    off[item] = (uint32_t)(item * per_item);
    cnt[item] = c;
}

// brc_reset: free every slot but keep its generation.  Cells are left alone: the next
// allocation of a slot bumps its generation, which makes every cell of the old key stale
// (send steps included, brc_step.h), so a reset costs O(keys), not O(cells).
__global__ void reset_slots(uint64_t* meta, uint32_t* mgen, uint64_t keys) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < keys) { meta[i] = 0; mgen[i] &= GEN_MASK; }
}

// Decide-round histogram: per instance, the round by which EVERY honest replica
// had decided (max of the first-decide rounds); bin 0 = some honest replica never decided; rounds
// >= bins-1 share the last bin.  One thread per instance; the bins are reduced in LDS first.
__global__ void round_histogram(const uint64_t* cons1, const uint64_t* byz, uint64_t instances, uint32_t ipw,
                                uint32_t lpi, uint32_t npad, uint32_t bw, uint32_t n, uint32_t bins,
                                unsigned long long* hist) {
    extern __shared__ unsigned long long sh[];
    for (uint32_t b = threadIdx.x; b < bins; b += blockDim.x) sh[b] = 0;
    __syncthreads();
    const uint64_t in = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (in < instances) {
        const uint64_t item = in / ipw, seg = in % ipw;
        uint32_t worst = 0;
        bool all = true;
        for (uint32_t d = 0; d < n; ++d) {
            if ((byz[in * bw + d / 64] >> (d % 64)) & 1ull) continue;
            const uint64_t c1 = cons1[item * lpi + seg * npad + d];
            if ((c1 & 0xFFFF) == 0) { all = false; break; }
            worst = max(worst, (uint32_t)((c1 >> 16) & 0xFFFF));
        }
        const uint32_t bin = all ? min(worst, bins - 1) : 0u;
        atomicAdd(&sh[bin], 1ull);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < bins; b += blockDim.x)
        if (sh[b]) atomicAdd(&hist[b], sh[b]);
}

// First decisions of the honest replicas (brc_read_value_decisions): per instance, count each honest
// replica's first decided value id (bin 8: never decided) and flag instances whose honest replicas
// decided different values.  One thread per instance; bins reduced in LDS first.
__global__ void decision_histogram(const uint64_t* cons1, const uint64_t* byz, uint64_t instances, uint32_t ipw,
                                   uint32_t lpi, uint32_t npad, uint32_t bw, uint32_t n,
                                   unsigned long long* out /* [10]: 9 value bins, disagreements */) {
    __shared__ unsigned long long sh[10];
    if (threadIdx.x < 10) sh[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t in = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (in < instances) {
        const uint64_t item = in / ipw, seg = in % ipw;
        uint32_t cnt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        uint32_t seen = 0;                       // value ids decided by some honest replica
        for (uint32_t d = 0; d < n; ++d) {
            if ((byz[in * bw + d / 64] >> (d % 64)) & 1ull) continue;
            const uint64_t c1 = cons1[item * lpi + seg * npad + d];
            if ((c1 & 0xFFFF) == 0) { ++cnt[8]; continue; }
            const uint32_t v = (uint32_t)(c1 >> 48) & 7u;      // first decided value id
            ++cnt[v];
            seen |= 1u << v;
        }
        for (int b = 0; b < 9; ++b) if (cnt[b]) atomicAdd(&sh[b], (unsigned long long)cnt[b]);
        if (seen & (seen - 1)) atomicAdd(&sh[9], 1ull);
    }
    __syncthreads();
    if (threadIdx.x < 10 && sh[threadIdx.x]) atomicAdd(&out[threadIdx.x], sh[threadIdx.x]);
}

// grid-stride fill: a dispatch holds < 2^32 work-items per dimension, and the cell array can
// exceed that (2^17 instances x 512 key slots x 64 lanes = 2^32 words at n = 64, Q = 8)
template <typename W> __global__ void fill_words(W* p, W v, uint64_t count) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) p[i] = v;
}

// ------------------------------------------------------------------------------------ host
// The plan (brc_plan.h: geometry, kernel family, buffer sizes -- fixed by brc_create) and the engine's run-time state
struct Engine : Plan {
    brc_config cfg;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_ms = 0.f;
    std::string err;
    uint64_t* cells = nullptr;
    uint64_t* meta = nullptr; uint32_t* mgen = nullptr; uint64_t* kdst = nullptr;
    uint64_t* act = nullptr; uint32_t* actany = nullptr; ItemState* items = nullptr;
    InstState* inst = nullptr; uint64_t* istats = nullptr;
    uint64_t* cons0 = nullptr; uint64_t* cons1 = nullptr; void* hmask = nullptr;
    InjDev* inj = nullptr; uint32_t* inj_off = nullptr; uint32_t* inj_cnt = nullptr; size_t inj_capacity = 0;
    uint64_t* byz = nullptr; int8_t* prop = nullptr;
    brc_event* events = nullptr; unsigned long long* event_count = nullptr;
    unsigned long long* gcount = nullptr;
    uint64_t* dbits = nullptr;                   // lean SPEC: per-wave delivery bitmaps (brc_step.h DBG)
    uint64_t* dring = nullptr;                   // per-link lifetime kernel: delivery bitmap ring (brc_life.h)
    uint32_t* lmeta = nullptr;                   // two-class lifetime kernel, key windows >= 32 (life_hbm_meta): slot metadata in HBM
    uint64_t* xsend = nullptr; uint32_t* xsn = nullptr;   // extra-SEND records (non-lean step kernels)
    bool values_wide = false;                    // a loaded proposal uses a value id >= 4 (no lifetime kernel)
    Params* dparams = nullptr;                   // device copy of the launch parameters
    Params hparams;
    std::vector<std::vector<InjDev>> pending;   // per item: uploaded-but-unconsumed + new
    bool inj_dirty = false, pattern_active = false;
    InjectBook book;                            // the injections taken, the slot generation budget (brc_inject.h)
    std::vector<uint64_t> hbyz;                 // host copy of the per-instance Byzantine masks [instance][bw]
    // key-lifetime kernel (brc_life.h; life_cfg: eligible configuration): engine fresh since create / reset,
    // and whether the last run used it (its instances are then final: no re-opening injections)
    bool fresh = true, life_done = false, last_life = false;
    bool cells_ready = false;                    // the step kernel's cell array (allocated on first use
                                                 // when the lifetime kernel may serve the engine)
};

thread_local std::string g_create_err;    // brc_last_error(NULL): the last brc_create failure

#define HIPCHK(e, x)                                                                   \
    do {                                                                               \
        hipError_t _r = (x);                                                           \
        if (_r != hipSuccess) {                                                        \
            (e)->err = std::string(#x) + ": " + hipGetErrorString(_r);                 \
            return BRC_E_HIP;                                                          \
        }                                                                              \
    } while (0)

// The one place a kernel is chosen: the plan's family and this run's `life` decision (brc_run)
static int launch_kernel(const Engine* e, bool life, const Params* P) {
    const int npad = e->npad, dm = e->dm, mode = e->kmode;
    const bool events = e->cfg.event_capacity != 0;
    const uint32_t items = (uint32_t)e->nitems, lds = e->lds_bytes;
    const uint32_t blocks = e->wide ? items : (uint32_t)((e->nitems + WPB - 1) / WPB);
    hipStream_t st = e->stream;
    if (life && e->wide) {
        // the wide key-lifetime kernel (BRC_FLAG_WIDE_LIFE): one workgroup of NPAD threads per instance
        if (e->life_val) return npad == 128 ? launch_life_128v(mode, e->life_pat, items, e->life_lds, st, P)
                              : npad == 256 ? launch_life_256v(mode, e->life_pat, items, e->life_lds, st, P) : BRC_E_INVALID;
        if (e->life_pat) return npad == 128 ? launch_life_128p(mode, items, e->life_lds, st, P)
                              : npad == 256 ? launch_life_256p(mode, items, e->life_lds, st, P) : BRC_E_INVALID;
        return npad == 128 ? launch_life_128(mode, items, e->life_lds, st, P)
             : npad == 256 ? launch_life_256(mode, items, e->life_lds, st, P) : BRC_E_INVALID;
    }
    if (life) return launch_life(mode, e->life_pl, e->life_rw == LIFE_RW16, e->cfg.key_window >= 64, e->has_lmeta, items,
                                 e->life_lds, st, P);
    if (e->regmask) return launch_step_64r(dm, events, mode, blocks, lds, st, P);
    if (e->wide_val) return npad == 128 ? launch_step_128v(dm, events, mode, blocks, lds, st, P)
                                        : launch_step_256v(dm, events, mode, blocks, lds, st, P);
    if (e->wide_rec) return npad == 128 ? launch_step_128x(dm, events, mode, blocks, lds, st, P)
                                        : launch_step_256x(dm, events, mode, blocks, lds, st, P);
    switch (npad) {
    case 4: return launch_step_4(dm, events, mode, blocks, lds, st, P);
    case 8: return launch_step_8(dm, events, mode, blocks, lds, st, P);
    case 16: return launch_step_16(dm, events, mode, blocks, lds, st, P);
    case 32: return launch_step_32(dm, events, mode, blocks, lds, st, P);
    case 64: return launch_step_64(dm, events, mode, blocks, lds, st, P);
    case 128: return launch_step_128(dm, events, mode, e->wide_wv4, blocks, lds, st, P);
    case 256: return launch_step_256(dm, events, mode, e->wide_wv4, blocks, lds, st, P);
    default: return BRC_E_INVALID;
    }
}

static void free_all(Engine* e) {
    void* ps[] = {e->cells, e->meta, e->mgen, e->kdst, e->act, e->actany, e->items, e->inst, e->istats,
                  e->cons0, e->cons1, e->hmask, e->inj, e->inj_off, e->inj_cnt, e->byz, e->prop, e->events,
                  e->event_count, e->gcount, e->dbits, e->dring, e->lmeta, e->xsend, e->xsn, e->dparams};
    for (void* p : ps) if (p) (void)hipFree(p);
    if (e->ev0) (void)hipEventDestroy(e->ev0);
    if (e->ev1) (void)hipEventDestroy(e->ev1);
    if (e->stream) (void)hipStreamDestroy(e->stream);
}

static int fill_cells(Engine* e) {
    const uint64_t cells = e->cells_n;
    const uint64_t fb = std::min<uint64_t>((cells + 255) / 256, 1u << 20);
    if (e->compact)
        hipLaunchKernelGGL(fill_words<uint32_t>, dim3((uint32_t)fb), dim3(256), 0, e->stream, (uint32_t*)e->cells,
                           C32_FRESH, (uint64_t)cells);
    else
        hipLaunchKernelGGL(fill_words<uint64_t>, dim3((uint32_t)fb), dim3(256), 0, e->stream, e->cells, TIMES_NEVER,
                           (uint64_t)cells);
    HIPCHK(e, hipGetLastError());
    return BRC_OK;
}

// the step kernel's cells, allocated at its first launch on an engine the lifetime kernel may serve
static int ensure_cells(Engine* e) {
    if (e->cells_ready) return BRC_OK;
    const size_t bytes = e->cells_bytes;
    if (e->cells) (void)hipFree(e->cells);
    e->cells = nullptr;
    if (hipMalloc(&e->cells, std::max<size_t>(bytes, 8)) != hipSuccess) {
        (void)hipGetLastError();
        e->err = "device allocation of " + std::to_string(bytes) + " B of step-kernel cells failed";
        return BRC_E_NOMEM;
    }
    e->cells_ready = true;
    return fill_cells(e);
}

static int clear_state(Engine* e, bool full) {
    if (!e->step_ok) {
        // lifetime kernel only: it keeps key slots in LDS; no cells, key metadata or activity ring
    } else if (full) {
        if (e->cells_ready) {
            const int rc = fill_cells(e);
            if (rc) return rc;
        }
        HIPCHK(e, hipMemsetAsync(e->meta, 0, e->meta_bytes, e->stream));
        HIPCHK(e, hipMemsetAsync(e->mgen, 0, e->mgen_bytes, e->stream));
        e->book.full_clear();
    } else {
        hipLaunchKernelGGL(reset_slots, dim3((uint32_t)((e->keys + 255) / 256)), dim3(256), 0, e->stream, e->meta, e->mgen,
                           e->keys);
        HIPCHK(e, hipGetLastError());
    }
    if (e->step_ok) HIPCHK(e, hipMemsetAsync(e->act, 0, e->act_bytes, e->stream));
    HIPCHK(e, hipMemsetAsync(e->actany, 0, e->item_u32_bytes, e->stream));
    HIPCHK(e, hipMemsetAsync(e->items, 0, e->items_bytes, e->stream));
    HIPCHK(e, hipMemsetAsync(e->inst, 0, e->inst_bytes, e->stream));
    HIPCHK(e, hipMemsetAsync(e->istats, 0, e->istats_bytes, e->stream));
    HIPCHK(e, hipMemsetAsync(e->cons0, 0, e->cons_rec_bytes, e->stream));
    HIPCHK(e, hipMemsetAsync(e->cons1, 0, e->cons_rec_bytes, e->stream));
    if (e->cons_bytes) HIPCHK(e, hipMemsetAsync(e->hmask, 0, e->hmask_bytes, e->stream));
    HIPCHK(e, hipMemsetAsync(e->gcount, 0, 8 * 8, e->stream));
    if (e->has_xsn) HIPCHK(e, hipMemsetAsync(e->xsn, 0, e->xsn_bytes, e->stream));
    if (e->event_count) HIPCHK(e, hipMemsetAsync(e->event_count, 0, 8, e->stream));
    return BRC_OK;
}

static int upload_injections(Engine* e) {
    if (!e->inj_dirty) return BRC_OK;
    std::vector<ItemState> its(e->nitems);
    HIPCHK(e, hipMemcpyAsync(its.data(), e->items, e->nitems * sizeof(ItemState), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    size_t total = 0;
    std::vector<uint32_t> off(e->nitems), cnt(e->nitems);
    for (uint64_t i = 0; i < e->nitems; ++i) {
        auto& v = e->pending[i];
        const size_t consumed = std::min<size_t>(its[i].inj_pos, v.size());   // part of the last upload
        v.erase(v.begin(), v.begin() + consumed);
        std::stable_sort(v.begin(), v.end(), [](const InjDev& a, const InjDev& b) { return a.t < b.t; });
        off[i] = (uint32_t)total; cnt[i] = (uint32_t)v.size();
        total += v.size();
        its[i].inj_pos = 0;
    }
    if (total > e->inj_capacity) {
        if (e->inj) (void)hipFree(e->inj);
        e->inj = nullptr;
        HIPCHK(e, hipMalloc(&e->inj, std::max<size_t>(total, 1) * sizeof(InjDev)));
        e->inj_capacity = total;
    }
    std::vector<InjDev> flat;
    flat.reserve(total);
    for (auto& v : e->pending) flat.insert(flat.end(), v.begin(), v.end());
    if (total) HIPCHK(e, hipMemcpyAsync(e->inj, flat.data(), total * sizeof(InjDev), hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(e->inj_off, off.data(), e->nitems * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(e->inj_cnt, cnt.data(), e->nitems * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(e->items, its.data(), e->nitems * sizeof(ItemState), hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->inj_dirty = false;
    return BRC_OK;
}

static int apply_pattern(Engine* e) {
    if (e->cfg.byz_pattern != BRC_BYZ_EQUIVOCATE) return BRC_OK;
    // BRC_FLAG_LIFE_PATTERN: the wide key-lifetime kernel reads the Byzantine mask itself, no injection list
    if (e->cfg.flags & BRC_FLAG_LIFE_PATTERN) return BRC_OK;
    const uint32_t cap = (uint32_t)e->ipw * 6u * e->cfg.n;   // worst case: every replica Byzantine
    const size_t total = (size_t)e->nitems * cap;
    if (total > e->inj_capacity) {
        if (e->inj) (void)hipFree(e->inj);
        e->inj = nullptr;
        HIPCHK(e, hipMalloc(&e->inj, total * sizeof(InjDev)));
        e->inj_capacity = total;
    }
    const uint32_t blocks = (uint32_t)((e->nitems + 127) / 128);
    hipLaunchKernelGGL(expand_equivocate, dim3(blocks), dim3(128), 0, e->stream, e->inj, e->inj_off, e->inj_cnt,
                       e->byz, e->cfg.instances, e->nitems, (uint32_t)e->ipw, e->cfg.n, e->cfg.variants,
                       e->cfg.key_window, cap, e->bw);
    HIPCHK(e, hipGetLastError());
    e->pattern_active = true;
    return BRC_OK;
}

}  // namespace

extern "C" {

int brc_abi_version(void) { return BRC_ABI_VERSION; }

int brc_device_count(int* count) {
    if (!count) return BRC_E_INVALID;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
    *count = c;
    return BRC_OK;
}

const char* brc_last_error(void* h) {
    if (!h) return g_create_err.c_str();   // why the last brc_create on this thread failed
    return static_cast<Engine*>(h)->err.c_str();
}

int brc_create(const brc_config* cfg, void** out) {
    g_create_err.clear();
    if (!cfg || !out) { g_create_err = "null argument"; return BRC_E_INVALID; }
    *out = nullptr;
    const brc_config& c = *cfg;
    PlanEnv env;
    env.kernel = getenv("BRC_KERNEL");
    env.total_mem = [](void*, int device, uint64_t* bytes) {
        if (hipSetDevice(device) != hipSuccess) return false;
        size_t fr = 0, tot = 0;
        const bool ok = hipMemGetInfo(&fr, &tot) == hipSuccess;
        (void)hipGetLastError();
        *bytes = tot;
        return ok;
    };
    Plan plan;
    if (make_plan(c, env, &plan, &g_create_err) != BRC_OK) return BRC_E_INVALID;
    Engine* e = new Engine();
    static_cast<Plan&>(*e) = plan;
    e->cfg = c;
    auto fail = [&](int code) {
        g_create_err = e->err.empty() ? std::string("brc_create: HIP call failed: ") + hipGetErrorString(hipGetLastError())
                                      : e->err;
        free_all(e); delete e; return code;
    };
    if (hipSetDevice(c.device) != hipSuccess) { g_create_err = "hipSetDevice failed"; delete e; return BRC_E_HIP; }
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) return fail(BRC_E_HIP);
    if (hipEventCreate(&e->ev0) != hipSuccess || hipEventCreate(&e->ev1) != hipSuccess) return fail(BRC_E_HIP);
    struct A { void** p; size_t bytes; } allocs[] = {
        {(void**)&e->cells, e->cells_up_front ? e->cells_bytes : 8}, {(void**)&e->meta, e->meta_bytes},
        {(void**)&e->mgen, e->mgen_bytes}, {(void**)&e->kdst, e->kdst_bytes}, {(void**)&e->act, e->act_bytes},
        {(void**)&e->actany, e->item_u32_bytes}, {(void**)&e->items, e->items_bytes}, {(void**)&e->inst, e->inst_bytes},
        {(void**)&e->istats, e->istats_bytes}, {(void**)&e->cons0, e->cons_rec_bytes}, {(void**)&e->cons1, e->cons_rec_bytes},
        {&e->hmask, e->hmask_bytes}, {(void**)&e->inj_off, e->item_u32_bytes}, {(void**)&e->inj_cnt, e->item_u32_bytes},
        {(void**)&e->byz, e->byz_bytes}, {(void**)&e->gcount, 64}, {(void**)&e->dparams, sizeof(Params)},
        {(void**)&e->dbits, e->dbits_bytes}, {(void**)&e->dring, e->dring_bytes}, {(void**)&e->lmeta, e->lmeta_bytes},
        {(void**)&e->xsend, e->xsend_bytes}, {(void**)&e->xsn, e->xsn_bytes},
    };
    for (auto& a : allocs)
        if (hipMalloc(a.p, std::max<size_t>(a.bytes, 8)) != hipSuccess) {
            e->err = "device allocation of " + std::to_string(a.bytes) + " B failed";
            return fail(BRC_E_NOMEM);
        }
    if (c.event_capacity) {
        if (hipMalloc(&e->events, (size_t)c.event_capacity * sizeof(brc_event)) != hipSuccess) return fail(BRC_E_NOMEM);
        if (hipMalloc(&e->event_count, 8) != hipSuccess) return fail(BRC_E_NOMEM);
    }
    e->cells_ready = e->cells_up_front;
    e->last_life = e->life_cfg;       // brc_last_kernel before the first run: the kernel a fresh run launches
    if (hipMemsetAsync(e->inj_off, 0, e->item_u32_bytes, e->stream) != hipSuccess) return fail(BRC_E_HIP);
    if (hipMemsetAsync(e->inj_cnt, 0, e->item_u32_bytes, e->stream) != hipSuccess) return fail(BRC_E_HIP);
    if (hipMemsetAsync(e->kdst, 0, e->kdst_bytes, e->stream) != hipSuccess) return fail(BRC_E_HIP);
    // the lifetime kernel leaves its bitmap ring zero at exit
    if (e->has_dring && hipMemsetAsync(e->dring, 0, e->dring_bytes, e->stream) != hipSuccess) return fail(BRC_E_HIP);
    {
        std::vector<uint64_t> bm((size_t)c.instances * e->bw);
        for (uint64_t i = 0; i < c.instances; ++i)
            for (uint32_t w = 0; w < e->bw; ++w)
                bm[i * e->bw + w] = (w == 0 ? c.byzantine_mask : c.byzantine_mask_hi[w - 1]) & word_mask(c.n, w);
        if (hipMemcpy(e->byz, bm.data(), bm.size() * 8, hipMemcpyHostToDevice) != hipSuccess) return fail(BRC_E_HIP);
        e->hbyz = bm;
    }
    if (clear_state(e, true) != BRC_OK) return fail(BRC_E_HIP);
    e->pending.assign(e->nitems, {});
    if (apply_pattern(e) != BRC_OK) return fail(BRC_E_HIP);
    if (hipStreamSynchronize(e->stream) != hipSuccess) return fail(BRC_E_HIP);
    *out = e;
    return BRC_OK;
}

int brc_load_proposals(void* h, const int8_t* proposals) {
    Engine* e = static_cast<Engine*>(h);
    if (!e || !proposals) return BRC_E_INVALID;
    if (e->cfg.proposals != BRC_PROPOSALS_LOADED) return BRC_E_STATE;
    const size_t bytes = e->cfg.instances * e->cfg.n;
    const int vmax = e->cfg.mode == BRC_MODE_SPEC ? 3 : (int)e->nval - 1;
    bool wide_ids = false;
    for (size_t i = 0; i < bytes; ++i) {
        if (proposals[i] < 0 || proposals[i] > vmax) {
            e->err = "proposal value ids must be in [0, " + std::to_string(vmax) + "] on this kernel" +
                     ((e->wide && !e->wide_val && e->cfg.mode != BRC_MODE_SPEC && e->cfg.peer_mode == BRC_PEER_SENDER)
                          ? " (ids 4..7 at n > 64: create the engine with BRC_FLAG_WIDE_VALUES)" : "");
            return BRC_E_INVALID;
        }
        wide_ids = wide_ids || proposals[i] > 3;
    }
    // the lifetime kernels keep 2-bit value ids, but for the wide one under BRC_FLAG_LIFE_VALUES
    e->values_wide = wide_ids && !e->life_val;
    if (!e->prop) HIPCHK(e, hipMalloc(&e->prop, bytes));
    HIPCHK(e, hipMemcpyAsync(e->prop, proposals, bytes, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return BRC_OK;
}

int brc_load_byzantine(void* h, const uint64_t* masks) {
    Engine* e = static_cast<Engine*>(h);
    if (!e || !masks) return BRC_E_INVALID;
    const uint32_t words = (e->cfg.n + 63) / 64;
    std::vector<uint64_t> bm((size_t)e->cfg.instances * e->bw, 0);
    for (uint64_t i = 0; i < e->cfg.instances; ++i)
        for (uint32_t w = 0; w < words; ++w) bm[i * e->bw + w] = masks[i * words + w] & word_mask(e->cfg.n, w);
    HIPCHK(e, hipMemcpyAsync(e->byz, bm.data(), bm.size() * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->hbyz = bm;
    if (e->cfg.byz_pattern) { int rc = apply_pattern(e); if (rc) return rc; }
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return BRC_OK;
}

// Everything brc_inject decides is stage_injections' (brc_inject.h); what is left is the device's part
int brc_inject(void* h, const brc_injection* list, size_t count) {
    Engine* e = static_cast<Engine*>(h);
    if (!e || (!list && count)) return BRC_E_INVALID;
    auto fetch = [e](std::vector<ItemState>& its, std::vector<InstState>& ist) -> int {
        its.resize(e->nitems); ist.resize(e->cfg.instances);
        HIPCHK(e, hipMemcpyAsync(its.data(), e->items, e->nitems * sizeof(ItemState), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(e, hipMemcpyAsync(ist.data(), e->inst, e->cfg.instances * sizeof(InstState), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(e, hipStreamSynchronize(e->stream));
        return BRC_OK;
    };
    InjectBatch b;
    const int rc = stage_injections(*e, e->cfg, e->book, e->hbyz, e->pattern_active, e->life_done, list, count, fetch, &b,
                                    &e->err);
    if (rc) return rc;
    const size_t words = (e->wide_rec ? WREC_W : 3) * XSEND_MAX;
    for (const auto& tb : b.tables) {
        HIPCHK(e, hipMemcpyAsync(e->xsend + tb.item * words, tb.words.data(), words * 8, hipMemcpyHostToDevice, e->stream));
        HIPCHK(e, hipMemcpyAsync(e->xsn + tb.item, &tb.count, 4, hipMemcpyHostToDevice, e->stream));
    }
    for (size_t i = 0; i < b.staged.size(); ++i) e->pending[b.staged_item[i]].push_back(b.staged[i]);
    for (const auto& ro : b.reopen)
        HIPCHK(e, hipMemcpyAsync(&e->inst[ro.first], &ro.second, sizeof(InstState), hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->book.commit(*e, e->cfg, b);
    if (count) e->inj_dirty = true;   // (also when nothing was staged: a repeated SEND with no link left)
    return BRC_OK;
}

int brc_run(void* h, uint32_t max_steps, uint32_t* running_left) {
    Engine* e = static_cast<Engine*>(h);
    if (!e) return BRC_E_INVALID;
    const brc_config& c = e->cfg;
    HIPCHK(e, hipSetDevice(c.device));
    if (c.protocol == BRC_PROTO_CONSENSUS && c.proposals == BRC_PROPOSALS_LOADED && !e->prop) {
        e->err = "proposals not loaded";
        return BRC_E_STATE;
    }
    const bool genfree = e->compact || e->wide;    // no cell generation tags (rows rewritten at allocation)
    // (a fresh engine has consumed no record: the upload below leaves `pending` as it is, and an engine that is
    // not fresh never takes the lifetime kernel)
    bool no_inj = true;
    for (const auto& v : e->pending) if (!v.empty()) { no_inj = false; break; }
    const bool life = e->life_cfg && e->fresh && no_inj && max_steps == 0 && !e->values_wide;
    bool gen_clear = false;                        // the slot generation budget (brc_inject.h run_budget)
    if (!e->book.run_budget(c, e->fresh, genfree, life, &gen_clear, &e->err)) return BRC_E_STATE;
    int rc = upload_injections(e);
    if (rc) return rc;
    if (!life && !e->step_ok) { e->err = life_only_why(*e, true); return BRC_E_UNSUPPORTED; }
    if (!life) {
        rc = ensure_cells(e);
        if (rc) return rc;
    }
    if (gen_clear) {
        rc = fill_cells(e);
        if (rc) return rc;
        HIPCHK(e, hipMemsetAsync(e->mgen, 0, e->mgen_bytes, e->stream));
        e->book.full_clear();   // (a fresh engine: gen_cur is 0 already)
    }
    Params P;
    memset(&P, 0, sizeof(P));
    P.n = c.n; P.f = c.f; P.D = c.delay_max; P.Q = c.key_window; P.NV = c.variants; P.NK = e->NK; P.nkw = e->nkw;
    P.protocol = c.protocol; P.delay_model = c.delay_model; P.dconst = c.delay_const; P.round_cap = c.round_cap;
    P.step_cap = c.step_cap; P.proposals = c.proposals;
    P.T_echo = (c.n + c.f) / 2 + 1;     // len > (N+f)/2        core/brbroadcast.py:95
    P.T_amp = c.f + 1;                  // len > f              :118
    P.T_del = 2 * c.f + 1;              // len > 2f             :111
    P.T_cnt = c.n - c.f + 1;            // value_count > N-f    core/byzantinerandomizedconsensus.py:71,86
    P.bound_p1 = c.n + c.f;             // 2|hosts| > N+f       :73
    P.bound_p2 = 4 * c.f;               // 2|hosts| > 4f        :88
    P.seed = c.seed; P.inst_offset = c.instance_offset; P.instances = c.instances; P.nitems = e->nitems;
    P.max_steps = max_steps ? max_steps : 0xFFFFFFFFu;
    P.nL = delay_values(c.delay_model, c.delay_max);
    P.event_cap = c.event_capacity;
    P.mode = c.mode; P.coin_seed = c.coin_seed;
    P.s_limit = e->book.s_limit(c, genfree, life);
    P.cells = e->cells; P.meta = e->meta; P.mgen = e->mgen; P.kdst = e->kdst;
    P.act = e->act; P.actany = e->actany; P.items = e->items;
    P.inst = e->inst; P.istats = e->istats; P.cons0 = e->cons0; P.cons1 = e->cons1; P.hmask = e->hmask;
    P.inj = e->inj; P.inj_off = e->inj_off; P.inj_cnt = e->inj_cnt; P.byz = e->byz; P.prop = e->prop;
    P.events = e->events; P.event_count = e->event_count; P.gcount = e->gcount; P.dbits = e->dbits;
    P.dring = e->dring; P.lmeta = e->lmeta; P.xsend = e->xsend; P.xsn = e->xsn;
    e->hparams = P;
    HIPCHK(e, hipMemcpyAsync(e->dparams, &e->hparams, sizeof(Params), hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemsetAsync(e->gcount + 6, 0, 8, e->stream));   // instances still running after this launch
    HIPCHK(e, hipEventRecord(e->ev0, e->stream));   // times the step kernel alone
    e->fresh = false;
    e->last_life = life;
    if (life) e->life_done = true;
    rc = launch_kernel(e, life, e->dparams);
    if (rc == BRC_E_INVALID) { e->err = "no kernel instantiation"; return rc; }
    if (rc) { e->err = std::string("step kernel launch: ") + hipGetErrorString(hipGetLastError()); return rc; }
    HIPCHK(e, hipEventRecord(e->ev1, e->stream));
    HIPCHK(e, hipEventSynchronize(e->ev1));
    HIPCHK(e, hipEventElapsedTime(&e->last_ms, e->ev0, e->ev1));
    unsigned long long gc[8];
    HIPCHK(e, hipMemcpy(gc, e->gcount, sizeof(gc), hipMemcpyDeviceToHost));
    if (!genfree && !life) e->book.note_run(c, gc[5]);   // gc[5]: max phase index
    if (running_left) *running_left = (uint32_t)gc[6];   // counted by the step kernel
    return BRC_OK;
}

int brc_reset(void* h) {
    Engine* e = static_cast<Engine*>(h);
    if (!e) return BRC_E_INVALID;
    HIPCHK(e, hipSetDevice(e->cfg.device));
    const bool full = e->book.close_epoch();
    int rc = clear_state(e, full);   // full: book.full_clear()
    if (rc) return rc;
    for (auto& v : e->pending) v.clear();
    e->book.clear_epoch();
    if (e->pattern_active) {
        e->pattern_active = false;
        rc = apply_pattern(e);
        if (rc) return rc;
    } else {
        HIPCHK(e, hipMemsetAsync(e->inj_off, 0, (size_t)e->nitems * 4, e->stream));
        HIPCHK(e, hipMemsetAsync(e->inj_cnt, 0, (size_t)e->nitems * 4, e->stream));
    }
    e->inj_dirty = false;
    e->fresh = true;
    e->life_done = false;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return BRC_OK;
}

int brc_read_instances(void* h, uint64_t first, uint64_t count, brc_instance_result* out) {
    Engine* e = static_cast<Engine*>(h);
    if (!e || !out || first + count > e->cfg.instances) return BRC_E_INVALID;
    if (!count) return BRC_OK;
    const brc_config& c = e->cfg;
    std::vector<InstState> ist(count);
    std::vector<uint64_t> st(count * 4);
    HIPCHK(e, hipMemcpyAsync(ist.data(), e->inst + first, count * sizeof(InstState), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(st.data(), e->istats + first * 4, count * 32, hipMemcpyDeviceToHost, e->stream));
    const uint64_t i0 = first / e->ipw, i1 = (first + count - 1) / e->ipw;
    std::vector<ItemState> its(i1 - i0 + 1);
    HIPCHK(e, hipMemcpyAsync(its.data(), e->items + i0, its.size() * sizeof(ItemState), hipMemcpyDeviceToHost, e->stream));
    std::vector<uint64_t> c1((i1 - i0 + 1) * e->lpi);
    std::vector<uint64_t> bm(count * e->bw);
    HIPCHK(e, hipMemcpyAsync(bm.data(), e->byz + first * e->bw, bm.size() * 8, hipMemcpyDeviceToHost, e->stream));
    if (c.protocol == BRC_PROTO_CONSENSUS)
        HIPCHK(e, hipMemcpyAsync(c1.data(), e->cons1 + i0 * e->lpi, c1.size() * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    for (uint64_t i = 0; i < count; ++i) {
        const uint64_t in = first + i, item = in / e->ipw, seg = in % e->ipw;
        brc_instance_result& r = out[i];
        r.status = ist[i].status; r.t_stop = ist[i].t_stop; r.t_now = its[item - i0].t;
        r.msgs_sent = st[i * 4 + 0]; r.arrivals = st[i * 4 + 1]; r.cell_steps = st[i * 4 + 2]; r.deliveries = st[i * 4 + 3];
        uint32_t dec = c.protocol == BRC_PROTO_CONSENSUS ? 1u : 0u;
        if (dec)
            for (uint32_t dd = 0; dd < c.n; ++dd) {
                if ((bm[i * e->bw + dd / 64] >> (dd % 64)) & 1ull) continue;
                if ((c1[(item - i0) * e->lpi + seg * e->npad + dd] & 0xFFFF) == 0) { dec = 0; break; }
            }
        r.decided = dec;
    }
    return BRC_OK;
}

int brc_read_replicas(void* h, uint64_t first, uint64_t count, brc_replica_result* out) {
    Engine* e = static_cast<Engine*>(h);
    if (!e || !out || first + count > e->cfg.instances) return BRC_E_INVALID;
    if (!count) return BRC_OK;
    const uint64_t i0 = first / e->ipw, i1 = (first + count - 1) / e->ipw;
    const size_t nl = (i1 - i0 + 1) * e->lpi;
    std::vector<uint64_t> c0(nl), c1(nl);
    HIPCHK(e, hipMemcpyAsync(c0.data(), e->cons0 + i0 * e->lpi, nl * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(c1.data(), e->cons1 + i0 * e->lpi, nl * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    for (uint64_t i = 0; i < count; ++i) {
        const uint64_t in = first + i, item = in / e->ipw, seg = in % e->ipw;
        for (uint32_t dd = 0; dd < e->cfg.n; ++dd) {
            const size_t l = (item - i0) * e->lpi + seg * e->npad + dd;
            brc_replica_result& r = out[i * e->cfg.n + dd];
            const uint64_t a = c0[l], b = c1[l];
            r.round = a & 0xFFFF; r.phase = (a >> 16) & 0xF; r.value_count = (a >> 48) & 0xFFFF;   // cons0_pack
            r.decide_count = b & 0xFFFF; r.first_decide_round = (b >> 16) & 0xFFFF;
            r.first_decide_t = (b >> 32) & 0xFFFF;
            r.first_decide_value = r.decide_count ? (int32_t)((b >> 48) & 0xFF) : -1;
            r.last_decide_value = r.decide_count ? (int32_t)((b >> 56) & 0xFF) : -1;
        }
    }
    return BRC_OK;
}

int brc_read_events(void* h, brc_event* out, size_t cap, size_t* count) {
    Engine* e = static_cast<Engine*>(h);
    if (!e || !count) return BRC_E_INVALID;
    if (!e->event_count) { *count = 0; return BRC_OK; }
    unsigned long long n = 0;
    HIPCHK(e, hipMemcpy(&n, e->event_count, 8, hipMemcpyDeviceToHost));
    *count = (size_t)n;
    const size_t avail = std::min<size_t>((size_t)n, e->cfg.event_capacity);
    if (out && cap) HIPCHK(e, hipMemcpy(out, e->events, std::min(avail, cap) * sizeof(brc_event), hipMemcpyDeviceToHost));
    return BRC_OK;
}

int brc_read_stats(void* h, brc_stats* out) {
    Engine* e = static_cast<Engine*>(h);
    if (!e || !out) return BRC_E_INVALID;
    memset(out, 0, sizeof(*out));
    const uint64_t N = e->cfg.instances;
    std::vector<brc_instance_result> r(N);
    int rc = brc_read_instances(h, 0, N, r.data());
    if (rc) return rc;
    out->instances = N;
    for (auto& x : r) {
        out->running += x.status == BRC_RUNNING;
        out->done += x.status == BRC_DONE;
        out->quiescent += x.status == BRC_QUIESCENT;
        out->stepcap += x.status == BRC_STEPCAP;
        out->overflow += x.status == BRC_OVERFLOW || x.status == BRC_BADINJ;
        out->decided += x.decided;
        out->msgs_sent += x.msgs_sent; out->arrivals += x.arrivals; out->cell_steps += x.cell_steps;
        out->deliveries += x.deliveries;
        out->max_t = std::max<uint64_t>(out->max_t, x.t_now);
    }
    unsigned long long gc[8] = {0};
    HIPCHK(e, hipMemcpy(gc, e->gcount, 64, hipMemcpyDeviceToHost));
    out->lane_loads = gc[4];
    if (e->cfg.protocol == BRC_PROTO_CONSENSUS) {
        std::vector<uint64_t> c1((size_t)e->nitems * e->lpi);
        std::vector<uint64_t> bm(N * e->bw);
        HIPCHK(e, hipMemcpy(c1.data(), e->cons1, c1.size() * 8, hipMemcpyDeviceToHost));
        HIPCHK(e, hipMemcpy(bm.data(), e->byz, bm.size() * 8, hipMemcpyDeviceToHost));
        for (uint64_t in = 0; in < N; ++in) {
            const uint64_t item = in / e->ipw, seg = in % e->ipw;
            for (uint32_t dd = 0; dd < e->cfg.n; ++dd)
                if (!((bm[in * e->bw + dd / 64] >> (dd % 64)) & 1ull))
                    out->decide_rounds_sum += (c1[item * e->lpi + seg * e->npad + dd] >> 16) & 0xFFFF;
        }
    }
    if (e->event_count) {
        unsigned long long n = 0;
        HIPCHK(e, hipMemcpy(&n, e->event_count, 8, hipMemcpyDeviceToHost));
        out->events_dropped = n > e->cfg.event_capacity ? n - e->cfg.event_capacity : 0;
    }
    return BRC_OK;
}

int brc_read_round_histogram(void* h, uint64_t* hist, uint32_t bins) {
    Engine* e = static_cast<Engine*>(h);
    if (!e || !hist || bins < 2 || bins > 4096) return BRC_E_INVALID;
    if (e->cfg.protocol != BRC_PROTO_CONSENSUS) { e->err = "round histogram needs the consensus protocol"; return BRC_E_STATE; }
    HIPCHK(e, hipSetDevice(e->cfg.device));
    unsigned long long* dh = nullptr;
    HIPCHK(e, hipMalloc(&dh, (size_t)bins * 8));
    if (hipMemsetAsync(dh, 0, (size_t)bins * 8, e->stream) != hipSuccess) { (void)hipFree(dh); return BRC_E_HIP; }
    const uint32_t tpb = 256;
    const uint32_t blocks = (uint32_t)((e->cfg.instances + tpb - 1) / tpb);
    hipLaunchKernelGGL(round_histogram, dim3(blocks), dim3(tpb), (size_t)bins * 8, e->stream, e->cons1, e->byz,
                       e->cfg.instances, (uint32_t)e->ipw, e->lpi, (uint32_t)e->npad, e->bw, e->cfg.n, bins, dh);
    hipError_t r = hipGetLastError();
    if (r == hipSuccess) r = hipMemcpyAsync(hist, dh, (size_t)bins * 8, hipMemcpyDeviceToHost, e->stream);
    if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
    (void)hipFree(dh);
    if (r != hipSuccess) { e->err = std::string("round histogram: ") + hipGetErrorString(r); return BRC_E_HIP; }
    return BRC_OK;
}

int brc_read_value_decisions(void* h, uint64_t* value_hist, uint64_t* disagreements) {
    Engine* e = static_cast<Engine*>(h);
    if (!e || !value_hist || !disagreements) return BRC_E_INVALID;
    if (e->cfg.protocol != BRC_PROTO_CONSENSUS) { e->err = "decisions need the consensus protocol"; return BRC_E_STATE; }
    HIPCHK(e, hipSetDevice(e->cfg.device));
    unsigned long long* d = nullptr;
    HIPCHK(e, hipMalloc(&d, 10 * 8));
    hipError_t r = hipMemsetAsync(d, 0, 10 * 8, e->stream);
    if (r == hipSuccess) {
        const uint32_t tpb = 256;
        const uint32_t blocks = (uint32_t)((e->cfg.instances + tpb - 1) / tpb);
        hipLaunchKernelGGL(decision_histogram, dim3(blocks), dim3(tpb), 0, e->stream, e->cons1, e->byz,
                           e->cfg.instances, (uint32_t)e->ipw, e->lpi, (uint32_t)e->npad, e->bw, e->cfg.n, d);
        r = hipGetLastError();
    }
    unsigned long long hout[10] = {0};
    if (r == hipSuccess) r = hipMemcpyAsync(hout, d, sizeof(hout), hipMemcpyDeviceToHost, e->stream);
    if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
    (void)hipFree(d);
    if (r != hipSuccess) { e->err = std::string("decision histogram: ") + hipGetErrorString(r); return BRC_E_HIP; }
    for (int b = 0; b < 9; ++b) value_hist[b] = hout[b];
    *disagreements = hout[9];
    return BRC_OK;
}

int brc_read_decisions(void* h, uint64_t* value_hist, uint64_t* disagreements) {
    Engine* e = static_cast<Engine*>(h);
    if (!e || !value_hist || !disagreements) return BRC_E_INVALID;
    uint64_t v9[9];
    const int rc = brc_read_value_decisions(h, v9, disagreements);
    if (rc) return rc;
    for (int b = 4; b < 8; ++b)
        if (v9[b]) { e->err = "value ids >= 4 were decided: use brc_read_value_decisions"; return BRC_E_STATE; }
    for (int b = 0; b < 4; ++b) value_hist[b] = v9[b];
    value_hist[4] = v9[8];
    return BRC_OK;
}

int brc_reset_at(void* h, uint64_t instance_offset) {
    Engine* e = static_cast<Engine*>(h);
    if (!e) return BRC_E_INVALID;
    e->cfg.instance_offset = instance_offset;
    return brc_reset(h);
}

int brc_read_events_range(void* h, size_t first, brc_event* out, size_t cap, size_t* total) {
    Engine* e = static_cast<Engine*>(h);
    if (!e || !total) return BRC_E_INVALID;
    if (!e->event_count) { *total = 0; return BRC_OK; }
    unsigned long long n = 0;
    HIPCHK(e, hipMemcpy(&n, e->event_count, 8, hipMemcpyDeviceToHost));
    *total = (size_t)n;
    const size_t avail = std::min<size_t>((size_t)n, e->cfg.event_capacity);
    if (out && cap && first < avail)
        HIPCHK(e, hipMemcpy(out, e->events + first, std::min(avail - first, cap) * sizeof(brc_event),
                            hipMemcpyDeviceToHost));
    return BRC_OK;
}

int brc_last_kernel(void* h, uint32_t* kind) {
    Engine* e = static_cast<Engine*>(h);
    if (!e || !kind) return BRC_E_INVALID;
    *kind = e->last_life ? BRC_KERNEL_LIFE : BRC_KERNEL_STEP;
    return BRC_OK;
}

int brc_last_kernel_ms(void* h, float* ms) {
    Engine* e = static_cast<Engine*>(h);
    if (!e || !ms) return BRC_E_INVALID;
    *ms = e->last_ms;
    return BRC_OK;
}

void brc_destroy(void* h) {
    Engine* e = static_cast<Engine*>(h);
    if (!e) return;
    (void)hipSetDevice(e->cfg.device);
    (void)hipStreamSynchronize(e->stream);
    free_all(e);
    delete e;
}

}  // extern "C"
