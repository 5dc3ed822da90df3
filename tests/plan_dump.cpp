// plan_dump.cpp -- walks a fixed grid of engine configurations through the planner (csrc/brc_plan.h) and prints, per
// configuration, a "C" line (the configuration, the BRC_KERNEL value, the device memory) and then either an "R" line
// (the refusal: rc and reason) or a "P" line (every field of the plan).  A plain host program: it needs no HIP header,
// and tests/test_plan.py builds it with the host compiler under the address and undefined-behaviour sanitizers.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include "../byzantinerandomizedconsensus_amd/csrc/brc_plan.h"

using namespace brc;

namespace {

struct Mem { bool known; uint64_t total; int asked; };
bool mem_query(void* ctx, int, uint64_t* bytes) {
    Mem* m = static_cast<Mem*>(ctx);
    ++m->asked;
    *bytes = m->total;
    return m->known;
}

const uint32_t NS[] = {1, 4, 5, 8, 9, 32, 33, 64, 65, 128, 129, 256};
const uint32_t FLAGS[] = {0, BRC_FLAG_GENERAL_KEYS, BRC_FLAG_WIDE_RECORDS, BRC_FLAG_WIDE_VALUES, BRC_FLAG_WIDE_WINDOWS,
                          BRC_FLAG_WIDE_LIFE, BRC_FLAG_LIFE_PATTERN, BRC_FLAG_WIDE_LIFE | BRC_FLAG_LIFE_PATTERN,
                          BRC_FLAG_WIDE_LIFE | BRC_FLAG_WIDE_RECORDS, BRC_FLAG_WIDE_RECORDS | BRC_FLAG_WIDE_VALUES,
                          BRC_FLAG_WIDE_WINDOWS | BRC_FLAG_WIDE_VALUES, 64 /* unknown */,
                          // the wide key-lifetime kernel at windows of 16 / 32
                          BRC_FLAG_WIDE_LIFE | BRC_FLAG_WIDE_WINDOWS,
                          BRC_FLAG_WIDE_LIFE | BRC_FLAG_LIFE_PATTERN | BRC_FLAG_WIDE_WINDOWS};
const char* const ENVS[] = {nullptr, "step", "life"};
const uint32_t DMAX[] = {1, 4, 8, 9, 16};
const uint32_t QS[] = {2, 8, 16, 32, 64, 128};
const uint32_t NVS[] = {1, 2, 4};

brc_config base_config(uint32_t n, uint32_t protocol, uint32_t mode, uint32_t peer, uint32_t model, uint32_t dmax,
                       uint32_t q, uint32_t nv, uint32_t proposals, uint32_t flags = 0, uint32_t byz = BRC_BYZ_NONE) {
    brc_config c = {};
    c.n = n; c.f = (n - 1) / 3; c.protocol = protocol; c.mode = mode; c.peer_mode = peer;
    c.instances = 5; c.seed = 1; c.delay_model = model; c.delay_max = dmax; c.delay_const = 1;
    c.round_cap = 1; c.step_cap = 4000; c.key_window = q; c.variants = nv; c.proposals = proposals;
    c.byz_pattern = byz; c.flags = flags;
    return c;
}

size_t emitted = 0;

// one configuration: its lines, and the plan's step_state_bytes (0 on refusal) for the memory axis
uint64_t emit(const brc_config& c, const char* kernel, bool mem_known = false, uint64_t mem_total = 0) {
    Mem mem = {mem_known, mem_total, 0};
    PlanEnv env;
    env.kernel = kernel;
    env.total_mem = mem_query;
    env.ctx = &mem;
    Plan p;
    std::string why;
    const int rc = make_plan(c, env, &p, &why);
    if (mem.asked > 1) { fprintf(stderr, "the planner asked for the device memory %d times\n", mem.asked); exit(2); }
    ++emitted;
    printf("C n=%u f=%u protocol=%u peer_mode=%u instances=%" PRIu64 " delay_model=%u delay_max=%u delay_const=%u "
           "step_cap=%u key_window=%u variants=%u proposals=%u byz_pattern=%u event_capacity=%u mode=%u flags=%u env=%s mem=",
           c.n, c.f, c.protocol, c.peer_mode, c.instances, c.delay_model, c.delay_max, c.delay_const, c.step_cap,
           c.key_window, c.variants, c.proposals, c.byz_pattern, c.event_capacity, c.mode, c.flags, kernel ? kernel : "-");
    if (mem_known) printf("%" PRIu64 "\n", mem_total); else printf("unknown\n");
    if (rc != BRC_OK) { printf("R rc=%d why=%s\n", rc, why.c_str()); return 0; }
    printf("P npad=%d dm=%d ipw=%d nkw_t=%d kmode=%d wide=%d wide_wv4=%d wide_rec=%d wide_val=%d regmask=%d compact=%d "
           "general=%d lpi=%u bw=%u NK=%u nkw=%u msize=%u lds_bytes=%u rows=%u rs=%u nval=%u cons_bytes=%" PRIu64
           " nitems=%" PRIu64 " life_cfg=%d life_pl=%d life_pat=%d life_rw=%u life_lds=%u step_ok=%d cells_up_front=%d "
           "has_dbits=%d has_dring=%d has_lmeta=%d has_xsn=%d keys=%" PRIu64 " cells_n=%" PRIu64 " step_state_bytes=%" PRIu64
           " cells_bytes=%" PRIu64 " meta_bytes=%" PRIu64 " mgen_bytes=%" PRIu64 " kdst_bytes=%" PRIu64 " act_bytes=%" PRIu64
           " items_bytes=%" PRIu64 " inst_bytes=%" PRIu64 " item_u32_bytes=%" PRIu64 " cons_rec_bytes=%" PRIu64
           " istats_bytes=%" PRIu64 " hmask_bytes=%" PRIu64 " byz_bytes=%" PRIu64 " dbits_bytes=%" PRIu64
           " dring_bytes=%" PRIu64 " lmeta_bytes=%" PRIu64 " xsend_bytes=%" PRIu64 " xsn_bytes=%" PRIu64 "\n",
           p.npad, p.dm, p.ipw, p.nkw_t, p.kmode, p.wide, p.wide_wv4, p.wide_rec, p.wide_val, p.regmask, p.compact,
           p.general, p.lpi, p.bw, p.NK, p.nkw, p.msize, p.lds_bytes, p.rows, p.rs, p.nval, p.cons_bytes, p.nitems,
           p.life_cfg, p.life_pl, p.life_pat, p.life_rw, p.life_lds, p.step_ok, p.cells_up_front, p.has_dbits, p.has_dring,
           p.has_lmeta, p.has_xsn, p.keys, p.cells_n, p.step_state_bytes, p.cells_bytes, p.meta_bytes, p.mgen_bytes,
           p.kdst_bytes, p.act_bytes, p.items_bytes, p.inst_bytes, p.item_u32_bytes, p.cons_rec_bytes, p.istats_bytes,
           p.hmask_bytes, p.byz_bytes, p.dbits_bytes, p.dring_bytes, p.lmeta_bytes, p.xsend_bytes, p.xsn_bytes);
    return p.step_state_bytes;
}

void emit_envs(const brc_config& c) { for (const char* k : ENVS) emit(c, k); }

// every value of each axis in turn around one configuration, and the key_window x variants plane
void sweep(const brc_config& b) {
    brc_config c;
    emit_envs(b);
    for (uint32_t n : NS) for (int ff = 0; ff < 2; ++ff) { c = b; c.n = n; c.f = ff ? (n - 1) / 3 : 0; emit(c, nullptr); }
    for (uint32_t v = 0; v <= BRC_MODE_BEB; ++v) { c = b; c.mode = v; emit(c, nullptr); }
    for (uint32_t v = 0; v <= BRC_PEER_CONNECTION; ++v) { c = b; c.peer_mode = v; emit(c, nullptr); }
    for (uint32_t v = 0; v <= BRC_PROTO_CONSENSUS; ++v) { c = b; c.protocol = v; emit(c, nullptr); }
    for (uint32_t m = 0; m <= BRC_DELAY_GEOMETRIC; ++m)
        for (uint32_t d : DMAX) { c = b; c.delay_model = m; c.delay_max = d; emit_envs(c); }
    for (uint32_t q : QS) for (uint32_t nv : NVS) { c = b; c.key_window = q; c.variants = nv; emit_envs(c); }
    for (uint32_t v = 0; v <= BRC_PROPOSALS_LOADED; ++v) { c = b; c.proposals = v; emit(c, nullptr); }
    for (uint32_t v = 0; v < 2; ++v) { c = b; c.event_capacity = v; emit_envs(c); }
    for (uint32_t v = 0; v <= BRC_BYZ_EQUIVOCATE; ++v) { c = b; c.byz_pattern = v; emit(c, nullptr); }
    for (uint32_t fl : FLAGS) { c = b; c.flags = fl; emit_envs(c); }
}

}  // namespace

int main() {
    const uint32_t CONS = BRC_PROTO_CONSENSUS, REF = BRC_MODE_REFERENCE, SPEC = BRC_MODE_SPEC, SND = BRC_PEER_SENDER,
                   CONN = BRC_PEER_CONNECTION, PHILOX = BRC_PROPOSALS_PHILOX;
    // 1. the cross product, thinned: every (n, flags, BRC_KERNEL) with three draws of the other axes (a fixed LCG)
    uint64_t lcg = 0x9E3779B97F4A7C15ull;
    auto draw = [&](uint32_t m) { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)((lcg >> 33) % m); };
    for (uint32_t n : NS)
        for (uint32_t fl : FLAGS)
            for (const char* k : ENVS)
                for (int rep = 0; rep < 3; ++rep) {
                    brc_config c = base_config(n, 0, 0, 0, 0, 1, 2, 1, 0, fl);     // (draws in statement order)
                    c.protocol = draw(2); c.mode = draw(3); c.peer_mode = draw(2); c.delay_model = draw(4);
                    c.delay_max = DMAX[draw(5)]; c.key_window = QS[draw(6)]; c.variants = NVS[draw(3)];
                    c.proposals = draw(2); c.byz_pattern = draw(2);
                    c.f = draw(2) ? (n - 1) / 3 : 0;
                    c.event_capacity = draw(2);
                    emit(c, k);
                }
    // 2. axis sweeps around one configuration of each kernel family
    const brc_config bases[] = {
        base_config(4, BRC_PROTO_BRB, REF, SND, BRC_DELAY_UNIFORM, 4, 8, 1, BRC_PROPOSALS_NONE),
        base_config(32, CONS, REF, SND, BRC_DELAY_SLOWSET, 8, 2, 2, PHILOX),
        base_config(64, CONS, REF, SND, BRC_DELAY_SLOWSET, 8, 8, 1, PHILOX),                       // lean, register masks
        base_config(64, CONS, SPEC, SND, BRC_DELAY_UNIFORM, 8, 8, 1, PHILOX),                      // lean, LDS masks
        base_config(64, CONS, REF, CONN, BRC_DELAY_SLOWSET, 8, 8, 1, PHILOX),
        base_config(33, CONS, REF, SND, BRC_DELAY_SLOWSET, 8, 8, 1, PHILOX, BRC_FLAG_GENERAL_KEYS),
        base_config(64, CONS, REF, SND, BRC_DELAY_SLOWSET, 8, 64, 1, PHILOX),                      // lifetime-only by window
        base_config(64, CONS, REF, CONN, BRC_DELAY_SLOWSET, 8, 128, 1, PHILOX),                    // ... by connection-peer LDS
        base_config(128, CONS, REF, SND, BRC_DELAY_SLOWSET, 8, 8, 1, PHILOX),                      // wide, 4 waves per SIMD
        base_config(129, CONS, REF, SND, BRC_DELAY_UNIFORM, 16, 16, 2, PHILOX, BRC_FLAG_WIDE_WINDOWS | BRC_FLAG_WIDE_VALUES),
        base_config(200, CONS, REF, SND, BRC_DELAY_CONST, 4, 8, 1, PHILOX, BRC_FLAG_WIDE_LIFE),
        base_config(256, CONS, REF, SND, BRC_DELAY_SLOWSET, 8, 4, 2, PHILOX, BRC_FLAG_WIDE_LIFE | BRC_FLAG_LIFE_PATTERN,
                    BRC_BYZ_EQUIVOCATE),
    };
    for (const brc_config& b : bases) sweep(b);
    // 3. the device-memory axis on the lean engines: 9 instances make the step state a multiple of 9, so that
    //    "state > total / 10 * 9" has an exact threshold.  Eligible for the lifetime kernel, per-link, and not eligible
    const brc_config lean[] = {
        base_config(64, CONS, REF, SND, BRC_DELAY_SLOWSET, 8, 8, 1, PHILOX),
        base_config(33, CONS, SPEC, SND, BRC_DELAY_GEOMETRIC, 16, 4, 2, PHILOX),
        base_config(64, BRC_PROTO_BRB, REF, SND, BRC_DELAY_SLOWSET, 8, 8, 1, BRC_PROPOSALS_NONE),
        base_config(64, CONS, BRC_MODE_BEB, SND, BRC_DELAY_CONST, 4, 32, 1, BRC_PROPOSALS_LOADED),
    };
    for (brc_config c : lean) {
        c.instances = 9;
        for (const char* k : ENVS) {
            const uint64_t need = emit(c, k);
            if (!need || need % 9) { fprintf(stderr, "memory axis: no exact threshold\n"); return 2; }
            const uint64_t at = need / 9 * 10;      // at / 10 * 9 == need: the state just fits
            for (uint64_t total : {at - 1, at, at + 1, at + 10, UINT64_MAX}) emit(c, k, true, total);
            emit(c, k, true, 0);
        }
    }
    // 4. single fields out of range, and the limits no sweep above reaches
    {
        const brc_config b = base_config(4, CONS, REF, SND, BRC_DELAY_CONST, 4, 4, 1, PHILOX);
        brc_config c;
        c = b; c.n = 0; emit(c, nullptr);
        c = b; c.n = 257; emit(c, nullptr);
        c = b; c.f = c.n; emit(c, nullptr);
        c = b; c.instances = 0; emit(c, nullptr);
        c = b; c.delay_max = 0; emit(c, nullptr);
        c = b; c.delay_max = 17; emit(c, nullptr);
        c = b; c.delay_const = 0; emit(c, nullptr);
        c = b; c.delay_const = 5; emit(c, nullptr);
        c = b; c.step_cap = STEP_LIMIT; emit(c, nullptr);
        c = b; c.step_cap = STEP_LIMIT + 1; emit(c, nullptr);
        c = b; c.peer_mode = 2; emit(c, nullptr);
        c = b; c.protocol = 2; emit(c, nullptr);
        c = b; c.delay_model = 4; emit(c, nullptr);
        c = b; c.key_window = 3; emit(c, nullptr);
        c = b; c.key_window = 256; emit(c, nullptr);
        c = b; c.variants = 3; emit(c, nullptr);
        c = b; c.proposals = 3; emit(c, nullptr);
        c = b; c.mode = 3; emit(c, nullptr);
        c = b; c.byz_pattern = 2; emit(c, nullptr);
        c = b; c.byz_pattern = BRC_BYZ_EQUIVOCATE; emit(c, nullptr);          // needs two variants
        // more wave items than a launch has workgroups
        // (connection peers: no device-memory question, so the library answers alike with and without a device)
        c = b; c.n = 64; c.peer_mode = CONN; c.instances = 0x7FFFFFFFull * WPB; emit(c, nullptr);
        c.instances = 0x7FFFFFFFull * WPB + 1; emit(c, nullptr);
        c = b; c.n = 200; c.instances = 0x80000000ull; emit(c, nullptr);
        // the one wide-window shape whose LDS carve exceeds 160 KB (include/brc.h), and its neighbours that fit
        c = base_config(256, CONS, REF, SND, BRC_DELAY_UNIFORM, 16, 32, 1, PHILOX, BRC_FLAG_WIDE_WINDOWS); emit(c, nullptr);
        c.key_window = 16; c.variants = 2; emit(c, nullptr);
        c.delay_max = 8; c.key_window = 32; c.variants = 1; emit(c, nullptr);
        c.mode = SPEC; c.key_window = 8; emit(c, nullptr);                    // the flag under SPEC
        c.flags = BRC_FLAG_WIDE_VALUES; emit(c, nullptr);
        // the lifetime kernel's forms at n in 33..64: key windows 32 (slot metadata in HBM), 64 and 128; delays above 8
        for (uint32_t q : {16u, 32u, 64u, 128u}) {
            c = base_config(64, CONS, REF, SND, BRC_DELAY_SLOWSET, 8, q, 1, PHILOX); emit_envs(c);
            c.peer_mode = CONN; emit_envs(c);
        }
        c = base_config(64, CONS, REF, CONN, BRC_DELAY_UNIFORM, 16, 8, 1, PHILOX); emit_envs(c);
        c = base_config(64, CONS, REF, SND, BRC_DELAY_GEOMETRIC, 16, 8, 1, PHILOX); emit_envs(c);
    }
    // 5. the fault bound's ends on every kernel family of tests/fault_bound_workloads.py: f = 0 and f = n - 1 run,
    //    f = n and f = n + 1 are refused by name
    for (uint32_t n : {1u, 2u, 3u, 4u, 33u, 64u, 65u, 256u}) {
        const uint32_t BEB = BRC_MODE_BEB, SLOW = BRC_DELAY_SLOWSET, UNIF = BRC_DELAY_UNIFORM;
        struct Fam { brc_config c; const char* env; };
        Fam fams[12];
        size_t nf = 0;
        if (n <= 32) {
            fams[nf++] = {base_config(n, BRC_PROTO_BRB, REF, SND, SLOW, 4, 8, 1, BRC_PROPOSALS_NONE), nullptr};
            for (uint32_t m : {REF, SPEC, BEB}) fams[nf++] = {base_config(n, CONS, m, SND, SLOW, 4, 8, 1, PHILOX), nullptr};
            fams[nf++] = {base_config(n, CONS, REF, CONN, UNIF, 4, 8, 1, PHILOX), nullptr};
        } else if (n <= 64) {
            for (uint32_t m : {REF, SPEC, BEB}) {
                fams[nf++] = {base_config(n, CONS, m, SND, SLOW, 8, 8, 1, PHILOX), "step"};     // lean
                fams[nf++] = {base_config(n, CONS, m, SND, SLOW, 8, 8, 1, PHILOX), "life"};     // two-class lifetime
            }
            fams[nf++] = {base_config(n, CONS, REF, SND, SLOW, 4, 8, 1, PHILOX, BRC_FLAG_GENERAL_KEYS), "step"};
            fams[nf++] = {base_config(n, CONS, REF, CONN, SLOW, 4, 8, 1, PHILOX), "step"};
            fams[nf++] = {base_config(n, CONS, REF, CONN, SLOW, 4, 8, 1, PHILOX), "life"};
            fams[nf++] = {base_config(n, CONS, SPEC, SND, UNIF, 12, 8, 1, PHILOX), "life"};     // per-link lifetime
            fams[nf++] = {base_config(n, CONS, REF, CONN, UNIF, 12, 8, 1, PHILOX), "life"};
        } else {
            for (uint32_t m : {REF, SPEC, BEB}) {
                fams[nf++] = {base_config(n, CONS, m, SND, SLOW, 8, 8, 1, PHILOX), nullptr};    // wide step
                fams[nf++] = {base_config(n, CONS, m, SND, SLOW, 8, 8, 1, PHILOX, BRC_FLAG_WIDE_LIFE), nullptr};
            }
            fams[nf++] = {base_config(n, CONS, REF, SND, SLOW, 8, 4, 2, PHILOX, BRC_FLAG_WIDE_RECORDS), nullptr};
            fams[nf++] = {base_config(n, CONS, REF, SND, SLOW, 8, 4, 2, PHILOX, BRC_FLAG_WIDE_LIFE | BRC_FLAG_LIFE_PATTERN,
                                      BRC_BYZ_EQUIVOCATE), nullptr};
        }
        for (size_t i = 0; i < nf; ++i)
            for (uint32_t f : {0u, n - 1, n, n + 1}) { brc_config c = fams[i].c; c.f = f; emit(c, fams[i].env); }
    }
    fprintf(stderr, "%zu configurations\n", emitted);
    return 0;
}
