// inject_dump.cpp -- drives scripted brc_inject batches through the staging function and the book of csrc/brc_inject.h,
// on engines planned by make_plan, with synthetic device state.  A plain host program: it needs no HIP header, and
// tests/test_inject.py (which writes the script) builds it with the host compiler under the address and
// undefined-behaviour sanitizers.  It does what brc_engine.hip does around the header, minus the device.
//
// Script on stdin, one command per line, numbers in any C base:
//   engine NAME n f protocol mode peer_mode delay_model delay_max key_window variants proposals byz_pattern flags
//          instances BRC_KERNEL|- byz0 byz1 byz2 byz3        plan an engine (every instance gets the Byzantine mask)
//   item I t initialized | inst I status | lifedone V          the synthetic ItemState / InstState / life_done
//   r t kind type instance node kp s value d0 d1 d2 d3         one brc_injection of the next batch
//   inject                                                     brc_inject of the batch
//   run life max_s                                             brc_run's budget decision, s_limit and, if it runs, note_run
//   reset                                                      brc_reset
//   quiet V                                                    V = 1: print no J / T / O lines
// Output: E (the plan, or its refusal), then per inject an I line (rc, state fetches, the text or the staged count), the
// staged records (J), every rewritten table word (T), the re-opened instances (O) and the book's counters (K); per run a
// G line; per reset a Z line.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include <iostream>
#include <sstream>

#include "../byzantinerandomizedconsensus_amd/csrc/brc_inject.h"

using namespace brc;

namespace {

struct Sim {
    brc_config c = {};
    Plan p;
    InjectBook book;
    std::vector<uint64_t> hbyz;
    std::vector<ItemState> its;
    std::vector<InstState> ist;
    std::vector<brc_injection> batch;
    bool ok = false, pattern_active = false, life_done = false, fresh = true, quiet = false;
};

uint64_t num(std::istringstream& in) {
    std::string tok;
    if (!(in >> tok)) { fprintf(stderr, "script: missing number\n"); exit(2); }
    return strtoull(tok.c_str(), nullptr, 0);
}

void counters(const Sim& s) {
    size_t sends = 0, recs = 0;
    for (const auto& kv : s.book.sends) sends += kv.second.size();
    for (const auto& kv : s.book.recs) recs += kv.second.size();
    printf("K gen_base=%" PRIu64 " gen_cur=%" PRIu64 " gen_smax=%" PRIu64 " gen_extra=%" PRIu64 " gen_props=%" PRIu64
           " gen_used=%" PRIu64 " sends=%zu links=%zu recs=%zu\n", s.book.gen_base, s.book.gen_cur, s.book.gen_smax,
           s.book.gen_extra, s.book.gen_props, s.book.gen_used(s.c), sends, s.book.links.size(), recs);
}

void engine(Sim& s, std::istringstream& in) {
    std::string name, env;
    in >> name;
    s = Sim();
    brc_config& c = s.c;
    c.n = (uint32_t)num(in); c.f = (uint32_t)num(in); c.protocol = (uint32_t)num(in); c.mode = (uint32_t)num(in);
    c.peer_mode = (uint32_t)num(in); c.delay_model = (uint32_t)num(in); c.delay_max = (uint32_t)num(in);
    c.key_window = (uint32_t)num(in); c.variants = (uint32_t)num(in); c.proposals = (uint32_t)num(in);
    c.byz_pattern = (uint32_t)num(in); c.flags = (uint32_t)num(in); c.instances = num(in);
    in >> env;
    c.byzantine_mask = num(in);
    for (int w = 0; w < 3; ++w) c.byzantine_mask_hi[w] = num(in);
    c.seed = 1; c.delay_const = 1; c.round_cap = 1; c.step_cap = 9000;
    PlanEnv pe;
    pe.kernel = env == "-" ? nullptr : env.c_str();
    std::string why;
    const int rc = make_plan(c, pe, &s.p, &why);
    if (rc != BRC_OK) { printf("E %s rc=%d why=%s\n", name.c_str(), rc, why.c_str()); return; }
    const Plan& p = s.p;
    s.ok = true;
    s.its.assign(p.nitems, ItemState{});
    s.ist.assign(c.instances, InstState{});
    for (uint64_t i = 0; i < c.instances; ++i)
        for (uint32_t w = 0; w < p.bw; ++w)
            s.hbyz.push_back((w == 0 ? c.byzantine_mask : c.byzantine_mask_hi[w - 1]) & word_mask(c.n, w));
    s.pattern_active = c.byz_pattern == BRC_BYZ_EQUIVOCATE && !(c.flags & BRC_FLAG_LIFE_PATTERN);
    printf("E %s rc=0 npad=%d ipw=%d bw=%u wide=%d wide_rec=%d compact=%d step_ok=%d nval=%u nitems=%" PRIu64 "\n", name.c_str(),
           p.npad, p.ipw, p.bw, p.wide, p.wide_rec, p.compact, p.step_ok, p.nval, p.nitems);
}

void inject(Sim& s) {
    int fetches = 0;
    auto fetch = [&](std::vector<ItemState>& its, std::vector<InstState>& ist) {
        ++fetches;
        its = s.its; ist = s.ist;
        return (int)BRC_OK;
    };
    InjectBatch b;
    std::string why;
    const int rc = stage_injections(s.p, s.c, s.book, s.hbyz, s.pattern_active, s.life_done, s.batch.data(), s.batch.size(),
                                    fetch, &b, &why);
    s.batch.clear();
    if (rc != BRC_OK) { printf("I rc=%d fetches=%d why=%s\n", rc, fetches, why.c_str()); return; }
    printf("I rc=0 fetches=%d staged=%zu\n", fetches, b.staged.size());
    for (size_t i = 0; !s.quiet && i < b.staged.size(); ++i) {
        const InjDev& r = b.staged[i];
        printf("J item=%" PRIu64 " t=%u slot=%u s=%u kind=%u type=%u seg=%u node=%u value=%d restricted=%u dst=%" PRIx64
               ",%" PRIx64 ",%" PRIx64 ",%" PRIx64 "\n", b.staged_item[i], r.t, r.slot, r.s, r.kind, r.type, r.seg, r.node,
               r.value, r.restricted, r.dst, r.dst_hi[0], r.dst_hi[1], r.dst_hi[2]);
    }
    for (const auto& tb : b.tables) {
        if (s.quiet) break;
        printf("T item=%" PRIu64 " count=%u words=", tb.item, tb.count);
        for (size_t j = 0; j < tb.words.size(); ++j) printf("%s%" PRIx64, j ? "," : "", tb.words[j]);
        printf("\n");
    }
    if (!s.quiet) {
        printf("O");
        for (const auto& ro : b.reopen) printf(" %" PRIu64, ro.first);
        printf("\n");
    }
    for (const auto& ro : b.reopen) s.ist[ro.first] = ro.second;
    s.book.commit(s.p, s.c, b);
    counters(s);
}

// brc_run around the launch: the budget decision, the full clear it may ask for, s_limit, the counters afterwards
void run(Sim& s, bool life, uint64_t max_s) {
    const bool genfree = s.p.compact || s.p.wide;
    bool clear = false;
    std::string why;
    if (!s.book.run_budget(s.c, s.fresh, genfree, life, &clear, &why)) { printf("G rc=%d why=%s\n", BRC_E_STATE, why.c_str()); return; }
    if (clear) s.book.full_clear();
    printf("G rc=0 clear=%d s_limit=%u\n", clear, s.book.s_limit(s.c, genfree, life));
    s.fresh = false;
    if (life) s.life_done = true;
    if (!genfree && !life) s.book.note_run(s.c, max_s);
    counters(s);
}

void reset(Sim& s) {
    const bool full = s.book.close_epoch();
    if (full && s.p.step_ok) s.book.full_clear();     // clear_state(full)
    s.book.clear_epoch();
    s.its.assign(s.p.nitems, ItemState{});
    s.ist.assign(s.c.instances, InstState{});
    s.fresh = true;
    s.life_done = false;
    printf("Z full=%d\n", full);
    counters(s);
}

}  // namespace

int main() {
    Sim s;
    std::string line, cmd;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        if (!(in >> cmd) || cmd[0] == '#') continue;
        if (cmd == "engine") { engine(s, in); continue; }
        if (!s.ok) { fprintf(stderr, "script: '%s' without an engine\n", cmd.c_str()); return 2; }
        if (cmd == "item") {
            const uint64_t i = num(in);
            if (i >= s.its.size()) { fprintf(stderr, "script: item out of range\n"); return 2; }
            s.its[i].t = (uint32_t)num(in); s.its[i].initialized = (uint32_t)num(in);
        } else if (cmd == "inst") {
            const uint64_t i = num(in);
            if (i >= s.ist.size()) { fprintf(stderr, "script: instance out of range\n"); return 2; }
            s.ist[i].status = (uint16_t)num(in);
        } else if (cmd == "lifedone") {
            s.life_done = num(in) != 0;
        } else if (cmd == "quiet") {
            s.quiet = num(in) != 0;
        } else if (cmd == "r") {
            brc_injection x = {};
            x.t = (uint32_t)num(in); x.kind = (uint16_t)num(in); x.type = (uint16_t)num(in); x.instance = num(in);
            x.node = (uint32_t)num(in); x.kp = (uint32_t)num(in); x.s = (uint32_t)num(in); x.value = (int32_t)(int64_t)num(in);
            x.dst_mask = num(in);
            for (int w = 0; w < 3; ++w) x.dst_mask_hi[w] = num(in);
            s.batch.push_back(x);
        } else if (cmd == "inject") {
            inject(s);
        } else if (cmd == "run") {
            const bool life = num(in) != 0;
            run(s, life, num(in));
        } else if (cmd == "reset") {
            reset(s);
        } else {
            fprintf(stderr, "script: unknown command '%s'\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
