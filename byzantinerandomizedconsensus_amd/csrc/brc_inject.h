// brc_inject.h -- what brc_inject decides before it touches the device, and the host's book of the injections an engine
// has taken: the checks and refusal texts, the links a Byzantine replica's ECHO / READY or a repeated SEND still has,
// the records of the item tables (brc_step.h's 3-word table, brc_step_wide.h's WREC_W-word one) as the packed words
// the device gets, the all-or-nothing rule, and the slot generation budget of brc_run and brc_reset.  A pure function
// of the plan, the brc_config, the host copy of the Byzantine masks, the book and two small device structs per
// instance, so it needs no HIP header and a stand-alone host program can call it (tests/inject_dump.cpp).
// brc_engine.hip executes the result: it uploads the tables, queues the records, re-opens instances, and commits.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <map>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "brc_layout.h"
#include "brc_plan.h"

namespace brc {

// bits of replicas 64w .. 64w+63 that exist in an n-replica instance
inline uint64_t word_mask(uint32_t n, uint32_t w) {
    const uint32_t lo = 64 * w;
    return n >= lo + 64 ? ~0ull : (n <= lo ? 0ull : ((1ull << (n - lo)) - 1));
}

// What stage_injections makes of an accepted brc_inject call
struct InjectBatch {
    struct Table { uint64_t item; std::vector<uint64_t> words; uint32_t count; };   // XSEND_MAX packed records, xsn
    struct SendDst { uint32_t node; uint64_t dst[4]; };
    struct Links { uint64_t w[4] = {0, 0, 0, 0}; bool rec = false; };
    // type: 0 = an extra SEND; BRC_ECHO / BRC_READY = a Byzantine replica's message to a subset of the peers.
    // Narrow tables: the senders in smask, one destination word; wide ones: one sender (node), four words
    struct Rec { uint32_t k, t, seg, type, node; uint64_t smask, dst[4]; };
    using LinkKey = std::pair<uint64_t, uint64_t>;   // instance, link_key(node, type, kp, s)
    std::vector<InjDev> staged;                      // the records for `pending` ...
    std::vector<uint64_t> staged_item;               // ... and their items
    std::vector<Table> tables;                       // the item tables to rewrite
    std::vector<std::pair<uint64_t, InstState>> reopen;   // QUIESCENT instances, as they are written back: RUNNING
    // the book's delta (InjectBook::commit): this call's SENDs per key; the links and the tables in flight it touched,
    // as they stand after it
    std::unordered_map<uint64_t, std::vector<SendDst>> sends;
    std::map<LinkKey, Links> links;
    std::map<uint64_t, std::vector<Rec>> recs;
};

// The injections an engine has taken since brc_create / brc_reset, and its slot generation budget
struct InjectBook {
    using SendDst = InjectBatch::SendDst;
    using Links = InjectBatch::Links;
    using Rec = InjectBatch::Rec;
    // injected SENDs per key (instance << 32 | kp << 16 | s): each sender's destinations (all four words: the wide
    // kernels' extra SENDs drop a node's used links over bw words)
    std::unordered_map<uint64_t, std::vector<SendDst>> sends;
    // injected ECHO / READY of Byzantine replicas on the kernels that take records, per (instance, node, type, key):
    // the links used so far, and whether some of them went through a record (the sending lane's cell then keeps no
    // send step, and a later broadcast becomes a record too).  The narrow kernels use word 0 (bw = 1)
    std::map<InjectBatch::LinkKey, Links> links;
    std::unordered_map<uint64_t, std::vector<Rec>> recs;    // item -> records in flight (P.xsend)
    // slot generation budget: the allocations of one key slot in an epoch (brc_reset to brc_reset) are bounded by
    // gen_used() below; gen_base sums the epochs since the last full clear
    uint64_t gen_base = 0, gen_cur = 0;
    // what bounds them (tagged kernels only; DESIGN.md section 3, "Key slots"), per epoch:
    // gen_smax: the largest phase index a launch has reported; gen_extra: over the key slots, the most injected
    // KEY / SEND records that can allocate one slot beyond one per key (under the consensus protocol every such
    // record: the kernel may allocate the key itself); gen_passes: the most PROPOSE records of one replica (each
    // starts its phase indices over), plus one when the engine proposes by itself
    uint64_t gen_smax = 0, gen_extra = 0, gen_props = 0;
    std::unordered_map<uint64_t, uint32_t> key_recs;    // instance << 32 | kp << 16 | s -> allocating records
    std::unordered_map<uint64_t, uint32_t> slot_extra;  // instance << 32 | slot -> the slot's count for gen_extra
    std::unordered_map<uint64_t, uint32_t> prop_recs;   // instance << 32 | node -> PROPOSE records

    static constexpr uint64_t GEN_HARD = GEN_MASK - 2;

    // brc_reset: the epoch's injections and counters (the generations spent stay: close_epoch)
    void clear_epoch() {
        sends.clear(); links.clear(); recs.clear(); key_recs.clear(); slot_extra.clear(); prop_recs.clear();
        gen_smax = gen_extra = gen_props = 0;
    }
    // every tag is zero again (clear_state(full), and the first run of an epoch that needs it)
    void full_clear() { gen_base = gen_cur = 0; }
    // brc_reset: whether it must clear fully; if not, the epoch's generations join gen_base
    bool close_epoch() {
        const bool full = gen_base + gen_cur >= GEN_FULL_CLEAR;
        if (!full) { gen_base += gen_cur; gen_cur = 0; }
        return full;
    }

    // Slot generations (tagged kernels): how far this epoch can have advanced the tag of one key slot, plus one to
    // spare.  The kernels allocate a slot (gen + 1, brc_step.h) in send_key_now -- a replica's own key of phase index
    // s, once per s and pass, s rising within a pass (a PROPOSE starts the next pass) -- and in send_rec, for every
    // KEY record and every SEND record whose key is not declared-and-unsent.  With one record per key the records are
    // the keys of the slot, at most smax / Q + 1 of them; every further record is counted in gen_extra.
    uint64_t gen_passes(const brc_config& c) const {
        return std::max<uint64_t>(1, gen_props + (c.proposals != BRC_PROPOSALS_NONE ? 1u : 0u));
    }
    uint64_t gen_used(const brc_config& c) const { return gen_passes(c) * (gen_smax / c.key_window + 1) + gen_extra + 1; }

    // brc_run's budget decision.  Slot generations are 13-bit tags: past the budget a stale cell could read as current.
    // brc_reset clears fully once gen_base + gen_cur reaches GEN_FULL_CLEAR, and so does the first run of an epoch
    // whose staged records need it (*clear; nothing has run: every slot is free, only tags and stale cells are
    // dropped), so gen_base stays below GEN_FULL_CLEAR and phase indices alone never get here (s_limit turns them into
    // BRC_OVERFLOW).  Injected records do: KEYs of one key allocate its slot once each, and nothing can clear an epoch
    // under way.  genfree: the lean (compact-cell) and the wide kernels keep no generation tags, nor does a run of the
    // lifetime kernel (life): a slot's row is rewritten at allocation, so only the 14-bit phase-index snapshot bounds
    // them.  false: refused, the text in *why
    bool run_budget(const brc_config& c, bool fresh, bool genfree, bool life, bool* clear, std::string* why) const {
        *clear = false;
        if (genfree || life) return true;
        *clear = fresh && gen_base > 0 && gen_base + gen_used(c) >= GEN_FULL_CLEAR;
        if ((*clear ? 0 : gen_base) + gen_used(c) < GEN_HARD) return true;
        // gen_used counts a key's first record under BRB as its one allocation: on a fresh engine the 8188th KEY
        // of one key (consensus protocol: the 8187th record of one slot) is the first to get here
        *why = "slot generation budget exhausted: call brc_reset (the records injected in this epoch can allocate "
               "one key slot more often than the " + std::to_string(GEN_HARD - 1 - (*clear ? 0 : gen_base)) +
               " generation tags left)";
        return false;
    }
    // P.s_limit: a slot allocated for phase index s has been reallocated at most gen_base + passes * (s / Q + 1) +
    // gen_extra times (gen_used; run_budget keeps the difference positive), and phase indices stay below 2^14 - 1: the
    // narrow kernel's consensus snapshot keeps s + 1 in 14 bits.  (The lifetime kernel reads no s_limit.)
    uint32_t s_limit(const brc_config& c, bool genfree, bool life) const {
        const uint64_t gen_spent = gen_base + gen_extra;
        return (genfree || life || gen_spent + 1 >= GEN_HARD)
                   ? 0x3FFEu
                   : (uint32_t)std::min<uint64_t>(0x3FFEull, (GEN_HARD - 1 - gen_spent) / gen_passes(c) * c.key_window);
    }
    // after a launch of a tagged step kernel; max_s: the largest phase index it reported
    void note_run(const brc_config& c, uint64_t max_s) {
        gen_smax = std::max<uint64_t>(gen_smax, max_s);
        gen_cur = std::max<uint64_t>(gen_cur, gen_used(c));
    }

    // An accepted call's delta, and the records that can allocate a key slot, for the generation budget: the tagged
    // kernels only (!(compact || wide)), every PROPOSE per replica, every KEY and first SEND per key -- beyond one per
    // key, or, under the consensus protocol, every one
    void commit(const Plan& p, const brc_config& c, const InjectBatch& b) {
        for (size_t i = 0; !(p.compact || p.wide) && i < b.staged.size(); ++i) {
            const InjDev& r = b.staged[i];
            const uint64_t in = b.staged_item[i] * p.ipw + r.seg;
            if (r.kind == BRC_INJ_PROPOSE) {
                gen_props = std::max<uint64_t>(gen_props, ++prop_recs[(in << 32) | r.node]);
            } else if (r.kind == BRC_INJ_KEY || (r.kind == BRC_INJ_SEND && !(r.type & 2))) {
                const uint32_t kp = r.slot / c.key_window;
                const uint32_t nth = ++key_recs[(in << 32) | ((uint64_t)kp << 16) | r.s];
                if (nth > 1 || c.protocol == BRC_PROTO_CONSENSUS)
                    gen_extra = std::max<uint64_t>(gen_extra, ++slot_extra[(in << 32) | r.slot]);
            }
        }
        for (const auto& kv : b.sends) {
            auto& v = sends[kv.first];
            v.insert(v.end(), kv.second.begin(), kv.second.end());
        }
        for (const auto& kv : b.links) links[kv.first] = kv.second;
        for (const auto& kv : b.recs) recs[kv.first] = kv.second;
    }
};

// (node, type, key) of an injected ECHO / READY: node < 256, kp < 1024, s < 2^16
inline uint64_t link_key(uint32_t node, uint32_t type, uint32_t kp, uint32_t s) {
    return ((uint64_t)node << 40) | ((uint64_t)(type == BRC_READY) << 32) | ((uint64_t)kp << 16) | s;
}

// The two device formats of a record table: XSEND_MAX records of 3 words (brc_step.h) or WREC_W words (brc_step_wide.h)
inline InjectBatch::Table pack_table(bool wide, uint64_t item, const std::vector<InjectBatch::Rec>& v) {
    const uint32_t W = wide ? WREC_W : 3;
    InjectBatch::Table tb{item, std::vector<uint64_t>(W * XSEND_MAX, 0), (uint32_t)v.size()};
    for (size_t j = 0; j < v.size(); ++j) {
        const auto& q = v[j];
        uint64_t* o = &tb.words[W * j];
        o[0] = (uint64_t)q.k | ((uint64_t)q.t << 16) | ((uint64_t)q.type << XS_TYPE_SH);
        if (wide) {
            o[0] |= (uint64_t)q.node << WREC_NODE_SH;
            for (int w = 0; w < 4; ++w) o[1 + w] = q.dst[w];
        } else {
            o[0] |= (uint64_t)q.seg << 40;
            o[1] = q.smask;
            o[2] = q.dst[0];
        }
    }
    return tb;
}

// One brc_inject call: BRC_OK and *out, or a return code with its text in *why and nothing else changed.
// pattern_active / life_done: the engine's byz_pattern list is in place; its last run was the key-lifetime kernel's.
// fetch(its, ist) reads the device's ItemState[nitems] and InstState[instances] (BRC_OK, or its own failure code, which
// is returned with *why left alone).  It is called once, at the first record that passes its static checks, and never
// for count == 0.
template <class Fetch>
int stage_injections(const Plan& p, const brc_config& c, const InjectBook& book, const std::vector<uint64_t>& hbyz,
                     bool pattern_active, bool life_done, const brc_injection* list, size_t count, Fetch&& fetch,
                     InjectBatch* out, std::string* why) {
    auto refuse = [&](int rc, const std::string& s) { *why = s; return rc; };
    // before any record is looked at: a pattern engine, then a lifetime-only one
    if (pattern_active) return refuse(BRC_E_STATE, "explicit injections cannot be combined with byz_pattern");
    if (!p.step_ok && count) return refuse(BRC_E_UNSUPPORTED, life_only_why(p, false));
    const uint64_t all = (c.n >= 64) ? ~0ull : ((1ull << c.n) - 1);
    std::vector<ItemState> its;
    std::vector<InstState> ist;
    bool have_state = false;
    InjectBatch b;
    // restricted ECHO / READY records: the non-lean narrow step kernels with sender peers (brc_step.h record pre-pass)
    // and the wide kernels of an engine created with BRC_FLAG_WIDE_RECORDS (sender peers: make_plan)
    const bool msg_records = (!p.wide && !p.compact && c.peer_mode == BRC_PEER_SENDER) || p.wide_rec;
    auto any4 = [](const uint64_t* w) { return (w[0] | w[1] | w[2] | w[3]) != 0; };
    // Per record, in this order: range, value / s, the kind's own checks, then the device state (time before the
    // current step, instance finished by the lifetime kernel, instance stopped).  The first failing record decides
    // the code and text; the records before it leave nothing behind, their link and SEND counts included (they live
    // in b until InjectBook::commit)
    for (size_t i = 0; i < count; ++i) {
        const brc_injection& x = list[i];
        if (x.instance >= c.instances || x.node >= c.n || x.t > c.step_cap) return refuse(BRC_E_INVALID, "injection out of range");
        if (x.value < 0 || x.value >= (int)(c.mode == BRC_MODE_SPEC ? 4u : p.nval) || x.s >= 0xFFFE)
            return refuse(BRC_E_INVALID,
                          "value id / phase index out of range (value ids 4..7 need n <= 32, connection peers up to n = 64, "
                          "BRC_FLAG_GENERAL_KEYS at n in 33..64 or BRC_FLAG_WIDE_VALUES at n > 64 with sender peers; not SPEC)");
        bool drop = false;                       // a repeated SEND carried on no link (sender peers)
        InjDev r = {};
        r.t = x.t; r.kind = (uint8_t)x.kind; r.type = (uint8_t)x.type; r.node = (uint8_t)x.node;
        r.seg = (uint8_t)(x.instance % p.ipw); r.value = (int8_t)x.value; r.s = (uint16_t)x.s;
        r.dst = x.dst_mask & all;
        bool full = (r.dst == word_mask(c.n, 0));
        for (uint32_t w = 1; w < p.bw; ++w) {
            r.dst_hi[w - 1] = x.dst_mask_hi[w - 1] & word_mask(c.n, w);
            full = full && r.dst_hi[w - 1] == word_mask(c.n, w);
        }
        uint64_t* dw[4] = {&r.dst, &r.dst_hi[0], &r.dst_hi[1], &r.dst_hi[2]};   // (the words past bw stay zero)
        r.restricted = (x.kind == BRC_INJ_SEND && !full) ? 1 : 0;
        if (x.kind == BRC_INJ_PROPOSE) {
            if (c.protocol != BRC_PROTO_CONSENSUS) return refuse(BRC_E_INVALID, "PROPOSE needs the consensus protocol");
        } else if (x.kind == BRC_INJ_DELIVER) {
            if (c.protocol != BRC_PROTO_CONSENSUS) return refuse(BRC_E_INVALID, "DELIVER needs the consensus protocol");
            if (c.mode == BRC_MODE_SPEC) return refuse(BRC_E_UNSUPPORTED, "DELIVER: SPEC consensus counts phase-indexed keys");
            if (x.kp >= c.n) return refuse(BRC_E_INVALID, "DELIVER host out of range");
            r.slot = (uint16_t)x.kp;               // the message's host
        } else if (x.kind == BRC_INJ_SEND || x.kind == BRC_INJ_MSG || x.kind == BRC_INJ_KEY) {
            if (x.kp >= c.n * c.variants) return refuse(BRC_E_INVALID, "kp out of range");
            r.slot = (uint16_t)(x.kp * c.key_window + (x.s % c.key_window));
            if (x.kind == BRC_INJ_MSG) {
                if (x.type != BRC_ECHO && x.type != BRC_READY) return refuse(BRC_E_INVALID, "MSG type must be ECHO or READY");
                if (!full && !msg_records)
                    return refuse(BRC_E_UNSUPPORTED,
                        c.peer_mode == BRC_PEER_CONNECTION
                        ? "an ECHO / READY to a subset of the peers: not with connection peers (every message is a new "
                          "peer there; the record pre-pass counts senders)"
                        : p.wide ? "an ECHO / READY to a subset of the peers: not on the wide kernels (n > 64), whose "
                                   "receivers ballot over the senders' cells"
                                 : "an ECHO / READY to a subset of the peers: not on the lean kernels (n in 33..64 with "
                                   "sender peers; BRC_FLAG_GENERAL_KEYS runs the general form)");
                // the record path is a Byzantine sender's: an honest one to a subset is refused
                const bool byz = (hbyz[x.instance * p.bw + x.node / 64] >> (x.node % 64)) & 1ull;
                if (!full && !byz)
                    return refuse(BRC_E_UNSUPPORTED,
                                  "an ECHO / READY to a subset of the peers needs a Byzantine sender: an honest replica's own "
                                  "later broadcast would need per-link suppression the cells do not have");
                if (msg_records && byz) {
                    // the links (node, type, key) used before, this batch included.  A message to a subset, and every
                    // later one of a (node, type, key) that had one, goes over the remaining links as a record of the
                    // item's table (possibly over none: it still is an action of its step); a broadcast to every peer
                    // with no record before it keeps the cell path, which uses every link, and still books its links
                    const auto lk = std::make_pair((uint64_t)x.instance, link_key(x.node, x.type, x.kp, x.s));
                    InjectBatch::Links u;
                    auto it = b.links.find(lk);
                    if (it != b.links.end()) u = it->second;
                    else if (auto jt = book.links.find(lk); jt != book.links.end()) u = jt->second;
                    if (!full || u.rec) {
                        const bool first = !any4(u.w);
                        for (int w = 0; w < 4; ++w) *dw[w] &= ~u.w[w];
                        const uint64_t left[4] = {*dw[0], *dw[1], *dw[2], *dw[3]};
                        // bit 1, a SEND event: no link was used before and one is left
                        r.restricted = (uint8_t)(1u | ((first && any4(left)) ? 2u : 0u));
                        u.rec = true;
                    }
                    for (int w = 0; w < 4; ++w) u.w[w] |= *dw[w];
                    b.links[lk] = u;
                }
            } else if (x.kind == BRC_INJ_SEND) {
                // a second SEND of a key (another origin or the same, one payload string SENT again):
                // an extra-SEND record on the non-lean narrow step kernels and on the wide kernels of an engine
                // created with BRC_FLAG_WIDE_RECORDS; the lean and the flagless wide kernels model one SEND per key
                const uint64_t k64 = (x.instance << 32) | (uint64_t)(x.kp * 0x10000u + x.s);
                // this node's earlier SENDs of the key (this batch included): r.type bit 0 marks a repeat
                // (brc_step.h: a COPY event with connection peers); sender peers carry a repeated
                // message on a link no further (the links it used are dropped from the record, over all four words)
                uint32_t before = 0;
                uint64_t prev[4] = {0, 0, 0, 0};
                bool had = false;
                const InjectBatch& cb = b;
                for (const auto* mp : {&book.sends, &cb.sends}) {
                    auto it = mp->find(k64);
                    if (it == mp->end()) continue;
                    before += (uint32_t)it->second.size();
                    for (const auto& q : it->second)
                        if (q.node == x.node) {
                            for (int w = 0; w < 4; ++w) prev[w] |= q.dst[w];
                            had = true;
                        }
                }
                const bool one_send = p.compact || (p.wide && !p.wide_rec);
                if (one_send && before)
                    return refuse(BRC_E_UNSUPPORTED,
                                  "a key can be SENT only once on this kernel (n in 33..64 with sender peers, or n > 64 "
                                  "without BRC_FLAG_WIDE_RECORDS)");
                b.sends[k64].push_back(InjectBatch::SendDst{x.node, {r.dst, r.dst_hi[0], r.dst_hi[1], r.dst_hi[2]}});
                // r.type bit 1: a key SENT before (by any node) on the kernels that take it, an extra-SEND record
                r.type = ((!one_send && before > 0) ? 2 : 0) | (had ? 1 : 0);
                if (c.peer_mode == BRC_PEER_SENDER)
                    for (int w = 0; w < 4; ++w) *dw[w] &= ~prev[w];
                drop = had && !(r.dst | r.dst_hi[0] | r.dst_hi[1] | r.dst_hi[2]);
            }
        } else {
            return refuse(BRC_E_INVALID, "unknown injection kind");
        }
        if (!have_state) {
            const int rc = fetch(its, ist);
            if (rc) return rc;
            have_state = true;
        }
        const uint64_t item = x.instance / p.ipw;
        if (its[item].initialized != 0 && x.t < its[item].t)
            return refuse(BRC_E_STATE, "injection time is before the instance's current step");
        if (ist[x.instance].status == BRC_QUIESCENT && life_done)
            return refuse(BRC_E_STATE, "instance finished by the key-lifetime kernel (no step state to resume): brc_reset first");
        if (ist[x.instance].status != BRC_QUIESCENT && ist[x.instance].status != BRC_RUNNING)
            return refuse(BRC_E_STATE, "instance already stopped");
        // a repeated SEND carried on no link (sender peers) changes no instance state: accepted, not staged
        // (after the stopped-instance checks: a stopped instance refuses it like every other injection; it stays
        // in b.sends, the SEND book-keeping)
        if (drop) continue;
        if (ist[x.instance].status == BRC_QUIESCENT) {
            InstState st = ist[x.instance];
            st.status = BRC_RUNNING;
            b.reopen.emplace_back(x.instance, st);
        }
        b.staged.push_back(r);
        b.staged_item.push_back(item);
    }
    // Extra-SEND records (r.type bit 1) and restricted ECHO / READY records (r.restricted) into their items' tables.
    // Only an item that gains a record has its table rebuilt, and the rebuild drops the records whose arrivals all lie
    // in steps already run (t + delay_max < item.t on an initialised item), so the kernel's per-step scan covers live
    // records only.  Narrow tables: a record of the same key, step, type and destinations without this sender takes it
    // into smask, else a new one; an extra SEND is recorded even with no link left, a restricted message is not.  Wide
    // tables: one sender per record, never merged, nothing recorded with no link left.  The 17th record of a table
    // refuses the call (all-or-nothing: nothing has changed)
    for (size_t i = 0; i < b.staged.size(); ++i) {
        const InjDev& r = b.staged[i];
        const uint64_t dst[4] = {r.dst, r.dst_hi[0], r.dst_hi[1], r.dst_hi[2]};
        const bool xsend = r.kind == BRC_INJ_SEND && (r.type & 2);
        const bool xmsg = r.kind == BRC_INJ_MSG && r.restricted;
        if ((!xsend && !xmsg) || (!any4(dst) && (p.wide || xmsg))) continue;
        const uint32_t rtype = xmsg ? r.type : 0u;
        const uint64_t item = b.staged_item[i];
        auto ins = b.recs.emplace(item, std::vector<InjectBatch::Rec>());
        auto& v = ins.first->second;
        if (ins.second)
            if (auto it = book.recs.find(item); it != book.recs.end())
                for (const auto& q : it->second)
                    if (!(its[item].initialized != 0 && q.t + c.delay_max < its[item].t)) v.push_back(q);
        size_t slot = v.size();
        for (size_t j = 0; !p.wide && j < v.size(); ++j)
            if (v[j].k == r.slot && v[j].t == r.t && v[j].seg == r.seg && v[j].type == rtype && v[j].dst[0] == r.dst &&
                !((v[j].smask >> r.node) & 1ull)) {
                slot = j;
                break;
            }
        if (slot < v.size()) v[slot].smask |= 1ull << r.node;
        else if (v.size() < XSEND_MAX)
            v.push_back(InjectBatch::Rec{r.slot, r.t, r.seg, rtype, r.node, p.wide ? 0ull : 1ull << r.node,
                                         {dst[0], dst[1], dst[2], dst[3]}});
        else
            return refuse(BRC_E_UNSUPPORTED, "more than " + std::to_string(XSEND_MAX) +
                                                 " extra-SEND / restricted ECHO / READY records in flight in one " +
                                                 (p.wide ? "instance" : "item"));
    }
    for (const auto& kv : b.recs) b.tables.push_back(pack_table(p.wide, kv.first, kv.second));
    *out = std::move(b);
    return BRC_OK;
}

}  // namespace brc
