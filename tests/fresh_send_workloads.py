"""Workloads of tests/test_gpu_fresh_send.py (GPU) and tests/test_fresh_send_workloads.py (their preconditions, on the
oracle and the schedule alone): the lean typed step kernels leave a new key's cell row unwritten until its first SEND
key-step stores it whole (csrc/brc_step.h BRC_FRESH_SEND, M_FRESH).  What can go wrong depends on what touches a slot
between its allocation and that key-step, not on the batch size: n = 64, f = 21 (one case at n = 33: lanes that are
no replicas), 8 instances a case, every one of them compared with the oracle.

Every case is a tests/step_noevent_workloads.Case: the GPU test compares the event-log-free build (the fresh path) with
its EV = true twin (rows written at allocation, the single mixed list) and with the C oracle.

Slow-set delays (two classes, 1 and 8 steps): every link from a replica of the instance's slow set takes 8 steps, so
the SEND of a slow origin stays in flight, its slot unwritten, for 8 steps; a fast origin's SEND has two landings
(fast receivers after 1 step, slow ones after 8): the first is the fresh key-step, the second an ordinary one.

Not here, on purpose: an ECHO / READY to a SUBSET of the peers on an unwritten slot.  brc_inject refuses a restricted
ECHO / READY on the compact-cell (lean) kernels (csrc/brc_engine.hip brc_inject: BRC_INJ_MSG with dst short of every
peer needs msg_records, the non-lean narrow kernels' record pre-pass), so that message cannot reach the kernels this
file is about.  The
fallbacks that do exist here: ECHO / READY to everyone before the SEND lands (fresh-*-early), a restricted SEND
(fresh-*-restricted), a declared key (fresh-*-declared), direct deliver() calls (fresh-ref-deliver).

mask_cases(): batches whose instances carry DIFFERENT Byzantine masks, loaded with brc_load_byzantine over a
configuration mask that equals none of them (tests/byz_mask_workloads.Case: its mask rules, its oracle runs of every
instance).  The fresh store takes its hit lanes from the wave's own honest mask, so this is the input that could break
"lanes that are not honest end with the fresh word".
"""
from tests import step_noevent_workloads as T
from tests import typed_list_workloads as W
from tests.golden import specs as S

N, F = 64, 21
SEED = 0xF5E5D
COUNT = 8
ALL64 = (1 << 64) - 1
BYZ = [58, 59, 60, 61, 62, 63]
ORIGINS = (0, 7, 13, 22, 31, 40, 49, 57)           # eight honest origins: some of every instance's slow set, some not
CUT_CAP = 4                                         # the step cap of the cut run: below the slow links' 8 steps


class Case(T.Case):
    def oracle_ids(self):
        return list(range(self.count))


def schedule(sp):
    from oracle.schedule import Schedule
    return Schedule(sp["n"], sp["f"], sp["seed"], sp["delay_model"], sp["dmax"], sp.get("dconst", 1))


def _cons(mode, model, dmax, round_cap, q, n=N, f=F, **kw):
    def make(g):
        if mode == T.SPEC:
            return S.spec_cons_spec(n, f, SEED, model, dmax, g, round_cap=round_cap, window=q, coin_seed=T.COIN, **kw)
        return S.cons_spec(n, f, SEED, model, dmax, g, round_cap=round_cap, **kw)
    return make


def _brb(mode, sends, extra=(), model=T.SLOW, dmax=8, dconst=1, step_cap=400, window=4):
    def make(g):
        sp = S.brb_spec(N, F, SEED, model, dmax, g, sends, dconst=dconst, byzantine=BYZ, extra=extra, step_cap=step_cap)
        if mode == T.SPEC:
            sp.update(mode="spec_brb", window=window, coin_seed=0)
        return sp
    return make


# ECHO and READY of every first-burst key, broadcast by two Byzantine replicas at step 1: the keys of slow origins are
# still in flight everywhere then (their rows unwritten), the others have had their first landing
EARLY = [dict(t=1, kind="byz", src=b, type=typ, kp=o, s=0, dst=ALL64) for b in (62, 63) for typ in (S.ECHO, S.READY)
         for o in ORIGINS]
FIRST = [(0, o, 0) for o in ORIGINS]
# a Byzantine origin's SEND to ten replicas, and another's to ten others two steps later (restricted: the general body)
RESTRICTED = W.restricted_send(60, 0, (1 << 10) - 1) + W.restricted_send(61, 2, 0x3FF << 20)
# a key declared at step 0 and never sent until step 120: its slot stays unwritten across the epoch move (rebase) that
# step 120 starts with, and across every launch boundary of a sliced run
DECLARED = [dict(t=0, kind="byz_key", kp=59, s=0, value=1),
            dict(t=120, kind="byz", src=59, type=S.SEND, kp=59, s=0, dst=ALL64),
            dict(t=120, kind="brb_send", node=3, kp=3, s=0, payload="TEST 4.0")]
# direct deliver() calls at step 2 on the honest replicas 5 and 6, for hosts whose keys are still in flight
DELIVERS = [dict(t=2, kind="deliver", node=d, kp=o, value=1) for d in (5, 6) for o in ORIGINS[:3]]
REUSE_Q = 4
# slot reuse: every origin SENDs sequence number 0 at step 0 and REUSE_Q (the same slot) at step 40
REUSE = FIRST + [(40, o, REUSE_Q) for o in ORIGINS]


def cases():
    out = []

    def add(name, mode, make, q, consensus=True, run=None, count=COUNT):
        # inst: the instantiation brc_create picks (NLR = 2 with at most two link delays, else 0)
        out.append(Case("fresh-" + name, T.instantiation(make(T.OFFSET), q), make, count, run or dict(proposals="inject"),
                        q, consensus=consensus))

    philox = dict(proposals="philox")
    for mode, mn, q in ((T.REF, "ref", 4), (T.SPEC, "spec", 8)):
        # the benchmark's own shape: slow-set delays up to 8, Philox proposals, round caps 1 and 3
        add("%s-cfg4-cap1" % mn, mode, _cons(mode, T.SLOW, 8, 1, q), q, run=philox)
        add("%s-cfg4-cap3" % mn, mode, _cons(mode, T.SLOW, 8, 3, 8), 8, run=philox)
        # one delay class: every SEND is a single fresh key-step
        add("%s-const3" % mn, mode, _cons(mode, T.CONST, 8, 1, q, dconst=3), q, run=philox)
        # per-link delays (masks in LDS): an origin's SEND lands at several steps, the first of them fresh
        add("%s-unif4-cap3" % mn, mode, _cons(mode, T.UNIF, 4, 3, 8), 8)
        add("%s-n33" % mn, mode, _cons(mode, T.SLOW, 8, 1, q, n=33, f=10), q, run=philox)
        add("%s-byz" % mn, mode, _cons(mode, T.SLOW, 8, 1, q, byzantine=BYZ), q)
        add("%s-early" % mn, mode, _brb(mode, FIRST, extra=EARLY), 4, consensus=False)
        add("%s-restricted" % mn, mode, _brb(mode, FIRST, extra=RESTRICTED), 4, consensus=False)
        add("%s-declared" % mn, mode, _brb(mode, FIRST, extra=DECLARED), 4, consensus=False)
        add("%s-reuse" % mn, mode, _brb(mode, REUSE, window=REUSE_Q), REUSE_Q, consensus=False)
        add("%s-cut" % mn, mode, _cons(mode, T.SLOW, 8, 1, q, step_cap=CUT_CAP), q, run=philox)
    # (key window 8: replicas 5 and 6 end their phases early and run ahead of the others; a window of 4 ends six
    # of the eight instances with BRC_OVERFLOW, the engine's own limit, which the oracle does not model)
    add("ref-deliver", T.REF, _cons(T.REF, T.SLOW, 8, 1, 8, extra=DELIVERS), 8)
    return out


def mask_cases():
    """Per-instance Byzantine masks: REFERENCE and SPEC with register delay masks (NLR = 2), SPEC with per-link delays
    (NLR = 0; the reference protocol stalls under them whatever the masks)."""
    from tests import byz_mask_workloads as B
    global _MASKS
    if _MASKS is None:
        _MASKS = [B.Case("fresh-masks-ref-slow8", B.REF, N, F, B.SLOW, 8, COUNT, 4),
                  B.Case("fresh-masks-spec-slow8", B.SPEC, N, F, B.SLOW, 8, COUNT, 8),
                  B.Case("fresh-masks-spec-n50-unif3", B.SPEC, 50, 16, B.UNIF, 3, COUNT, 8)]
    return _MASKS


_MASKS = None
_CASES = None


def by_name():
    global _CASES
    if _CASES is None:
        _CASES = {c.name: c for c in cases()}
    return _CASES


SLICED = ("fresh-ref-cfg4-cap1", "fresh-spec-cfg4-cap1", "fresh-ref-early", "fresh-ref-restricted", "fresh-ref-declared",
          "fresh-ref-unif4-cap3", "fresh-ref-reuse", "fresh-spec-reuse")
INTERLEAVED = ("fresh-ref-early", "fresh-spec-early")
LATE = ("fresh-ref-early", "fresh-ref-reuse", "fresh-ref-declared")
LATE_T0 = 59700                                     # the declared case runs 144 steps: all of it below STEP_LIMIT
