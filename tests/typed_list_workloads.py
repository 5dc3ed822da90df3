"""Workloads of tests/test_gpu_typed_lists.py (GPU) and tests/test_typed_list_workloads.py (their preconditions,
on the oracle alone): the lean step kernels' type-sorted key list (csrc/brc_step.h BRC_TYPED).  What can go wrong
there depends on how one step's list is composed -- which message types land on which keys, how many keys a
class holds, which key word a delivery falls in -- not on the batch size: n = 64, f = 21 (one case at n = 33,
the lean minimum with padding lanes), 16 instances a case.

Every case is a tests/step_noevent_workloads.Case, so the GPU test compares the event-log-free build (the typed
list) with its EV = true twin (the single mixed list) and with the C oracle through the same helpers.
"""
from tests import step_noevent_workloads as T
from tests.golden import specs as S

N, F = 64, 21
BYZ = list(range(58, 64))
ALL64 = (1 << 64) - 1
SEED = 0x7E11D
COUNT = 16
CONST3 = dict(model=T.CONST, dmax=8, dconst=3)      # every link takes three steps


def _cons(mode, model, dmax, round_cap, q, n=N, f=F, **kw):
    def make(g):
        if mode == T.SPEC:
            return S.spec_cons_spec(n, f, SEED, model, dmax, g, round_cap=round_cap, window=q, coin_seed=T.COIN, **kw)
        return S.cons_spec(n, f, SEED, model, dmax, g, round_cap=round_cap, **kw)
    return make


def _brb(mode, sends, extra=(), byzantine=BYZ, model=T.CONST, dmax=8, dconst=3):
    def make(g):
        sp = S.brb_spec(N, F, SEED, model, dmax, g, sends, dconst=dconst, byzantine=byzantine, extra=extra, step_cap=400)
        if mode == T.SPEC:
            sp.update(mode="spec_brb", window=8, coin_seed=0)
        return sp
    return make


def restricted_send(kp, t, dst):
    """A Byzantine origin's SEND that reaches only the replicas of ``dst`` (the kernel's kdst path)."""
    return [dict(t=t, kind="byz_key", kp=kp, s=0, value=1),
            dict(t=t, kind="byz", src=kp, type=S.SEND, kp=kp, s=0, dst=dst)]


# The merge case: consensus under three-step links, key window 8 (slot = 8 x origin + phase index mod 8, so key word
# w holds origins 8 w .. 8 w + 7).  Exactly as many replicas as a phase end needs deliveries -- MERGE_T0: more than
# n - f under the reference protocol (core/byzantinerandomizedconsensus.py:71), n - f under SPEC; origins 0 ..
# MERGE_T0 - 1, key words 0 .. 5 -- propose at step 0, the other honest ones one step later.  Their phase-0 keys
# deliver at every honest replica at step 9, when their READYs land, and a Byzantine ECHO of key (1, 0) injected at
# step 6 lands at step 9 too: that step's list holds all but one of the keys in the READY segment (words 0, 1, .. 5
# in turn) and key (1, 0) in the later ECHO + READY segment.  The kernel
# collects a key word's deliveries in a register and stores it when another word starts: word 0 is stored when word
# 1 starts, and key (1, 0) brings word 0 up again -- its store must merge with the bits already written this step,
# not replace them.  The consensus pass reads those words: a replica that has proposed ends phase 1 at step 9 only if
# it sees all MERGE_T0 deliveries (its phase-1 SEND leaves at step 9); with word 0's READY-segment bits lost it would
# see seven fewer and end the phase a step later, which moves every later event, t_stop and the message counts.
# (Checked once on an MI355X with a build whose flush overwrote instead: both cases then stop a step late, t_stop 19
# for 18 under the reference protocol and 37 for 36 under SPEC, and the comparison with twin and oracle fails.)
MERGE_T0 = {T.REF: N - F + 1, T.SPEC: N - F}        # proposers at step 0


def merge_starts(mode):
    return [0 if i < MERGE_T0[mode] else 1 for i in range(N)]


MERGE_EXTRA = [dict(t=6, kind="byz", src=63, type=S.ECHO, kp=1, s=0, dst=ALL64)]
MERGE_STEP = 9
MERGE_Q = 8
# the order in which the kernel walks the segments of one step's list (brc_step.h tcls_tb -- restated here, to be kept
# in step with it; "G": the general body, first -- any key with a SEND beside other types, or a restricted SEND)
SEGMENT_ORDER = ("G", "E", "R", "S", "ER")


def delivery_word_walk(exp, q, step, dconst):
    """From an oracle result with send and deliver events, under constant link delays and one key variant: the keys
    that deliver at ``step``, in the order the typed list visits them -- [(segment, key prefix, phase index, key
    word)], segments in SEGMENT_ORDER, ascending slot (q x prefix + phase index mod q) inside a segment.  A key's
    segment follows from the message types landing on it at ``step``: those sent at step - dconst."""
    types = {}
    for t, node, typ, kp, s in exp["events"]["send"]:
        if t == step - dconst:
            types.setdefault((kp, s), set()).add(typ)
    name = {frozenset([S.ECHO]): "E", frozenset([S.READY]): "R", frozenset([S.SEND]): "S",
            frozenset([S.ECHO, S.READY]): "ER"}
    walk = []
    for kp, s in sorted({(k, s) for t, node, k, s in exp["events"]["deliver"] if t == step}):
        slot = kp * q + s % q
        walk.append((name.get(frozenset(types.get((kp, s), ())), "G"), kp, s, slot // 64, slot))
    walk.sort(key=lambda e: (SEGMENT_ORDER.index(e[0]), e[4]))
    return [e[:4] for e in walk]


# staggered starts: replica i proposes at step i % 5, so early steps hold a few keys of a class and some classes none
STARTS = [i % 5 for i in range(N)]


def cases():
    out = []

    def add(name, mode, make, q, consensus=True, count=COUNT):
        inst = ("step", 64, 0, mode, 0)
        out.append(T.Case("typed-" + name, inst, make, count, dict(proposals="inject"), q, consensus=consensus))

    for mode, mn, q in ((T.REF, "ref", 4), (T.SPEC, "spec", 8)):
        add("%s-slow8-cap1" % mn, mode, _cons(mode, T.SLOW, 8, 1, q), q)
        add("%s-slow8-cap3" % mn, mode, _cons(mode, T.SLOW, 8, 3, 8), 8)
        add("%s-unif2-cap1" % mn, mode, _cons(mode, T.UNIF, 2, 1, q), q)
        add("%s-unif4-cap3" % mn, mode, _cons(mode, T.UNIF, 4, 3, 8), 8)
        add("%s-stagger" % mn, mode, _cons(mode, T.SLOW, 8, 1, 8, starts=STARTS), 8)
        add("%s-n33" % mn, mode, _cons(mode, T.SLOW, 8, 1, q, n=33, f=10), q)
        # a Byzantine SEND to ten replicas beside the honest SENDs of the same step, and later beside their ECHOs
        add("%s-kdst" % mn, mode, _brb(mode, [(0, o, 0) for o in range(5)] + [(3, 7, 0)],
                                       extra=restricted_send(60, 0, (1 << 10) - 1) + restricted_send(61, 3, 0x3FF << 20),
                                       model=T.SLOW, dconst=1), 8, consensus=False)
        add("%s-merge" % mn, mode, _cons(mode, T.CONST, 8, 1, MERGE_Q, dconst=3, byzantine=BYZ, starts=merge_starts(mode),
                                         extra=MERGE_EXTRA), MERGE_Q)
    return out


def by_name():
    return {c.name: c for c in cases()}
