"""Workload table of tests/test_gpu_wide_xsend.py (GPU) and tests/test_wide_xsend_workloads.py (its preconditions, on
the oracle alone): a second SEND of one key (include/brc.h, "Extra SENDs") on the wide step kernels (n > 64) of an
engine created with BRC_FLAG_WIDE_RECORDS.

A case is an interleaved_workloads.Case: 3 instances, consecutive global ids from 777, one configuration, one
workgroup per instance.  n = 70 pads to 128 (two destination words), n = 128 fills its padding, n = 130 pads to 256
(three caller words against the engine's stride of four).  Every instance draws its own senders and destination
sets.  Broadcast cases, by local id (pattern()):

  0  "split": the highest Byzantine replica declares a key and SENDs it to a set A; one step later the middle
     Byzantine replica (above 63; at n = 130 in word 1) SENDs it to a set B that overlaps A, and a step after that the origin SENDs it again to a set C
     (sender peers: only its links C \\ A carry it).  The receivers of (B | C) \\ A get the key from an extra SEND only.
  1  "same-step": an honest origin SENDs its key, a second honest node (in the highest word) SENDs the same payload
     at the same step, and the origin SENDs it again one step later (no link left: accepted, changes nothing).  Where
     the two links to a receiver have one delay, both SENDs land on one cell in one step.
  2  "with-records": an honest origin SENDs its key; at step 1 the highest Byzantine replica SENDs it to a subset and
     ECHOes and READYs it to two other subsets, all at that step.  Best-effort broadcast has no ECHO / READY: there
     the instance repeats "split" with other sets.

The consensus case splits a Byzantine origin's declared phase-0 key over two Byzantine senders (half the peers each);
the wrap case SENDs six sequence numbers of one origin through a key window of four, with extra SENDs on the first and
on the fifth (which reuses the first's slot after its extra SEND has gone quiet).

GARBAGE: the cases whose GPU injections carry random destination bits at and above n (the engine masks them off).
late: instance 1's second honest SEND without a time (and without the origin's repeat); Case stamps it with a step at
which the instance has arrivals, and the at_now policy injects it with t == t_now (the re-entered step).
"""
import random

from tests import interleaved_workloads as I
from tests.golden import specs as S

OFFSET = I.OFFSET
REF, SPEC, BEB = I.REF, I.SPEC, I.BEB
UNIF, SLOW, GEO = I.UNIF, I.SLOW, I.GEO
XSEND_MAX = I.XSEND_MAX
CKEYS = I.CKEYS
COUNT = 3


def subset(n, salt):
    """A proper subset of the n peers with members in every 64-replica word."""
    rng = random.Random(0x2E59B000 + salt)
    while True:
        m = rng.getrandbits(n)
        if m != (1 << n) - 1 and all((m >> lo) & ((1 << min(64, n - lo)) - 1) for lo in range(0, n, 64)):
            return m


def top_word(n, salt):
    """A non-empty subset of the replicas of the highest word, never all of them."""
    lo = 64 * ((n - 1) // 64)
    return random.Random(0x2E59C000 + salt).randrange(1, (1 << (n - lo)) - 1) << lo


def garbage(n, salt):
    """Random bits at and above n, up to the 256 a destination mask holds."""
    return random.Random(0x2E59D000 + salt).getrandbits(256 - n) << n


def send(t, node, key):
    """An honest node's broadcast(SEND) of the payload of `key` (its own, or another origin's)."""
    return dict(t=t, kind="brb_send", node=node, kp=key[0], s=key[1], payload="TEST %d.%d" % (key[0] + 1, key[1]))


def byz(t, src, typ, key, dst):
    return dict(t=t, kind="byz", src=src, type=typ, kp=key[0], s=key[1], dst=dst)


def split(n, g, byzs, t0, salt=0):
    lo, hi = sorted(byzs)[1], max(byzs)          # the second sender: the middle one (at n = 130 in word 1)
    A, B = subset(n, 8 * g + salt), subset(n, 8 * g + salt + 1)
    C = top_word(n, 8 * g + salt) | (subset(n, 8 * g + salt + 2) & ~A)
    assert C & ~A
    return [dict(t=t0, kind="byz_key", kp=hi, s=0, value=0), byz(t0, hi, S.SEND, (hi, 0), A),
            byz(t0 + 1, lo, S.SEND, (hi, 0), B), byz(t0 + 2, hi, S.SEND, (hi, 0), C)]


def pattern(n, g, i, byzs, beb=False):
    """(sends, extra) of instance i (module docstring)."""
    hi = max(byzs)
    if i == 0:
        return [(0, 1, 0)], split(n, g, byzs, 1)
    if i == 1:
        o = g % 5
        high = [x for x in range(n - 1, 64 * ((n - 1) // 64) - 1, -1) if x not in byzs]
        second = high[g % min(3, len(high))]
        return [(0, o, 0)], [send(0, second, (o, 0)), send(1, o, (o, 0))]
    if beb:
        return [(0, 2, 0)], split(n, g, byzs, 2, salt=4)
    key = (0, 0)
    return [(0, 0, 0)], [byz(1, hi, S.SEND, key, subset(n, 8 * g + 5)), byz(1, hi, S.ECHO, key, subset(n, 8 * g + 6)),
                         byz(1, hi, S.READY, key, subset(n, 8 * g + 7))]


def extra_sends(sp):
    """The SENDs of a key SENT before them in sp's action list (time order, list order within a step)."""
    from oracle.oracle import expand_actions
    seen, out = set(), []
    for a in expand_actions(sp["actions"], sp["n"]):
        if a["kind"] == "brb_send" or (a["kind"] == "byz" and a["type"] == S.SEND):
            key = (a["kp"], a["s"])
            if key in seen:
                out.append(a)
            seen.add(key)
    return out


def without_extras(sp):
    """sp with every SEND of a key SENT before removed."""
    ex = extra_sends(sp)
    return dict(sp, actions=[a for a in sp["actions"] if a not in ex])


def table_records(sp):
    """Records the instance's table holds when its actions are injected at once (nothing is pruned then), by
    brc_inject's rules: an extra SEND over the links its node has not used for SENDs of the key, and a Byzantine
    ECHO / READY over the links its (node, type, key) has not used (restricted, or after a restricted one), take a
    record each unless no link is left.  (count, empty remainders)."""
    from oracle.oracle import expand_actions
    allm = (1 << sp["n"]) - 1
    recs, empty, used, hadrec, sent, sused = 0, 0, {}, set(), set(), {}
    for a in expand_actions(sp["actions"], sp["n"]):
        if a["kind"] == "brb_send" or (a["kind"] == "byz" and a["type"] == S.SEND):
            key, node = (a["kp"], a["s"]), a.get("node", a.get("src"))
            dst = a.get("dst", allm) & allm & ~sused.get((node, key), 0)
            sused[(node, key)] = sused.get((node, key), 0) | dst
            if key in sent:
                recs += bool(dst)
                empty += not dst
            sent.add(key)
            continue
        if a["kind"] != "byz" or a["src"] not in sp["byzantine"]:
            continue
        ident = (a["src"], a["type"], a["kp"], a["s"])
        dst = a["dst"] & allm
        if dst != allm or ident in hadrec:
            dst &= ~used.get(ident, 0)
            hadrec.add(ident)
            recs += bool(dst)
            empty += not dst
        used[ident] = used.get(ident, 0) | dst
    return recs, empty


BYZ70, BYZ128, BYZ130 = [5, 66, 69], [9, 70, 127], [7, 100, 129]


def _late(n, i, byzs):
    """Instance i's second honest SEND, without a time."""
    sends, extra = pattern(n, OFFSET + i, 1, byzs)
    return [{k: v for k, v in extra[0].items() if k != "t"}]


def _build():
    out = []

    def add(name, family, inst, make, consensus, key_window, late=None, byzs=()):
        out.append(I.Case(name, family, inst, make, COUNT, key_window, consensus, late=late, byz=byzs))

    def brb(n, f, seed, model, dmax, byzs, mode=None, late=()):
        def make(g, i):
            sends, extra = pattern(n, g, i, byzs, beb=mode == "beb")
            if i in late:                # the second honest SEND comes at_now (Case stamps it), without the repeat
                extra = []
            if mode == "spec":
                return S.spec_brb_spec(n, f, seed, model, dmax, g, sends, byzantine=byzs, extra=extra, window=4)
            if mode == "beb":
                return S.beb_spec(n, seed, model, dmax, g, sends, byzantine=byzs, extra=extra)
            return S.brb_spec(n, f, seed, model, dmax, g, sends, byzantine=byzs, extra=extra)
        return make

    def cons(n, f, seed, model, dmax, byzs):
        def make(g, i):
            # Byzantine origin hi's phase-0 key: to the lower half of the peers from hi itself, to the upper half
            # (split point drawn per instance) from the second Byzantine replica one step later
            lo, hi = min(byzs), max(byzs)
            cut = 30 + (g * 7 + i) % 12
            low, high = (1 << cut) - 1, ((1 << n) - 1) & ~((1 << cut) - 1)
            extra = [dict(t=0, kind="byz_key", kp=hi, s=0, value=1 + i % 2), byz(0, hi, S.SEND, (hi, 0), low),
                     byz(i % 2, lo, S.SEND, (hi, 0), high)]
            return S.cons_spec(n, f, seed, model, dmax, g, round_cap=1, byzantine=byzs, extra=extra)
        return make

    def wrap(n, f, seed, model, dmax, byzs):
        def make(g, i):
            # six sequence numbers of origin i through Q = 4, 16 steps apart; a node above 63 SENDs the first again one step
            # later and the fifth (the first's slot, reused) two steps later
            sends = I.stream(i, 6, 16)
            second = (64, 65, 67)[i]
            extra = [send(1, second, (i, 0)), send(4 * 16 + 2, second, (i, 4)), send(4 * 16 + 3, i, (i, 4))]
            return S.brb_spec(n, f, seed, model, dmax, g, sends, byzantine=byzs, extra=extra)
        return make

    # ---- n = 70: NPAD 128, two destination words
    add("xw-128-ref-brb", "wide128", ("wide", 128, 8, REF, 0), brb(70, 23, 0x2E590070, SLOW, 8, BYZ70, late=(1,)), False, 4,
        late={1: _late(70, 1, BYZ70)}, byzs=BYZ70)
    add("xw-128-ref-unif", "wide128", ("wide", 128, 4, REF, 0), brb(70, 23, 0x2E591070, UNIF, 4, BYZ70), False, 4, byzs=BYZ70)
    add("xw-128-spec-brb", "wide128", ("wide", 128, 4, SPEC, 0), brb(70, 23, 0x2E592070, UNIF, 4, BYZ70, mode="spec", late=(1,)),
        False, 4, late={1: _late(70, 1, BYZ70)}, byzs=BYZ70)
    add("xw-128-beb-brb", "wide128", ("wide", 128, 4, BEB, 0), brb(70, 0, 0x2E593070, UNIF, 4, BYZ70, mode="beb"), False, 4,
        byzs=BYZ70)
    add("xw-128-ref-cons", "wide128", ("wide", 128, 8, REF, 0), cons(70, 23, 0x2E594070, SLOW, 8, BYZ70), True, 8, byzs=BYZ70)
    add("xw-128-ref-wrap", "wide128", ("wide", 128, 8, REF, 0), wrap(70, 23, 0x2E595070, SLOW, 8, BYZ70), False, 4, byzs=BYZ70)
    # ---- n = 128 = NPAD: sender 127, garbage at and above n
    add("xw-128full-ref-brb", "wide128", ("wide", 128, 8, REF, 0), brb(128, 42, 0x2E590128, SLOW, 8, BYZ128), False, 4,
        byzs=BYZ128)
    # ---- n = 130: NPAD 256; geometric delays up to 16 run the DM = 16 build
    add("xw-256-ref-brb", "wide256", ("wide", 256, 16, REF, 0), brb(130, 43, 0x2E590130, GEO, 16, BYZ130, late=(1,)), False, 4,
        late={1: _late(130, 1, BYZ130)}, byzs=BYZ130)
    add("xw-256-spec-brb", "wide256", ("wide", 256, 4, SPEC, 0), brb(130, 43, 0x2E591130, UNIF, 4, BYZ130, mode="spec"), False, 4,
        byzs=BYZ130)
    assert len({c.name for c in out}) == len(out)
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


def by_name():
    return {c.name: c for c in cases()}


INTERLEAVED = ("xw-128-ref-brb", "xw-128-spec-brb", "xw-256-ref-brb")
GARBAGE = ("xw-128-ref-unif", "xw-128full-ref-brb", "xw-256-ref-brb")


def overflow_spec():
    """n = 70, one instance: origin 0 SENDs its key, and XSEND_MAX + 1 other nodes (on both sides of replica 64) SEND
    it again, four per step from step 1 -- records with links each, injected at once: the last finds the table full."""
    nodes = [x for x in range(1, 12) if x not in BYZ70][:8] + [x for x in range(58, 70) if x not in BYZ70][:XSEND_MAX + 1 - 8]
    assert all(b not in BYZ70 for b in nodes) and max(nodes) >= 64
    extra = [send(1 + j // 4, b, (0, 0)) for j, b in enumerate(nodes)]
    return dict(S.brb_spec(70, 23, 0x2E5900F0, UNIF, 4, OFFSET, [(0, 0, 0)], byzantine=BYZ70, extra=extra), name="overflow-xsend/0",
                step_cap=I.STEP_CAP)


oracle_results = I.oracle_results
