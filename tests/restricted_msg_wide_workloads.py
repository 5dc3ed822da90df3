"""Workload table of tests/test_gpu_restricted_msg_wide.py (GPU) and tests/test_restricted_msg_wide_workloads.py (its
preconditions, on the oracle alone): a Byzantine replica ECHOes / READYs a key to a subset of the peers
(include/brc.h, "Restricted ECHO / READY") on the wide step kernels (n > 64) of an engine created with
BRC_FLAG_WIDE_RECORDS.

A case is an interleaved_workloads.Case: 3 instances, consecutive global ids from 777, one configuration, one
workgroup per instance.  n = 70 pads to 128 (two destination words), n = 130 to 256 (three caller words against the
engine's stride of four).  Every instance draws its own destination sets; by local id:

  0  an ECHO and a READY of one key to two subsets at ONE step, from the highest Byzantine replica (id >= 64, at
     n = 130 >= 128); two steps later the same ECHO to every peer: a record over the remaining links
  1  the ECHO to every peer (the cell path), a READY to destinations in the highest word only, then the ECHO again to a
     subset: every link is used, the remainder is empty (accepted, no record, no counter changes)
  2  a READY to Byzantine destinations only (msgs_sent grows, nothing arrives), and an ECHO from the lowest Byzantine
     replica to a subset one step later

GARBAGE: the cases whose GPU injections carry random destination bits at and above n (the engine masks them off).
late: restricted records without a time; Case stamps them with a step at which the instance has arrivals, and the
at_now policy injects them with t == t_now (the re-entered step).
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
    rng = random.Random(0x2E57B000 + salt)
    while True:
        m = rng.getrandbits(n)
        if m != (1 << n) - 1 and all((m >> lo) & ((1 << min(64, n - lo)) - 1) for lo in range(0, n, 64)):
            return m


def top_word(n, salt):
    """A non-empty subset of the replicas of the highest word, never all of them."""
    lo = 64 * ((n - 1) // 64)
    return random.Random(0x2E57C000 + salt).randrange(1, (1 << (n - lo)) - 1) << lo


def msg(t, src, typ, key, dst):
    return dict(t=t, kind="byz", src=src, type=typ, kp=key[0], s=key[1], dst=dst)


def restricted(n, g, i, byz, key, t0):
    """Instance i's pattern (module docstring) on `key`, from step t0."""
    allm = (1 << n) - 1
    lo, hi = min(byz), max(byz)
    A, B = subset(n, 4 * g), subset(n, 4 * g + 1)
    if i == 0:
        return [msg(t0, hi, S.ECHO, key, A), msg(t0, hi, S.READY, key, B), msg(t0 + 2, hi, S.ECHO, key, allm)]
    if i == 1:
        return [msg(t0, hi, S.ECHO, key, allm), msg(t0 + 1, hi, S.READY, key, top_word(n, g)), msg(t0 + 2, hi, S.ECHO, key, A)]
    return [msg(t0, hi, S.READY, key, sum(1 << b for b in byz)), msg(t0 + 1, lo, S.ECHO, key, B)]


def widened(sp):
    """sp with every restricted ECHO / READY sent to all peers instead."""
    allm = (1 << sp["n"]) - 1
    return dict(sp, actions=[dict(a, dst=allm) if a["kind"] == "byz" and a["type"] != S.SEND else a for a in sp["actions"]])


def is_restricted(sp, a):
    return a["kind"] == "byz" and a["type"] != S.SEND and a["dst"] != (1 << sp["n"]) - 1


def table_records(sp):
    """Records the instance's table holds when its actions are injected at once (nothing is pruned then), by
    brc_inject's rules: a Byzantine ECHO / READY over the links its (node, type, key) has not used (restricted, or
    after a restricted one) takes a record, one sender each.  (count, empty remainders)."""
    from oracle.oracle import expand_actions
    allm = (1 << sp["n"]) - 1
    recs, empty, used, hadrec = 0, 0, {}, set()
    for a in expand_actions(sp["actions"], sp["n"]):
        if a["kind"] != "byz" or a["type"] == S.SEND or a["src"] not in sp["byzantine"]:
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


def garbage(n, salt):
    """Random bits at and above n, up to the 256 a destination mask holds."""
    return random.Random(0x2E57D000 + salt).getrandbits(256 - n) << n


BYZ70, BYZ130 = [5, 66, 69], [7, 100, 129]


def _late(n, i, byz, key):
    return [{k: v for k, v in a.items() if k != "t"} for a in restricted(n, OFFSET + i, 0, byz, key, 0)[:2]]


def _build():
    out = []

    def add(name, family, inst, make, consensus, key_window, late=None, byz=()):
        out.append(I.Case(name, family, inst, make, COUNT, key_window, consensus, late=late, byz=byz))

    def brb(n, f, seed, model, dmax, byz, mode=None):
        def make(g, i):
            extra = restricted(n, g, i, byz, (0, 0), 1)
            sends = [(0, 0, 0)]
            if mode == "spec":
                return S.spec_brb_spec(n, f, seed, model, dmax, g, sends, byzantine=byz, extra=extra, window=4)
            if mode == "beb":
                return S.beb_spec(n, seed, model, dmax, g, sends, byzantine=byz, extra=extra)
            return S.brb_spec(n, f, seed, model, dmax, g, sends, byzantine=byz, extra=extra)
        return make

    def cons(n, f, seed, model, dmax, byz, spec=False):
        def make(g, i):
            # ECHOes / READYs of an honest proposal's key (origin 1 + i, proposed at step 0)
            extra = restricted(n, g, i, byz, (1 + i, 0), 1)
            if spec:
                return S.spec_cons_spec(n, f, seed, model, dmax, g, round_cap=1, window=4, byzantine=byz, extra=extra)
            return S.cons_spec(n, f, seed, model, dmax, g, round_cap=1, byzantine=byz, extra=extra)
        return make

    # ---- n = 70: NPAD 128, two destination words
    add("rw-128-ref-brb", "wide128", ("wide", 128, 4, REF, 0), brb(70, 23, 0x2E580070, UNIF, 4, BYZ70), False, 4,
        late={1: _late(70, 1, BYZ70, (0, 0))}, byz=BYZ70)
    add("rw-128-ref-cons", "wide128", ("wide", 128, 8, REF, 0), cons(70, 23, 0x2E581070, SLOW, 8, BYZ70), True, 8, byz=BYZ70)
    add("rw-128-spec-brb", "wide128", ("wide", 128, 4, SPEC, 0), brb(70, 23, 0x2E582070, UNIF, 4, BYZ70, mode="spec"), False, 4,
        byz=BYZ70)
    add("rw-128-beb-brb", "wide128", ("wide", 128, 4, BEB, 0), brb(70, 0, 0x2E583070, UNIF, 4, BYZ70, mode="beb"), False, 4,
        byz=BYZ70)
    # ---- n = 130: NPAD 256; geometric delays up to 16 run the DM = 16 build
    add("rw-256-ref-brb", "wide256", ("wide", 256, 16, REF, 0), brb(130, 43, 0x2E580130, GEO, 16, BYZ130), False, 4,
        late={2: _late(130, 2, BYZ130, (0, 0))}, byz=BYZ130)
    add("rw-256-spec-cons", "wide256", ("wide", 256, 8, SPEC, 0), cons(130, 43, 0x2E581130, SLOW, 5, BYZ130, spec=True), True, 4,
        byz=BYZ130)
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


INTERLEAVED = ("rw-128-ref-brb", "rw-256-ref-brb")
GARBAGE = ("rw-128-ref-cons", "rw-256-ref-brb", "rw-256-spec-cons")


def overflow_spec():
    """n = 70, one instance: at step 1 Byzantine replicas 66 and 69 ECHO and READY the key to a subset each, and so do
    they at steps 2 .. 5 with other sets -- XSEND_MAX + 1 records with a remainder each, injected at once: the last
    finds the table full."""
    n = 70
    extra = []
    for j in range(XSEND_MAX + 1):
        b, typ = (66, 69)[j % 2], (S.ECHO, S.READY)[(j // 2) % 2]
        extra.append(msg(1 + j // 4, b, typ, (0, 0), 1 << (j // 4) | 1 << (64 + j // 4)))
    return dict(S.brb_spec(n, 23, 0x2E5800F0, UNIF, 4, OFFSET, [(0, 0, 0)], byzantine=BYZ70, extra=extra), name="overflow-wide/0",
                step_cap=I.STEP_CAP)


oracle_results = I.oracle_results
