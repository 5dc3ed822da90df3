"""Workload table of tests/test_gpu_wide_values.py (GPU) and tests/test_wide_values_workloads.py (its preconditions, on
the oracle alone): three-bit consensus value ids (seven proposal strings besides "-1") on the wide step kernels
(n > 64) of an engine created with BRC_FLAG_WIDE_VALUES.

A case is an interleaved_workloads.Case: 3 instances, consecutive global ids from 777, one configuration, one
workgroup per instance, ``values = VALUES8``, round cap 1.  The proposals are loaded (brc_load_proposals), every other
action is injected.  n = 70 pads to 128, n = 128 fills its padding, n = 130 pads to 256; delays up to 4 / 8 / 16 pick
the DM = 4 / 8 / 16 builds.  The reference protocol gets slow-set or geometric delays (uniform ones stall its
broadcast).  f is small against n wherever a decision is to carry a value: with f = n / 3 the reference's windows
(n - f + 1 deliveries, 2 |hosts| > n + f) end in "-1" whatever is proposed.

  wv-128-maj        n = 70   DM 8   REF  a majority of one new id (4 .. 7, by instance), every other id present
  wv-128full-eight  n = 128  DM 4   REF  all eight ids proposed, id 0 ("-1") among them, id 4 by a majority: a replica's
                                         first window holds eight ids (`order` is full)
  wv-128-smallf     n = 70   DM 16  REF  f = 5: ids 5, 6 and 7 are proposed by a third each, so every replica ends
                                         phase 1 with "-1" (id 0).  At that step every third replica is handed id 6
                                         from 12 hosts by direct deliver() calls: in its phase 2 ids 6 and 0 both pass
                                         2 |hosts| > 4 f and id 6, inserted first, decides against the 60 and more
                                         hosts of id 0 (a phase-0 key that lands after the phase's end leaves its id
                                         below the bound)
  wv-256-deliver    n = 130  DM 4   BEB  direct deliver() calls (BRC_INJ_DELIVER) carrying ids 4 .. 7 on top of a
                                         majority of id 7
  wv-256-byzkey     n = 130  DM 16  REF  Byzantine origins declare a phase-0 key of value 6 and SEND it, beside a
                                         majority of id 6 among the honest proposals
  wv-128-both       n = 70   DM 8   REF  both flags: a majority of id 5, and a Byzantine replica ECHOes an honest
                                         origin's phase-0 key to a subset of the peers (a record)
  wv-128full-beb    n = 128  DM 8   BEB  a majority of one new id over best-effort broadcast

fold(sp) is sp with every value id taken ``& 3`` -- what a kernel that kept two bits would run.
"""
import copy
import random

from tests import interleaved_workloads as I
from tests.golden import specs as S

OFFSET = I.OFFSET
REF, BEB = I.REF, I.BEB
UNIF, SLOW, GEO = I.UNIF, I.SLOW, I.GEO
CKEYS = I.CKEYS
COUNT = 3
BYZ70, BYZ128, BYZ130 = [5, 66, 69], [9, 70, 127], [7, 100, 129]


def majority(n, g, major, share, others):
    """n proposals: `share` of them the id `major`, the rest cycling through `others`; shuffled per instance."""
    pat = [major] * share + [others[j % len(others)] for j in range(n - share)]
    random.Random(0x3B17A000 + g).shuffle(pat)
    return pat


def fold(sp):
    out = copy.deepcopy(sp)
    for a in out["actions"]:
        if "value" in a:
            a["value"] &= 3
    return out


def _cons(n, f, seed, model, dmax, byzs, pat, extra=None, beb=False):
    def make(g, i):
        ex = extra(g, i) if extra else []
        mk = S.beb_cons_spec if beb else S.cons_spec
        return dict(mk(n, f, seed, model, dmax, g, round_cap=1, proposals=pat(g, i), byzantine=byzs, extra=ex), values=S.VALUES8)
    return make


def _build():
    out = []

    def add(name, family, inst, make, byzs, both=False):
        c = I.Case(name, family, inst, make, COUNT, 8, True, byz=byzs)
        c.both = both                 # the engine is created with BRC_FLAG_WIDE_RECORDS as well
        out.append(c)

    rest = lambda m: [v for v in range(8) if v != m]                     # noqa: E731
    add("wv-128-maj", "wide128", ("wide", 128, 8, REF, 0),
        _cons(70, 5, 0x3B170070, SLOW, 8, BYZ70, lambda g, i: majority(70, g, 4 + (g + i) % 4, 56, rest(4 + (g + i) % 4))), BYZ70)
    add("wv-128full-eight", "wide128", ("wide", 128, 4, REF, 0),
        _cons(128, 10, 0x3B170128, SLOW, 4, BYZ128, lambda g, i: majority(128, g, 4, 93, rest(4))), BYZ128)

    def early_six(g, i):
        # the step at which replica 0 (as every replica: the keys deliver in bursts) ends phase 1, from the oracle's run
        # without the calls; the calls are actions of that step, performed after its messages
        from oracle import oracle
        base = smallf(g, i)
        t1 = sorted(e[0] for e in oracle.run(base, kinds=("deliver",))["events"]["deliver"] if e[1] == 0)[70 - 5]
        return [dict(t=t1, kind="deliver", node=d, kp=h, value=6) for d in range(0, 70, 3) if d not in BYZ70 for h in range(10, 22)]
    smallf = _cons(70, 5, 0x3B171070, GEO, 16, BYZ70, lambda g, i: majority(70, g, 5, 24, [6, 7]))
    add("wv-128-smallf", "wide128", ("wide", 128, 16, REF, 0),
        _cons(70, 5, 0x3B171070, GEO, 16, BYZ70, lambda g, i: majority(70, g, 5, 24, [6, 7]), extra=early_six), BYZ70)

    def delivers(g, i):
        rng = random.Random(0x3B17D000 + g)
        hon = [d for d in range(130) if d not in BYZ130]
        return [dict(t=rng.randint(0, 3), kind="deliver", node=rng.choice(hon), kp=rng.randrange(130), value=rng.randint(4, 7))
                for _ in range(60)]
    add("wv-256-deliver", "wide256", ("wide", 256, 4, BEB, 0),
        _cons(130, 20, 0x3B170130, UNIF, 4, BYZ130, lambda g, i: majority(130, g, 7, 100, rest(7)), extra=delivers, beb=True), BYZ130)

    def byzkey(g, i):
        allm = (1 << 130) - 1
        acts = []
        for b in BYZ130:
            acts += [dict(t=0, kind="byz_key", kp=b, s=0, value=6), dict(t=0, kind="byz", src=b, type=S.SEND, kp=b, s=0, dst=allm)]
        return acts
    add("wv-256-byzkey", "wide256", ("wide", 256, 16, REF, 0),
        _cons(130, 8, 0x3B171130, GEO, 16, BYZ130, lambda g, i: majority(130, g, 6, 100, rest(6)), extra=byzkey), BYZ130)

    def restricted(g, i):
        rng = random.Random(0x3B17E000 + g)
        dst = rng.getrandbits(70) | 1 | 1 << 65
        return [dict(t=1, kind="byz", src=69, type=S.ECHO, kp=g % 5 if g % 5 not in BYZ70 else 0, s=0, dst=dst & ~(1 << 3))]
    add("wv-128-both", "wide128", ("wide", 128, 8, REF, 0),
        _cons(70, 5, 0x3B172070, SLOW, 8, BYZ70, lambda g, i: majority(70, g, 5, 56, rest(5)), extra=restricted), BYZ70, both=True)
    add("wv-128full-beb", "wide128", ("wide", 128, 8, BEB, 0),
        _cons(128, 10, 0x3B173128, SLOW, 8, BYZ128, lambda g, i: majority(128, g, 5 + (g + i) % 3, 100, rest(5 + (g + i) % 3)), beb=True),
        BYZ128)
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


SLICED = ("wv-128full-eight", "wv-256-deliver")
RESET_AT = "wv-128-smallf"
oracle_results = I.oracle_results
expected_read_side = I.expected_read_side


def replay(sp, exp):
    """core/byzantinerandomizedconsensus.py:53-106 replayed over the oracle's DELIVER events of a reference-protocol
    consensus spec (processing order: step, receiver, key; a step's direct deliver() calls after its messages, in list
    order): per replica the value table in insertion order and the host sets.  Returns (decide events [t, node, round,
    value id], the most ids one replica held in one window, per decision the ids with 2 |hosts| above the phase-2 bound)."""
    n, f = sp["n"], sp["f"]
    t_cnt, b1, b2 = n - f + 1, n + f, 4 * f
    value = {(a["node"], 0): a["value"] for a in sp["actions"] if a["kind"] == "propose"}
    value.update({(a["kp"], a["s"]): a["value"] for a in sp["actions"] if a["kind"] == "byz_key"})
    st = {d: dict(round=1, phase=1, order=[], hosts={}, count=0) for (d, _s) in value if d not in sp["byzantine"]}
    decides, widest, above = [], 0, []

    def best(r, bound):
        return next((v for v in r["order"] if 2 * len(r["hosts"][v]) > bound), 0)

    calls = [(a["t"], 1, j) for j, a in enumerate(sp["actions"]) if a["kind"] == "deliver"]
    for item in sorted([(t, 0, (d, kp, s)) for t, d, kp, s in exp["events"]["deliver"]] + calls):
        t = item[0]
        if item[1]:
            a = sp["actions"][item[2]]
            d, kp, v = a["node"], a["kp"], a["value"]
        else:
            d, kp, s = item[2]
            v = value[(kp, s)]
        r = st[d]
        if v not in r["order"]:
            r["order"].append(v)
            r["hosts"][v] = set()
        r["hosts"][v].add(kp)
        r["count"] += 1
        widest = max(widest, len(r["order"]))
        if r["count"] >= t_cnt and r["phase"] == 1:
            value[(d, 2 * (r["round"] - 1) + 1)] = best(r, b1)
            r.update(phase=2, order=[], hosts={}, count=0)
        if r["count"] >= t_cnt and r["phase"] == 2:
            dec = best(r, b2)
            above.append([v for v in r["order"] if 2 * len(r["hosts"][v]) > b2])
            decides.append([t, d, r["round"], dec])
            r.update(round=r["round"] + 1, phase=1, order=[], hosts={}, count=0)
            value[(d, 2 * (r["round"] - 1))] = dec
    return decides, widest, above
