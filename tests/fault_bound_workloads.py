"""Workload table of tests/test_gpu_fault_bounds.py (GPU) and tests/test_fault_bound_workloads.py (its preconditions, on
the oracle alone): fault bounds off f = (n - 1) // 3 -- 0, (n - 1) // 3 + 1, ceil(n / 2), n - 1 -- and committees below 4
on every kernel family.

Every kernel header restates the four quorum comparisons (> n - f, 2 * count > n + f, > 2 * f, > f) inline, and f is also
the size of the slow set, from which the two-class lifetime kernels derive their receiver classes.  The other tables
run f = (n - 1) // 3 (a few f = 0 rows aside), where a slip in one restatement can coincide with the oracle.

A case is one batch, one configuration (n, f, mode, delays, round cap, key window), COUNT instances with consecutive
global ids from 777; step_noevent_workloads' Case, instantiation() and oracle cache are reused.  Each family row of the
grid gets one case per (n, f) shape, the row's modes going round the shapes so that every mode of the row runs (a full
shapes x modes product would be some 110 batches; the thresholds sit in the header, which every mode of a row shares):

  packed4     NPAD 4            (1,0) (2,0) (2,1) (3,0) (3,2) (4,3)                  REF BRB, REF consensus, SPEC, BEB consensus
  packed      NPAD 8 / 16 / 32  (7,0) (7,3) (7,6) (16,8) (16,15) (29,0) (29,14)      REF consensus, SPEC, connection peers; masks
  lean        n in 33..64       (40,0) (40,14) (40,20) (64,32) (64,63)               REF, SPEC, BEB (step kernel)
  general64   NPAD 64           (40,0) (40,20)                                       general keys, connection peers
  life        two-class         (40,0) (40,39) (64,32)                               REF, SPEC, BEB, connection; masks
  life-pl     per-link, D = 12  (50,0) (50,25)                                       SPEC, connection
  wide        n > 64, step      (70,0) (70,24) (70,35) (130,65) (130,129)            REF, SPEC, BEB; one with wide_records
  wide-life   BRC_FLAG_WIDE_LIFE  (70,0) (70,35) (70,69) (130,65)                    REF, SPEC, BEB
  pattern     BRC_FLAG_LIFE_PATTERN  (70,24) (70,35)                                 REF, variants 2

Nothing of the grid is refused by the planner.

masks: the instances carry different silent Byzantine sets (brc_load_byzantine), different within every packed wave
item; at f = n - 1 a third of the instances have the ONE fast replica Byzantine (no fast class is left).

Regimes (tests/test_fault_bound_workloads.py checks each on the oracle):
  unreachable  2 f + 1 exceeds the honest replicas: no READY quorum under the reference and SPEC broadcasts, nothing is
               delivered (the best-effort broadcast has no quorum and delivers all the same);
  second       a phase ends on a replica's second delivery: n - f = 2 under SPEC (n - f distinct origins), n - f = 1
               under the reference's consensus (its count must EXCEED n - f), which only the best-effort broadcast
               can feed -- above n = 1 f = n - 1 is unreachable for the two others;
  trickle      under the two-class delay models a SPEC phase's deliveries land at one step at every replica once f exceeds
               the standard bound (every quorum then needs the slow replicas), so the count jumps past n - f and
               past n - (n - 1) // 3 together; the per-link cases one above the standard bound (p32-n29f14-spec,
               wide-n70f24-spec, lifepl-n50f17-spec: uniform delays) are the ones whose counts pass between the two;
  step cap     SPEC one above the standard bound keeps proposing "-1" and flipping the coin (f + 1 faults are more than
               it tolerates): those batches stop at a step cap of 60 .. 400, a stop every kernel must place alike;
  stall        reference / best-effort consensus at f = 0: n origins give n deliveries, the count never exceeds n - f = n,
               so no phase ends (the ">" a ">=" would break).  These cases, and the unreachable ones, are the
               consensus cases without a phase end; every other consensus case has one;
  f = 0        no slow replica; f = n - 1: exactly one fast replica, in every instance.

The engine's key window: the oracle does not model BRC_OVERFLOW under the reference and best-effort protocols, so
every case but three has a window that holds the oracle's largest count of live phases per origin
(wide_window_workloads.needs).  The three named *-ovf (one per step-kernel family: packed, lean, wide) are chosen the
other way: a window of 2 under a round cap of 3, where needs() exceeds the window.
"""
import random

from tests import step_noevent_workloads as T
from tests.golden import specs as S

OFFSET = T.OFFSET
COIN = T.COIN
REF, SPEC, BEB, CONN, XREF = T.REF, T.SPEC, T.BEB, T.CONN, T.XREF
CONST, UNIF, SLOW, GEO = T.CONST, T.UNIF, T.SLOW, T.GEO
CKEYS = ("status", "t_stop", "msgs_sent", "arrivals", "cell_steps")
STEP_CAP = 400
XREF_PATS = [[4] * 30 + [1, 2, 3, 5] * 2 + [5, 5], [1, 2, 3, 4, 5] * 8, [5] * 29 + [1, 2, 3, 4] * 2 + [4, 3, 2]]


def standard(n):
    return (n - 1) // 3


def fast_replica(n, seed, model, dmax, g):
    """The one replica outside the slow set at f = n - 1."""
    from oracle.schedule import Schedule
    return (Schedule(n, n - 1, seed, model, dmax, 1).slow_offset(g) + n - 1) % n


def count_for(n):
    """NPAD 4: two full wave items and a tail (33); NPAD 8 / 16 / 32: 17, whole items and a tail; else 16."""
    npad = T.pick_npad(n)
    return 16 if npad >= 64 else 33 if npad == 4 else 17


class FCase(T.Case):
    """T.Case plus: family, kind (the GPU runner: "step", "records", "life", "wide_life", "pattern"), mode, n, f, q,
    masks (per-instance Byzantine lists, loaded with brc_load_byzantine; None: none), overflow, tags."""

    def __init__(self, name, family, kind, mode, n, f, model, dmax, q, round_cap=1, protocol="consensus", masks=False,
                 overflow=False, bump=0, nv=1, step_cap=STEP_CAP, tags=()):
        self.family, self.kind, self.mode, self.n, self.f, self.q = family, kind, mode, n, f, q
        self.model, self.dmax, self.round_cap, self.nv = model, dmax, round_cap, nv
        self.overflow, self.tags = overflow, set(tags)
        self.seed = seed = 0xFB0D0000 + sum(map(ord, name)) * 0x10 + 0x100000 * bump
        count = count_for(n)
        self.masks = self._draw_masks(name, count) if masks else None
        consensus = protocol == "consensus"
        kw = dict(dconst=dmax) if model == CONST else {}
        case = self

        def make(g, f=f, byz=None):
            byz = list(case.masks[g - OFFSET]) if (byz is None and case.masks) else list(byz or ())
            if kind == "pattern":
                return S.cons_spec(n, f, seed, model, dmax, g, round_cap=round_cap, byzantine=byz, nv=nv,
                                   extra=S.equivocation_actions(n, byz, nv=nv), step_cap=step_cap, **kw)
            if not consensus:
                rng = random.Random(seed * 131 + g)
                honest = [o for o in range(n) if o not in byz]
                sends = [(rng.randint(0, 3), o, 0) for o in rng.sample(honest, min(len(honest), 3))]
                return T._brb(mode, n, f, seed, model, dmax, g, sends, byzantine=byz, step_cap=step_cap, **kw)
            if mode == XREF:
                return dict(S.cons_spec(n, f, seed, model, dmax, g, round_cap=round_cap, proposals=XREF_PATS[g % 3],
                                        byzantine=byz, step_cap=step_cap, **kw), values=S.VALUES8, general_keys=True)
            sp = T._cons(mode, n, f, seed, model, dmax, g, round_cap, q, byzantine=byz, nv=nv, step_cap=step_cap, **kw)
            return dict(sp, wide_records=True) if kind == "records" else sp
        self.make_f = make
        run = dict(proposals="loaded" if mode == XREF else "philox" if consensus else "inject")
        sp0 = make(OFFSET)
        if kind in ("life", "wide_life", "pattern"):
            inst = (kind, T.pick_npad(n), T.pick_dm(dmax), mode, 0)
        else:
            inst = T.instantiation(sp0, q)
            if kind == "records":
                inst = inst[:4] + (0,)
        T.Case.__init__(self, name, inst, make, count, run, q, consensus=consensus, constant=model == CONST)
        self.cfg_byz = [] if not self.masks else next(m for m in ([1, 2], [0, 1], [0], [2, 3]) if m not in self.masks and max(m) < n)

    def _draw_masks(self, name, count):
        """Silent sets of 0 .. 2 replicas, the neighbours of every wave item different; at f = n - 1 every third
        instance has exactly its fast replica Byzantine."""
        n, f = self.n, self.f
        rng = random.Random("fault-bounds/" + name)
        ipw = max(1, 64 // T.pick_npad(n))
        out = []
        for i in range(count):
            while True:
                if f == n - 1 and i % 3 == 1:
                    m = [fast_replica(n, self.seed, self.model, self.dmax, OFFSET + i)]
                elif self.kind == "pattern":
                    m = sorted(rng.sample(range(n), rng.randint(1, 3)))
                else:
                    m = sorted(rng.sample(range(n), rng.randint(0, min(2, n - 1))))
                if i % ipw == 0 or m != out[-1] or ipw == 1:
                    break
            out.append(m)
        return out

    def oracle_ids(self):
        """n <= 64: every instance; else the first, the last and two seeded ids between them."""
        if self.n <= 64:
            return list(range(self.count))
        rng = random.Random("fault-bounds/ids/" + self.name)
        return sorted({0, self.count - 1} | set(rng.sample(range(1, self.count - 1), 2)))

    def standard_spec(self, i):
        """Instance i under f = (n - 1) // 3, everything else (its Byzantine list included) the same."""
        return dict(self.make_f(OFFSET + i, f=standard(self.n)), name="%s/%d/std" % (self.name, i))

    def byz(self, i):
        return self.specs[i]["byzantine"]

    def open_kw(self, **kw):
        out = dict(self.run, key_window=self.key_window, **kw)
        if self.masks:
            out.update(load_masks=True, cfg_byzantine=self.cfg_byz)
        return out

    def unreachable(self, i):
        """No READY quorum in instance i: 2 f + 1 exceeds its honest replicas (a best-effort broadcast has none)."""
        return self.mode != BEB and 2 * self.f + 1 > self.n - len(self.byz(i))

    def second(self):
        """A phase ends on a replica's second delivery (module docstring)."""
        if not self.consensus:
            return False
        return (self.mode == SPEC and self.n - self.f == 2) or (self.mode == BEB and self.n - self.f == 1)

    def stalls(self):
        """Reference / best-effort consensus at f = 0 without a second key variant: no phase can end."""
        return self.consensus and self.mode != SPEC and self.f == 0 and self.kind != "pattern"


def _build():
    out = []

    def add(*a, **kw):
        out.append(FCase(*a, **kw))
    # ---- packed NPAD 4
    add("p4-n1f0-brb", "packed4", "step", REF, 1, 0, SLOW, 3, 4, protocol="brb")
    add("p4-n1f0-ref", "packed4", "step", REF, 1, 0, UNIF, 3, 8)
    add("p4-n2f0-ref", "packed4", "step", REF, 2, 0, SLOW, 2, 8, round_cap=2)
    add("p4-n2f1-spec", "packed4", "step", SPEC, 2, 1, SLOW, 3, 4, round_cap=2)
    add("p4-n2f1-beb", "packed4", "step", BEB, 2, 1, SLOW, 3, 8, round_cap=2)
    add("p4-n3f0-spec", "packed4", "step", SPEC, 3, 0, UNIF, 3, 4, round_cap=2)
    add("p4-n3f0-beb", "packed4", "step", BEB, 3, 0, SLOW, 3, 8)
    add("p4-n3f2-beb", "packed4", "step", BEB, 3, 2, SLOW, 2, 8, round_cap=2)
    add("p4-n3f2-brb", "packed4", "step", REF, 3, 2, SLOW, 3, 4, protocol="brb")
    add("p4-n4f3-spec", "packed4", "step", SPEC, 4, 3, SLOW, 4, 4)
    add("p4-n4f3-beb", "packed4", "step", BEB, 4, 3, SLOW, 2, 8, round_cap=2)
    add("p4-n3f1-spec", "packed4", "step", SPEC, 3, 1, SLOW, 3, 8, round_cap=2)          # n - f = 2: the second delivery
    # ---- packed NPAD 8 / 16 / 32, masks
    add("p8-n7f0-ref", "packed", "step", REF, 7, 0, SLOW, 4, 8, round_cap=2, masks=True)
    add("p8-n7f3-spec", "packed", "step", SPEC, 7, 3, SLOW, 4, 8, round_cap=2, masks=True)
    add("p8-n7f3-ref", "packed", "step", REF, 7, 3, SLOW, 3, 8, round_cap=2, masks=True)
    add("p8-n7f6-conn", "packed", "step", CONN, 7, 6, SLOW, 4, 8, masks=True)
    add("p16-n16f8-spec", "packed", "step", SPEC, 16, 8, SLOW, 5, 4, masks=True)
    add("p16-n16f15-ref", "packed", "step", REF, 16, 15, SLOW, 6, 8, masks=True)
    add("p32-n29f0-spec", "packed", "step", SPEC, 29, 0, SLOW, 8, 4, round_cap=2, masks=True)
    add("p32-n29f14-ref", "packed", "step", REF, 29, 14, SLOW, 4, 8, masks=True)
    add("p32-n29f14-spec", "packed", "step", SPEC, 29, 14, UNIF, 3, 8, masks=True, step_cap=100)
    add("p8-n7f3-ref-ovf", "packed", "step", REF, 7, 3, SLOW, 3, 2, round_cap=3, overflow=True)
    # ---- lean n in 33..64, the step kernel
    add("lean-n40f0-spec", "lean", "step", SPEC, 40, 0, SLOW, 4, 4)
    add("lean-n40f14-ref", "lean", "step", REF, 40, 14, SLOW, 4, 8)
    add("lean-n40f14-beb", "lean", "step", BEB, 40, 14, UNIF, 3, 8, round_cap=2)
    add("lean-n40f14-spec", "lean", "step", SPEC, 40, 14, SLOW, 4, 4, step_cap=60)
    add("lean-n40f20-spec", "lean", "step", SPEC, 40, 20, SLOW, 6, 4)
    add("lean-n64f32-ref", "lean", "step", REF, 64, 32, SLOW, 8, 8)
    add("lean-n64f63-ref", "lean", "step", REF, 64, 63, SLOW, 5, 8)
    add("lean-n40f0-beb", "lean", "step", BEB, 40, 0, SLOW, 5, 8)
    add("lean-n40f14-ref-ovf", "lean", "step", REF, 40, 14, SLOW, 3, 2, round_cap=3, overflow=True)
    # ---- general keys and connection peers at NPAD 64
    add("gen-n40f0-xref", "general64", "step", XREF, 40, 0, SLOW, 4, 8)
    add("gen-n40f20-xref", "general64", "step", XREF, 40, 20, SLOW, 4, 8)
    add("conn-n40f0", "general64", "step", CONN, 40, 0, SLOW, 6, 8)
    add("conn-n40f20", "general64", "step", CONN, 40, 20, SLOW, 6, 8)
    # ---- key-lifetime kernel, two-class, masks
    add("life-n40f0-ref", "life", "life", REF, 40, 0, SLOW, 5, 8, masks=True)
    add("life-n40f0-spec", "life", "life", SPEC, 40, 0, CONST, 2, 8, round_cap=2, masks=True)
    add("life-n40f14-spec", "life", "life", SPEC, 40, 14, SLOW, 5, 8, masks=True, step_cap=60)
    add("life-n40f39-spec", "life", "life", SPEC, 40, 39, SLOW, 5, 8, masks=True)
    add("life-n40f0-beb", "life", "life", BEB, 40, 0, SLOW, 5, 8, masks=True)
    add("life-n40f39-conn", "life", "life", CONN, 40, 39, SLOW, 4, 8, masks=True)
    add("life-n64f32-spec", "life", "life", SPEC, 64, 32, SLOW, 8, 8, masks=True)
    add("life-n64f32-beb", "life", "life", BEB, 64, 32, CONST, 2, 8, round_cap=2, masks=True)
    # ---- key-lifetime kernel, per-link, uniform D = 12
    add("lifepl-n50f0-spec", "life-pl", "life", SPEC, 50, 0, UNIF, 12, 8)
    add("lifepl-n50f25-conn", "life-pl", "life", CONN, 50, 25, GEO, 12, 8)
    add("lifepl-n50f25-spec", "life-pl", "life", SPEC, 50, 25, UNIF, 12, 8)
    add("lifepl-n50f17-spec", "life-pl", "life", SPEC, 50, 17, UNIF, 12, 8, step_cap=100)
    add("lifepl-n50f0-conn", "life-pl", "life", CONN, 50, 0, GEO, 12, 8)
    # ---- wide step kernels
    add("wide-n70f0-spec", "wide", "step", SPEC, 70, 0, SLOW, 4, 4)
    add("wide-n70f24-ref", "wide", "step", REF, 70, 24, SLOW, 6, 8)
    add("wide-n70f24-ref-rec", "wide", "records", REF, 70, 24, SLOW, 6, 4, nv=2)
    add("wide-n70f35-ref", "wide", "step", REF, 70, 35, SLOW, 8, 8)
    add("wide-n70f24-beb", "wide", "step", BEB, 70, 24, SLOW, 4, 8)
    add("wide-n70f24-spec", "wide", "step", SPEC, 70, 24, UNIF, 4, 4, step_cap=60)
    add("wide-n130f65-spec", "wide", "step", SPEC, 130, 65, SLOW, 5, 4)
    add("wide-n130f129-ref", "wide", "step", REF, 130, 129, SLOW, 4, 8)
    add("wide-n70f24-ref-ovf", "wide", "step", REF, 70, 24, SLOW, 3, 2, round_cap=3, overflow=True)
    # ---- wide key-lifetime kernel
    add("wlife-n70f0-spec", "wide-life", "wide_life", SPEC, 70, 0, SLOW, 4, 8)
    add("wlife-n70f35-ref", "wide-life", "wide_life", REF, 70, 35, SLOW, 8, 8)
    add("wlife-n70f69-ref", "wide-life", "wide_life", REF, 70, 69, SLOW, 4, 8)
    add("wlife-n130f65-beb", "wide-life", "wide_life", BEB, 130, 65, SLOW, 5, 8)
    add("wlife-n70f24-spec", "wide-life", "wide_life", SPEC, 70, 24, SLOW, 4, 8, step_cap=60)
    add("wlife-n70f24-ref", "wide-life", "wide_life", REF, 70, 24, SLOW, 6, 8)
    # ---- wide key-lifetime kernel, pattern form, variants 2
    add("pat-n70f24-ref", "pattern", "pattern", REF, 70, 24, SLOW, 4, 4, nv=2, masks=True)
    add("pat-n70f35-ref", "pattern", "pattern", REF, 70, 35, SLOW, 4, 4, nv=2, masks=True)
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


# run(3) slices, and brc_reset_at to another offset (best-effort consensus: a replica decides when its own deliveries
# come in, so the records follow the instance's slow set; the reference-protocol batches decide "-1" at one step whatever the id)
SLICED = {"packed": "p8-n7f3-spec", "wide": "wide-n70f24-beb"}


# ---- the oracle, once per spec ------------------------------------------------------------------------------------
_ORACLE = {}
_STD = {}
VID = T.VID


def _pool(fn, items):
    import concurrent.futures
    with concurrent.futures.ThreadPoolExecutor(8) as ex:
        return list(ex.map(fn, items))


def oracle_results(case):
    """{local id: (result with canonically sorted deliver / decide / send lists, per replica [(round, t, value id) of
    every decide event], deliver count)} of the compared ids."""
    from oracle import oracle
    from tests import golden_io
    ids = case.oracle_ids()
    todo = [i for i in ids if (case.name, i) not in _ORACLE]
    for i, exp in zip(todo, _pool(lambda i: oracle.run(case.specs[i]), todo)):
        dec = {}
        for t, node, rnd, val in sorted(exp["events"]["decide"], key=lambda r: (r[0], r[1], r[2])):
            dec.setdefault(node, []).append((rnd, t, VID[val]))
        exp["events"] = golden_io.canonical_events(exp["events"])
        _ORACLE[(case.name, i)] = (exp, dec, exp["counts"]["deliver"])
    return {i: _ORACLE[(case.name, i)] for i in ids}


def summary(exp):
    """Every field of the instance and replica records the oracle gives: the counters and the decide events."""
    return tuple(exp[k] for k in CKEYS) + (exp["counts"]["deliver"], tuple(map(tuple, sorted(exp["events"]["decide"], key=str))))


def all_summaries(case, std=False):
    """summary() of EVERY instance (not only the compared ids), under the case's f or under f = (n - 1) // 3."""
    from oracle import oracle
    key = (case.name, std)
    if key not in _STD:
        specs = [case.standard_spec(i) for i in range(case.count)] if std else case.specs
        _STD[key] = [summary(r) for r in _pool(lambda sp: oracle.run(sp, kinds=("decide",)), specs)]
    return _STD[key]


def expected_read_side(case, res):
    """(round_histogram(66), decisions() counts by value id, undecided, disagreements) over the instances of res."""
    hist, counts, undecided, dis = [0] * 66, {}, 0, 0
    for i, (_exp, dec, _d) in res.items():
        hon = [d for d in range(case.n) if d not in case.byz(i)]
        firsts = [dec[d][0] for d in hon if d in dec]
        undecided += len(hon) - len(firsts)
        for (_r, _t, v) in firsts:
            counts[v] = counts.get(v, 0) + 1
        dis += len({v for (_r, _t, v) in firsts}) > 1
        hist[min(max(r for (r, _t, _v) in firsts), 65) if len(firsts) == len(hon) else 0] += 1
    return hist, counts, undecided, dis
