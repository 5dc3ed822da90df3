"""Workload table of tests/test_gpu_byz_masks.py (GPU) and tests/test_byz_mask_workloads.py (its preconditions,
on the oracle alone): batches whose instances carry DIFFERENT Byzantine masks, loaded with brc_load_byzantine
(include/brc.h).  Every other parity test passes one byzantine= list through brc_config, so the per-instance
mask reads of the kernels (brc_step.h: P.byz[inst] of the lane's own segment; brc_step_wide.h: P.byz[inst * NW +
wid]; brc_life.h: the class sizes nHF / nHS), of expand_equivocate and of the read side (round_histogram,
decision_histogram, brc_read_instances' decided, brc_read_stats) have only seen identical masks.

A case: name, specs (harness format, consecutive global ids from OFFSET = 777; spec i carries its own
"byzantine" list), inst (the step-kernel instantiation brc_create picks, step_noevent_workloads.instantiation),
kernel ("life": the batch also runs on the key-lifetime kernel), life (the lifetime kernel's form), run / key_window
(engine_runner.open_batch keywords), cfg_byz (the engine's configuration mask: non-empty and equal to none of the
loaded masks, which replace it) and garbage (a seed: the loaded words carry random bits at and above n).

Mask rules (test_byz_mask_workloads.py checks them):
  * n <= 64 (count >= 5): the masks of a case include the empty set, {0}, {n - 1} and a set of the largest size
    that still decides: f - 1 silent replicas under the reference and BEB protocols (a phase ends on n - f + 1
    deliveries), f under SPEC and BRB;
  * reference-protocol (and BEB) consensus cases with f >= 2: exactly one instance has f silent replicas; the
    oracle ends it quiescent and undecided (histogram bin 0, the never-decided bin, decided == 0).  At f = 1
    (n = 4) {0} and {n - 1} ARE sets of f replicas and the empty set is the only mask that decides, so there about a
    third of the instances stall: "the masks matter for half of the instances" cannot hold with one;
  * packed kernels: the live segments of every wave item with two or more of them carry at least two different masks;
  * wide kernels (3 instances: the four named masks do not fit): the masks differ per instance and each carries
    replicas of every mask word, 0 and n - 1 among them; one has the largest size that decides and, under the
    reference protocol, one has f members;
  * equivocation pattern: the equivocator sets differ in membership and size, 0..f under SPEC, 0..f - 1 under the
    reference protocol (f equivocators leave n - f delivered keys, one short of its phase end).
Seeds (Case bump) were picked on the oracle so that the preconditions hold.
"""
import random

from tests import step_noevent_workloads as T
from tests.golden import specs as S

OFFSET = T.OFFSET
COIN = T.COIN
REF, SPEC, BEB, CONN, XREF = T.REF, T.SPEC, T.BEB, T.CONN, T.XREF
CONST, UNIF, SLOW, GEO = T.CONST, T.UNIF, T.SLOW, T.GEO
CKEYS = ("status", "t_stop", "msgs_sent", "arrivals", "cell_steps")
XREF_PATS = [[4] * 30 + [1, 2, 3, 5] * 2 + [5, 5], [1, 2, 3, 4, 5] * 8, [5] * 29 + [1, 2, 3, 4] * 2 + [4, 3, 2]]


def ipw(n):
    npad = T.pick_npad(n)
    return 64 // npad if npad < 64 else 1


def items(n, count):
    """Engine-local instance ids per wave item."""
    w = ipw(n)
    return [list(range(a, min(a + w, count))) for a in range(0, count, w)]


def largest_deciding(mode, f, consensus=True):
    if not consensus:
        return f
    return f if mode == SPEC else f - 1


def _cover(rng, n, k):
    """k replicas with one of every mask word, 0 and n - 1 among them."""
    must = {0, n - 1} | {64 * w for w in range(1, (n + 63) // 64)}
    assert k >= len(must)
    rest = [d for d in range(n) if d not in must]
    return sorted(must | set(rng.sample(rest, k - len(must))))


def draw_masks(name, n, f, count, kmax, stall, bump=0):
    """The masks of one case, in instance order (module docstring)."""
    rng = random.Random("byz-masks/%s/%d" % (name, bump))
    if n > 64:
        assert count == 3
        words = sorted({0, n - 1} | {64 * w for w in range(1, (n + 63) // 64)} | {64 * w + 6 for w in range(1, (n + 63) // 64)
                                                                                   if 64 * w + 6 < n})
        out = [words, _cover(rng, n, kmax), _cover(rng, n, f if stall else (kmax + len(words)) // 2)]
        rng.shuffle(out)
        return out
    need = [[], [0], [n - 1]]
    if kmax >= 2:
        need.append(sorted(rng.sample(range(n), kmax)))
    if stall and f >= 2:
        need.append(sorted(rng.sample(range(n), f)))
    assert len(need) <= count, name
    for _ in range(1000):
        out = list(need)
        while len(out) < count:
            if kmax == 0:       # f = 1 under the reference protocol: every non-empty mask stalls
                out.append([rng.randrange(n)] if rng.random() < 0.3 else [])
            else:
                out.append(sorted(rng.sample(range(n), rng.randint(0, kmax))))
        rng.shuffle(out)
        differ = sum(out[i] != out[(i + 1) % count] for i in range(count))
        if (all(len({tuple(out[i]) for i in it}) >= 2 for it in items(n, count) if len(it) >= 2)
                and (differ * 4 >= count * 3 or kmax == 0 and differ * 2 >= count + 2)):
            return out
    raise AssertionError("no mask order for " + name)


class Case:
    def __init__(self, name, mode, n, f, model, dmax, count, q, round_cap=1, consensus=True, kernel="step", life=None,
                 general=False, equivocate=False, garbage=None, bump=0, nv=1, masks_of=None):
        self.name, self.mode, self.n, self.f, self.count, self.key_window = name, mode, n, f, count, q
        self.consensus, self.kernel, self.life, self.garbage, self.equivocate = consensus, kernel, life, garbage, equivocate
        self.kmax = largest_deciding(mode, f, consensus)
        self.stall = consensus and mode != SPEC and not equivocate
        self.masks = draw_masks(masks_of or name, n, f, count, self.kmax, self.stall, bump)
        self.seed = 0xB12A0000 + sum(map(ord, masks_of or name)) + 0x10000 * bump
        kw = dict(dconst=dmax) if model == CONST else {}
        if nv != 1:
            kw["nv"] = nv
        seed = self.seed

        def make(g, byz):
            byz = list(byz)
            if not consensus:
                rng = random.Random(seed * 131 + g)
                honest = [o for o in range(n) if o not in byz]
                sends = [(rng.randint(0, 3), o, 0) for o in rng.sample(honest[:-1], 3) + [honest[-1]]]
                return T._brb(mode, n, f, seed, model, dmax, g, sends, byzantine=byz, **kw)
            if general:
                return dict(S.cons_spec(n, f, seed, model, dmax, g, round_cap=round_cap, proposals=XREF_PATS[g % 3],
                                        byzantine=byz, **kw), values=S.VALUES8, general_keys=True)
            extra = dict(extra=S.equivocation_actions(n, byz)) if equivocate else {}
            return T._cons(mode, n, f, seed, model, dmax, g, round_cap, q, byzantine=byz, **kw, **extra)
        self.make = make
        self.run = dict(proposals="loaded" if general else "philox" if consensus else "inject")
        if equivocate:
            self.run["byz_pattern"] = True
        self.cfg_byz = next(m for m in ([1, 2], [2, 3], [1, 3], [1, 2, 3]) if m not in self.masks)
        self.inst = T.instantiation(self.make(OFFSET, []), q)
        self._specs = None

    @property
    def specs(self):
        if self._specs is None:
            self._specs = [dict(self.make(OFFSET + i, m), name="%s/%d" % (self.name, i)) for i, m in enumerate(self.masks)]
        return self._specs

    def neighbour_spec(self, i):
        """Instance i under the mask of instance (i + 1) mod count."""
        return self.make(OFFSET + i, self.masks[(i + 1) % self.count])

    def open_kw(self, **kw):
        return dict(self.run, key_window=self.key_window, load_masks=True, cfg_byzantine=self.cfg_byz,
                    mask_garbage=self.garbage, **kw)

    def stalled(self):
        """Instances the oracle must leave quiescent and undecided: f silent replicas, reference / BEB consensus."""
        return [i for i, m in enumerate(self.masks) if self.stall and len(m) >= self.f]


def _build():
    out = []

    def add(*a, **kw):
        out.append(Case(*a, **kw))

    def packed(n):
        return 2 * ipw(n) + 1
    # ---- packed narrow kernels: 2 IPW + 1 instances (two full wave items and a tail with one live segment)
    add("p4-ref-geo3", REF, 4, 1, GEO, 3, packed(4), 8, round_cap=2)             # TUNED n4-dm4-ref
    add("p4-spec-unif4", SPEC, 4, 1, UNIF, 4, packed(4), 4, round_cap=2)
    add("p8-ref-slow4", REF, 7, 2, SLOW, 4, packed(7), 8, round_cap=2)
    add("p8-spec-geo5", SPEC, 7, 2, GEO, 5, packed(7), 8, round_cap=2)
    add("p16-ref-n13-slow8", REF, 13, 4, SLOW, 8, packed(13), 8, round_cap=2)
    add("p16-spec-n13-unif4", SPEC, 13, 4, UNIF, 4, packed(13), 4)
    add("p16-ref-n16-unif2", REF, 16, 5, UNIF, 2, packed(16), 8)              # per-link delays the reference survives
    # (slow-set delays of 12 over two rounds overflow the engine's key window of 8 on the empty mask, loaded or
    # configured alike -- BRC_OVERFLOW is the engine's own limit, DESIGN section 7 -- so one round at delay 9)
    add("p16-spec-n16-slow9", SPEC, 16, 5, SLOW, 9, packed(16), 8)
    add("p32-ref-n31-slow5", REF, 31, 10, SLOW, 5, packed(31), 8)
    add("p32-spec-n31-geo6", SPEC, 31, 10, GEO, 6, packed(31), 4)
    add("p16-conn-n16-unif2", CONN, 16, 5, UNIF, 2, packed(16), 8)
    add("p16-beb-n13-slow6", BEB, 13, 4, SLOW, 6, packed(13), 8, round_cap=2)
    add("p8-brb-ref-slow4", REF, 7, 2, SLOW, 4, packed(7), 4, consensus=False)
    # bits at and above n set at random in the loaded words: the same masks, the same result
    add("p16-ref-n13-slow8-garbage", REF, 13, 4, SLOW, 8, packed(13), 8, round_cap=2, garbage=0x6A2BA6E,
        masks_of="p16-ref-n13-slow8")
    # ---- NPAD = 64 on the step kernel (engine_runner.open_batch forces it), 5 instances
    add("n64-lean-ref-slow8", REF, 64, 21, SLOW, 8, 5, 4)                       # register masks; bit 63 is a replica
    add("n64-lean-spec-n45-slow5", SPEC, 45, 14, SLOW, 5, 5, 8, round_cap=2)
    # no register masks (three link delays).  Uniform delays up to 3 stall the reference protocol whatever the
    # masks (step_noevent_workloads.TUNED's note): f = 8 and a seed at which three instances decide
    add("n64-lean-ref-n50-unif3", REF, 50, 8, UNIF, 3, 5, 8, bump=1)
    add("n64-xref-n40-slow4", REF, 40, 13, SLOW, 4, 5, 8, round_cap=2, general=True)
    add("n64-conn-n40-slow6", CONN, 40, 13, SLOW, 6, 5, 8)
    # ---- the key-lifetime kernel (BRC_KERNEL=life) and the step kernel on the same batch, 5 instances
    add("life-ref-n50-slow5", REF, 50, 16, SLOW, 5, 5, 4, round_cap=2, kernel="life", life="two-class")
    add("life-spec-n64-slow8", SPEC, 64, 21, SLOW, 8, 5, 8, round_cap=2, kernel="life", life="two-class")
    add("life-conn-n45-const2", CONN, 45, 14, CONST, 2, 5, 4, round_cap=2, kernel="life", life="two-class")
    add("life-conn-n45-unif2", CONN, 45, 14, UNIF, 2, 5, 8, round_cap=2, kernel="life", life="per-link")
    add("life-ref-n40-slow5-q32", REF, 40, 13, SLOW, 5, 5, 32, round_cap=2, kernel="life", life="two-class-hbm")
    # ---- wide kernels: 3 instances, round cap 1
    add("w128-ref-n70-slow8", REF, 70, 23, SLOW, 8, 3, 4)                       # WV = 4
    add("w128-spec-n96-unif4", SPEC, 96, 31, UNIF, 4, 3, 4)                     # delay planes
    add("w256-ref-n140-slow6", REF, 140, 46, SLOW, 6, 3, 8)                     # caller's stride 3 words, engine's 4
    add("w256-spec-n140-slow6", SPEC, 140, 46, SLOW, 6, 3, 4)
    add("w256-ref-n140-slow6-garbage", REF, 140, 46, SLOW, 6, 3, 8, garbage=0x6A2BA6F, masks_of="w256-ref-n140-slow6")
    # ---- the engine's equivocation pattern, re-expanded by brc_load_byzantine (cfg3's shape; one wide case)
    add("eq-ref-n16-unif2", REF, 16, 5, UNIF, 2, 13, 4, equivocate=True, nv=2)
    add("eq-spec-n16-unif4", SPEC, 16, 5, UNIF, 4, 13, 4, equivocate=True, nv=2)
    add("eq-ref-n70-slow4", REF, 70, 23, SLOW, 4, 3, 4, equivocate=True, nv=2)
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


# ---- the oracle, once per spec: every instance, nothing sampled ------------------------------------------
_ORACLE = {}
VID = T.VID


def _run_all(specs, kinds):
    import concurrent.futures

    from oracle import oracle
    with concurrent.futures.ThreadPoolExecutor(min(8, len(specs))) as ex:
        return list(ex.map(lambda sp: oracle.run(sp, light=True) if kinds is None else oracle.run(sp, kinds=kinds), specs))


def oracle_results(case, events=False):
    """{local id: (result, per replica [(round, t, value id) of every decide event], deliver count)} of every
    instance.  events: the results carry the full, canonically sorted deliver / decide / send lists."""
    from tests import golden_io
    key = (case.name, events)
    if key not in _ORACLE:
        if not events and (case.name, True) in _ORACLE:
            return _ORACLE[(case.name, True)]
        outs = _run_all(case.specs, ("deliver", "decide", "send") if events else ("decide",))
        res = {}
        for i, exp in enumerate(outs):
            dec = {}
            for t, node, rnd, val in sorted(exp["events"]["decide"]):
                dec.setdefault(node, []).append((rnd, t, VID[val]))
            if events:
                exp["events"] = golden_io.canonical_events(exp["events"])
            res[i] = (exp, dec, exp["counts"]["deliver"])
        _ORACLE[key] = res
    return _ORACLE[key]


def neighbour_results(case):
    """The oracle's CKEYS of every instance under its neighbour's mask."""
    key = (case.name, "neighbour")
    if key not in _ORACLE:
        outs = _run_all([case.neighbour_spec(i) for i in range(case.count)], None)
        _ORACLE[key] = [tuple(o[k] for k in CKEYS) for o in outs]
    return _ORACLE[key]


def honest(case, i):
    return [d for d in range(case.n) if d not in case.masks[i]]


def expected_read_side(case):
    """(round_histogram(66), decisions() counts by value id with "undecided", disagreements) from the oracle's
    decide events, honest meaning honest under the instance's own mask."""
    hist = [0] * 66
    counts = {}
    undecided = dis = 0
    for i, (_exp, dec, _d) in oracle_results(case).items():
        hon = honest(case, i)
        firsts = [dec[d][0] for d in hon if d in dec]
        undecided += len(hon) - len(firsts)
        for (_r, _t, v) in firsts:
            counts[v] = counts.get(v, 0) + 1
        dis += len({v for (_r, _t, v) in firsts}) > 1
        hist[min(max(r for (r, _t, _v) in firsts), 65) if len(firsts) == len(hon) else 0] += 1
    return hist, counts, undecided, dis
