"""Workload table of tests/test_gpu_key_domain.py (GPU) and tests/test_key_domain_workloads.py (its preconditions, on the
oracle alone): seeds, coin seeds and global instance ids with a non-zero high word, on every device call site of the
Philox draw (csrc/schedule.h draw(seed, g, a, purpose, b): key (seed_lo, seed_hi), counter (g_lo, g_hi, ...)).

Every other table keeps its seeds below 2^32 and its ids near 777, so key word k1 and counter word c1 are zero in every
launch they make.  Here one small consensus batch per draw site and per way of holding g (fifteen families) runs in
four placements of the high bits (PLACEMENTS), 60 batches:

  seed-hi   seed = lo | HI << 32 (SPEC: coin seed = clo | CHI << 32 as well), ids from 777
  g-hi      ids from 3 * 2^32 + 777, the family's 32-bit seed
  carry     ids from 2^32 - c, 0 < c < count: the first c instances have g_hi = 0, the others g_hi = 1; on the packed
            kernels c is no multiple of 64 / NPAD, so the boundary falls inside one wave item
  top       ids from 2^64 - 100 (no wrap), seed and coin seed with bit 63 set

Each batch has its low-word twins (Batch.twins): the batch a kernel computes that loses the word -- the seed's (and, a
twin of its own, the coin seed's) low 32 bits under seed-hi, every id's low 32 bits under the three others.  The
preconditions prove on the oracle that each twin differs from the batch (under carry: on an instance past the
boundary; before it batch and twin are one spec), so a kernel that loses a high word fails the oracle comparison.

Proposals are Philox draws on the device (PURPOSE_PROPOSAL), with one exception: only the common coin reads the coin
seed, so the SPEC families' seed-hi batches load an even split of "0" and "1", after which no phase-1 majority forms,
phase 2 tallies stay at or below f and the coin sets the next estimate.  COIN_DIFFERS records, per SPEC family, the
local ids of that batch on which the oracle's result under the coin seed's low word differs (a scan of the batch's
consecutive ids, run once and written down; the preconditions recompute it).

Every instance of every batch is compared with the oracle: at n > 64 a batch has three instances -- the first, the
last and the one just past the carry boundary are all of them.

Choices found on the oracle alone (tests/test_key_domain_workloads.py's conditions).  The reference protocol ignores a
SEND that arrives after an ECHO of its key, so under uniform delays up to 5 no instance of the per-link lifetime family
(connection peers, n = 37) decides at any fault bound 0 .. 36: it takes geometric delays up to 5 and f = 8, as
step_noevent_workloads.TUNED does for the same reason; the packed connection-peer family geometric delays up to 3 and
f = 2.  The pattern family's seed is the first of four on which every placement has a differing twin.
"""
from tests import step_noevent_workloads as T
from tests.golden import specs as S

OFFSET = T.OFFSET
M32 = 0xFFFFFFFF
REF, SPEC, BEB, CONN, XREF = T.REF, T.SPEC, T.BEB, T.CONN, T.XREF
CONST, UNIF, SLOW, GEO = T.CONST, T.UNIF, T.SLOW, T.GEO
CKEYS = ("status", "t_stop", "msgs_sent", "arrivals", "cell_steps")

HI = 0x9E3779B1                 # odd, bits in both of its halves
CHI = 0x85EBCA6B                # the coin seed's: another odd constant
TOP_HI = 0xC2B2AE35             # bit 31 set: bit 63 of the seed
TOP_CHI = 0xA54FF53B
CLO = T.COIN + 5                # the coin seed's low word (COIN_DIFFERS)
G_HI = 3 * 2 ** 32 + OFFSET
TOP = 2 ** 64 - 100
PLACEMENTS = ("seed-hi", "g-hi", "carry", "top")


class Family:
    """One draw site and one way of holding g.  kind is the engine the GPU test opens: "step" (BRC_KERNEL=step at
    n in 33..64), "life" (BRC_KERNEL=life), "wide_life" (BRC_FLAG_WIDE_LIFE), "pattern" (and BRC_FLAG_LIFE_PATTERN with
    the engine's own equivocation pattern).  lo: the 32-bit seed.  c: the carry placement's boundary (ids from
    2^32 - c).  INTENDED has the step-kernel instantiation instantiation() must name for it."""

    def __init__(self, name, kind, mode, n, f, model, dmax, q, lo, c, general=False, byz=(), nv=1, step_cap=400):
        self.name, self.kind, self.mode, self.n, self.f, self.model, self.dmax, self.q = name, kind, mode, n, f, model, dmax, q
        self.lo, self.c, self.general, self.byz, self.nv, self.step_cap = lo, c, general, list(byz), nv, step_cap
        self.npad = T.pick_npad(n)
        self.count = 3 if self.npad > 64 else 5 if self.npad == 64 else 3 * (64 // self.npad) + 1
        self.round_cap = 2 if n <= 64 else 1
        self.split = [1 + d % 2 for d in range(n)]           # "0", "1", "0", ...: the even split of the SPEC batches

    def spec(self, g, seed, coin, loaded):
        kw = dict(byzantine=list(self.byz), step_cap=self.step_cap, nv=self.nv)
        if self.kind == "pattern":
            kw["extra"] = S.equivocation_actions(self.n, self.byz, nv=self.nv)
        if loaded:
            kw["proposals"] = self.split
        sp = T._cons(self.mode, self.n, self.f, seed, self.model, self.dmax, g, self.round_cap, self.q, **kw)
        if self.mode == SPEC:
            sp = dict(sp, coin_seed=coin)
        return dict(sp, general_keys=True) if self.general else sp

    def keys(self, placement):
        """(seed, coin seed, first id, loaded proposals) of a placement."""
        spec = self.mode == SPEC
        if placement == "seed-hi":
            return self.lo | HI << 32, CLO | CHI << 32, OFFSET, spec
        if placement == "g-hi":
            return self.lo, CLO, G_HI, False
        if placement == "carry":
            return self.lo, CLO, 2 ** 32 - self.c, False
        assert placement == "top"
        return self.lo | TOP_HI << 32, CLO | TOP_CHI << 32, TOP, False


class Batch:
    """What state_compare.oracle_mismatches and step_noevent_workloads.oracle_results ask of a case (name, specs,
    oracle_ids, consensus), fault_bound_workloads.expected_read_side (n, byz) and the GPU test (family, placement,
    run, key_window, twins).  name is made of the batch's content, so two batches that are one batch (the twin of
    seed-hi and the twin of g-hi: the family's 32-bit seed from id 777) share their oracle runs; label is the test id."""
    consensus = True

    def __init__(self, fam, label, seed, coin, ids, loaded, placement=None):
        self.family, self.label, self.placement, self.loaded = fam, label, placement, loaded
        self.seed, self.coin, self.ids = seed, coin, list(ids)
        self.n, self.count, self.key_window = fam.n, len(self.ids), fam.q
        self.run = dict(proposals="loaded" if loaded else "philox")
        run = len(self.ids) == 1 + self.ids[-1] - self.ids[0]
        self.name = "kd/%s/s%x/c%x/%s/%s" % (fam.name, seed, coin if fam.mode == SPEC else 0,
                                             ("o%x" % self.ids[0]) + ("" if run else "+%d-low32" % self.count), "split" if loaded else "philox")
        self.twins = []
        self._specs = None

    @property
    def specs(self):
        if self._specs is None:
            self._specs = [dict(self.family.spec(g, self.seed, self.coin, self.loaded), name="%s/%d" % (self.name, i))
                           for i, g in enumerate(self.ids)]
        return self._specs

    def oracle_ids(self):
        return list(range(self.count))

    def byz(self, i):
        return self.family.byz

    def past_boundary(self):
        """The local ids whose global id has a non-zero high word."""
        return [i for i, g in enumerate(self.ids) if g >> 32]


def _build_families():
    out = []

    def add(*a, **kw):
        out.append(Family(*a, **kw))
    # ---- narrow step kernel, packed (brc_step.h): 64 / NPAD instances with different g in one wave
    add("p4-beb-n3", "step", BEB, 3, 1, GEO, 3, 8, 0x4B1D0403, 21)
    add("p8-spec-n8", "step", SPEC, 8, 2, UNIF, 4, 4, 0x4B1D0808, 11)
    add("p16-conn-n13", "step", CONN, 13, 2, GEO, 3, 8, 0x4B1D100D, 6)
    add("p32-ref-n32", "step", REF, 32, 10, SLOW, 8, 8, 0x4B1D2020, 3)
    # ---- narrow step kernel at NPAD 64, BRC_KERNEL=step: lean, register masks, general keys
    add("lean-ref-n50", "step", REF, 50, 9, GEO, 5, 8, 0x4B1D4032, 2)
    add("regmask-beb-n64", "step", BEB, 64, 21, SLOW, 8, 8, 0x4B1D4040, 3)
    add("general-n40", "step", REF, 40, 9, GEO, 5, 8, 0x4B1D4028, 1, general=True)
    # ---- narrow key-lifetime kernel (brc_life.h), BRC_KERNEL=life
    add("life2c-ref-n45", "life", REF, 45, 14, SLOW, 8, 8, 0x4B1D1F2D, 4)
    add("lifepl-conn-n37", "life", CONN, 37, 8, GEO, 5, 8, 0x4B1D1F25, 2)
    add("life-spec-n64", "life", SPEC, 64, 21, SLOW, 8, 8, 0x4B1D1F40, 3)
    # ---- wide step kernel (brc_step_wide.h)
    add("w128-spec-n70", "step", SPEC, 70, 23, SLOW, 5, 4, 0x4B1D8046, 1)
    add("w256-ref-n130", "step", REF, 130, 42, GEO, 5, 8, 0x4B1D0182, 2)
    # ---- wide key-lifetime kernel (brc_life_wide.h), BRC_FLAG_WIDE_LIFE
    add("wlife-ref-n96", "wide_life", REF, 96, 31, SLOW, 8, 8, 0x4B1D1F60, 2)
    add("wpat-ref-n73", "pattern", REF, 73, 24, SLOW, 4, 4, 0x4B1E1F49, 1, byz=[3, 66, 70], nv=2)
    add("wlife-spec-n129", "wide_life", SPEC, 129, 42, SLOW, 5, 8, 0x4B1D1F81, 2)
    assert len({f.name for f in out}) == len(out)
    return out


# the instantiation (or, for the lifetime families, the kernel file's form) each family is meant for
INTENDED = {
    "p4-beb-n3": ("step", 4, 4, BEB, 0),
    "p8-spec-n8": ("step", 8, 4, SPEC, 0),
    "p16-conn-n13": ("step", 16, 4, CONN, 0),
    "p32-ref-n32": ("step", 32, 8, REF, 0),
    "lean-ref-n50": ("step", 64, 8, REF, 0),
    "regmask-beb-n64": ("step", 64, 8, BEB, 2),
    "general-n40": ("step", 64, 8, XREF, 0),
    "life2c-ref-n45": "life",
    "lifepl-conn-n37": "life",
    "life-spec-n64": "life",
    "w128-spec-n70": ("wide", 128, 8, SPEC, 4),
    "w256-ref-n130": ("wide", 256, 8, REF, 0),
    "wlife-ref-n96": "life",
    "wpat-ref-n73": "life",
    "wlife-spec-n129": "life",
}

# seed-hi batches of the SPEC families: the local ids on which the coin seed's low word gives another result
# (the scan: CLO = COIN + k for k = 0, 1, ...; k = 5 is the first at which all three instances of the n > 64 batches differ.
# The coin is one bit per (instance, round), so about half of the instances of any batch differ.)
COIN_DIFFERS = {
    "p8-spec-n8": [0, 1, 2, 3, 4, 8, 10, 11, 12, 14, 15, 16, 17, 18, 19, 20],
    "life-spec-n64": [0, 1, 2, 3, 4],
    "w128-spec-n70": [0, 1, 2],
    "wlife-spec-n129": [0, 1, 2],
}

# one family per kernel file: the event-log twin (placement g-hi) and the re-keyed engine
PER_KERNEL_FILE = {"brc_step.h": "p16-conn-n13", "brc_step_wide.h": "w128-spec-n70", "brc_life.h": "life2c-ref-n45",
                   "brc_life_wide.h": "wlife-ref-n96"}

_FAMILIES = None
_BATCHES = None


def families():
    global _FAMILIES
    if _FAMILIES is None:
        _FAMILIES = _build_families()
    return _FAMILIES


def family(name):
    return {f.name: f for f in families()}[name]


def consecutive(fam, seed, coin, first, count, loaded=False, label=None, placement=None):
    return Batch(fam, label or "%s@%x" % (fam.name, first), seed, coin, range(first, first + count), loaded, placement)


def _batch(fam, placement):
    seed, coin, first, loaded = fam.keys(placement)
    b = consecutive(fam, seed, coin, first, fam.count, loaded, "%s-%s" % (fam.name, placement), placement)
    if placement == "seed-hi":
        b.twins.append(("seed & 0xFFFFFFFF", consecutive(fam, seed & M32, coin, first, fam.count, loaded)))
        if fam.mode == SPEC:
            b.twins.append(("coin_seed & 0xFFFFFFFF", consecutive(fam, seed, coin & M32, first, fam.count, loaded)))
    else:
        b.twins.append(("g & 0xFFFFFFFF", Batch(fam, b.label + "-low32", seed, coin, [g & M32 for g in b.ids], loaded)))
    return b


def batches():
    global _BATCHES
    if _BATCHES is None:
        _BATCHES = [_batch(f, p) for f in families() for p in PLACEMENTS]
        assert len({b.label for b in _BATCHES}) == len(_BATCHES)
    return _BATCHES


def by_label():
    return {b.label: b for b in batches()}


def summary(exp, dec, delivers):
    """What the twins are compared in: the counters and every decide row."""
    return tuple(exp[k] for k in CKEYS) + (tuple(sorted((d, tuple(rows)) for d, rows in dec.items())),)


def differing(batch, twin):
    """The local ids on which the oracle's result on the batch differs from its result on a twin."""
    a, b = T.oracle_results(batch), T.oracle_results(twin)
    return [i for i in range(batch.count) if summary(*a[i]) != summary(*b[i])]
