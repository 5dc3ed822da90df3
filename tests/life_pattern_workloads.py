"""Workload table of tests/test_gpu_life_pattern.py (GPU) and tests/test_life_pattern_workloads.py (its preconditions, on
the oracle alone): the equivocation pattern (BRC_BYZ_EQUIVOCATE) on the wide key-lifetime kernel's pattern form
(csrc/brc_life_wide.h PAT) of an engine created with BRC_FLAG_WIDE_LIFE | BRC_FLAG_LIFE_PATTERN, n in 65..256 under
constant and slow-set delays.

A batch is COUNT = 8 instances, consecutive global ids from 777, one configuration, one workgroup per instance.  The
oracle runs the pattern as actions (specs.equivocation_actions); the engine proposes by itself (Philox draws, or loaded
value ids) and derives the pattern from the Byzantine mask: nothing is injected.

  lp-128-ref-masks   n = 70   f = 23  slow-set D = 8   REF  cap 1  window 4 x 2   a mask per instance (brc_load_byzantine):
                                                                                none, f replicas, and sets with both
                                                                                parities in both delay classes
  lp-256-ref-c3      n = 130  f = 43  constant D = 3   REF  cap 1  window 4 x 2   Byzantine replicas in both waves
  lp-256-ref-loaded  n = 256  f = 85  slow-set D = 8   REF  cap 1  window 4 x 2   loaded proposals, ids 1 .. 3; 84 Byzantine
                                                                                replicas (every third one), so n - f + 1
                                                                                honest ones are left and a round decides
  lp-128-beb-d4      n = 100  f = 33  slow-set D = 4   BEB  cap 1  window 4 x 2
  lp-128-f1-const    n = 65   f = 1   constant D = 2   REF  cap 1  window 4 x 2   one odd Byzantine replica (33)
  lp-128-f1-slow     n = 65   f = 1   slow-set D = 4   REF  cap 1  window 4 x 2   the same: the even half plus the origin's
                                                                                own ECHO reach the ECHO quorum
  lp-128-f0-const    n = 65   f = 0   constant D = 2   REF  cap 1  window 4 x 2   one even Byzantine replica (32)
  lp-128-f0-slow     n = 65   f = 0   slow-set D = 4   REF  cap 1  window 4 x 2   the same: each half plus the origin's ECHO
                                                                                reaches the quorum, both variants deliver
  lp-128-ref-q16     n = 70   f = 23  slow-set D = 4   REF  cap 4  window 8 x 2   with BRC_FLAG_WIDE_WINDOWS
  lp-128-ref-nv4     n = 70   f = 23  constant D = 1   REF  cap 1  window 2 x 4   (lock-step: phase leakage overflows a
                                                                                window of 2 under slow-set delays)

No n / f >= 1 lets one replica deliver both variants of an origin: the odd half plus the origin holds floor(n / 2) ECHOs,
the quorum is floor((n + f) / 2) + 1.  The nearest shape that does is n = 65, f = 0 with an even Byzantine replica.
"""
from tests import interleaved_workloads as I
from tests.golden import specs as S

OFFSET = I.OFFSET
CKEYS = I.CKEYS
CONST, SLOW = I.CONST, I.SLOW
COUNT = 8
FLAG_LIFE, FLAG = 16, 32                     # include/brc.h BRC_FLAG_WIDE_LIFE, BRC_FLAG_LIFE_PATTERN
STEP_CAP = I.STEP_CAP


class Batch:
    """name; specs; nv, q (variants, key window); wide_windows; proposals ("philox" | "loaded"); load_masks (the
    instances' Byzantine lists differ: brc_load_byzantine); cfg_byz (the configuration's own mask)."""

    def __init__(self, name, make, nv=2, q=4, wide_windows=False, proposals="philox", load_masks=False, cfg_byz=()):
        self.name, self._make, self.nv, self.q = name, make, nv, q
        self.wide_windows, self.proposals, self.load_masks, self.cfg_byz = wide_windows, proposals, load_masks, list(cfg_byz)
        self.count = COUNT
        self._specs = None

    @property
    def specs(self):
        if self._specs is None:
            self._specs = [dict(self._make(OFFSET + i, i), name="%s/%d" % (self.name, i)) for i in range(self.count)]
        return self._specs


def slow_set(n, f, seed, model, dmax, g):
    """The slow replicas of one instance (csrc/schedule.h slow set; none under constant delays or D = 1)."""
    from oracle.schedule import Schedule
    if model != SLOW or dmax <= 1:
        return []
    off = Schedule(n, f, seed, model, dmax, 1).slow_offset(g)
    return [(off + j) % n for j in range(f)]


def _spec(n, f, seed, model, dmax, g, cap, byz, nv=2, beb=False, dconst=1, proposals=None):
    mk = S.beb_cons_spec if beb else S.cons_spec
    byz = sorted(byz)
    return mk(n, f, seed, model, dmax, g, round_cap=cap, byzantine=byz, nv=nv, dconst=dconst, proposals=proposals,
              extra=S.equivocation_actions(n, byz, nv=nv), step_cap=STEP_CAP)


def _ids(n, g, byz):
    """Loaded proposals: value ids 1 .. 3, a majority of one of them (so that a round can decide)."""
    import random
    rng = random.Random(0x1FE50000 + g)
    top = 1 + g % 3
    return [0 if d in byz else (top if rng.random() < 0.8 else 1 + rng.randrange(3)) for d in range(n)]


def masks70(g, i):
    """Instance i's Byzantine replicas at n = 70, f = 23: none (i = 0), f of them (i = 1: every third replica), else two
    neighbours (both parities) at the start of the slow set and two or more after its end (fast ones)."""
    n, f = 70, 23
    if i == 0:
        return []
    if i == 1:
        return list(range(1, 70, 3))
    slow = slow_set(n, f, SEED70, SLOW, 8, g)
    return sorted({slow[0], slow[1]} | {(slow[-1] + 1 + j) % n for j in range(2 + i % 3)})


SEED70 = 0x1FE50070
BYZ130 = [5, 6, 64, 65, 127, 128, 129]
BYZ256 = list(range(1, 256, 3))[:84]
BYZ100 = [1, 2, 50, 51, 98, 99]
BYZ70 = [5, 66]
BYZ70V4 = [5, 66, 67]


def _build():
    out = []

    def add(name, make, **kw):
        out.append(Batch(name, make, **kw))

    add("lp-128-ref-masks", lambda g, i: _spec(70, 23, SEED70, SLOW, 8, g, 1, masks70(g, i)), load_masks=True, cfg_byz=[3])
    add("lp-256-ref-c3", lambda g, i: _spec(130, 43, 0x1FE50130, CONST, 3, g, 1, BYZ130, dconst=3))
    add("lp-256-ref-loaded", lambda g, i: _spec(256, 85, 0x1FE50256, SLOW, 8, g, 1, BYZ256, proposals=_ids(256, g, BYZ256)),
        proposals="loaded")
    add("lp-128-beb-d4", lambda g, i: _spec(100, 33, 0x1FE50100, SLOW, 4, g, 1, BYZ100, beb=True))
    add("lp-128-f1-const", lambda g, i: _spec(65, 1, 0x1FE50065, CONST, 2, g, 1, [33], dconst=2))
    add("lp-128-f1-slow", lambda g, i: _spec(65, 1, 0x1FE50066, SLOW, 4, g, 1, [33]))
    add("lp-128-f0-const", lambda g, i: _spec(65, 0, 0x1FE50067, CONST, 2, g, 1, [32], dconst=2))
    add("lp-128-f0-slow", lambda g, i: _spec(65, 0, 0x1FE50068, SLOW, 4, g, 1, [32]))
    add("lp-128-ref-q16", lambda g, i: _spec(70, 23, 0x1FE50071, SLOW, 4, g, 4, BYZ70), q=8, wide_windows=True)
    add("lp-128-ref-nv4", lambda g, i: _spec(70, 23, 0x1FE50072, CONST, 1, g, 1, BYZ70V4, nv=4), nv=4, q=2)
    assert len({b.name for b in out}) == len(out)
    return out


_BATCHES = None
_ORACLE = {}

SMALL_F = ("lp-128-f1-const", "lp-128-f1-slow", "lp-128-f0-const", "lp-128-f0-slow")
RESET = "lp-128-ref-masks"                   # brc_reset / brc_reset_at / brc_load_byzantine again


def batches():
    global _BATCHES
    if _BATCHES is None:
        _BATCHES = _build()
    return _BATCHES


def by_name():
    return {b.name: b for b in batches()}


def oracle_all():
    """Every batch's oracle runs through one pool, longest first.  Returns the wall-clock seconds spent."""
    import concurrent.futures
    import time
    t0 = time.perf_counter()
    todo = [(b, i, sp) for b in batches() if b.name not in _ORACLE for i, sp in enumerate(b.specs)]
    todo.sort(key=lambda x: -(x[2]["n"] - len(x[2]["byzantine"])) ** 3 * max(1, x[2]["round_cap"]))
    with concurrent.futures.ThreadPoolExecutor(8) as ex:
        got = list(ex.map(lambda x: I.oracle_run(x[2]), todo))
    for (b, i, _sp), r in zip(todo, got):
        _ORACLE.setdefault(b.name, {})[i] = r
    for name in list(_ORACLE):
        _ORACLE[name] = dict(sorted(_ORACLE[name].items()))     # local id order, whatever order the pool ran them in
    return time.perf_counter() - t0


def oracle_results(batch):
    """{local id: (result, per replica [(round, t, value id) of every decide event], deliver count)}, computed once per
    batch in this process (interleaved_workloads.oracle_run)."""
    import concurrent.futures
    if batch.name not in _ORACLE:
        with concurrent.futures.ThreadPoolExecutor(min(8, len(batch.specs))) as ex:
            _ORACLE[batch.name] = dict(enumerate(ex.map(I.oracle_run, batch.specs)))
    return _ORACLE[batch.name]


def rotated_masks(batch):
    """The batch's Byzantine lists moved one instance on: other masks for the same engine."""
    lists = [sp["byzantine"] for sp in batch.specs]
    return lists[1:] + lists[:1]


def equivocated_deliveries(sp, exp):
    """(deliveries of a Byzantine origin's keys at honest replicas, (replica, origin) pairs that delivered both variants)."""
    byz, nv = set(sp["byzantine"]), sp["nv"]
    got = {}
    count = 0
    for _t, node, kp, _s in exp["events"]["deliver"]:
        if kp // nv in byz:
            count += 1
            got.setdefault((node, kp // nv), set()).add(kp % nv)
    return count, sum(len(v) == 2 for v in got.values())


def class_sizes4(sp):
    """Honest replicas per (fast | slow) x (even | odd): [fast even, fast odd, slow even, slow odd] (no fast class under
    constant delays or D = 1; no slow replica at f = 0)."""
    n = sp["n"]
    two = sp["delay_model"] == SLOW and sp["dmax"] > 1
    slow = set(slow_set(n, sp["f"], sp["seed"], sp["delay_model"], sp["dmax"], sp["g"]))
    out = [0, 0, 0, 0]
    for d in range(n):
        if d not in sp["byzantine"]:
            out[(2 if d in slow or not two else 0) + (d & 1)] += 1
    return out


def lds_bytes_life_wide(npad, q, nv, spec, pat=False):
    """csrc/brc_internal.h lds_bytes_life_wide."""
    nk = npad * q * nv
    nkw = nk // 64
    cons = (q * npad + 1) // 2 if spec else 4 * (npad // 64) * npad
    return 16 * nkw + 8 * cons + 4 * nk + 4 * (4 * 32 + 16) + 2 * nk + q * npad + (16 * nkw + 64 + 4 * npad if pat else 0)
