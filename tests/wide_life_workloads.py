"""Workload table of tests/test_gpu_wide_life.py (GPU) and tests/test_wide_life_workloads.py (its preconditions, on the
oracle alone): the wide key-lifetime kernel (csrc/brc_life_wide.h) of an engine created with BRC_FLAG_WIDE_LIFE, n in
65..256 under constant and slow-set delays.

A batch is COUNT = 8 instances (2 at n = 256, where an oracle run takes half a minute), consecutive global ids from 777, one configuration, one workgroup per
instance.  The engine proposes by itself (Philox draws, or loaded value ids): the kernel takes no injection.

  wl-128-ref-d8      n = 70   f = 23  slow-set D = 8   REF   round cap 2   window 8    (NPAD 128, the last word partial)
  wl-256-ref-byz     n = 130  f = 43  slow-set D = 5   REF   round cap 2   window 8    silent Byzantine replicas 7 and 129
  wl-256-spec-c2     n = 130  f = 43  constant D = 2   SPEC  round cap 3   window 8    (no fast class)
  wl-128-beb-d4      n = 100  f = 33  slow-set D = 4   BEB   round cap 1   window 8
  wl-256-ref-full    n = 256  f = 85  slow-set D = 8   REF   round cap 1   window 8    2 instances (every lane a replica)
  wl-128-loaded      n = 90   f = 29  slow-set D = 6   REF   round cap 1   window 8    loaded proposals, ids 1 .. 3
  wl-128-ref-q16     n = 70   f = 23  slow-set D = 8   REF   round cap 5   window 16   with BRC_FLAG_WIDE_WINDOWS: the specs
                                                                                     of wide_window_workloads' ww-128-ref-q16
                                                                                     (silent Byzantine replicas 5 and 66)
  wl-128-ref-d1      n = 70   f = 23  slow-set D = 1   REF   round cap 2   window 8    one class only
  wl-128-stepcap     n = 70   f = 23  slow-set D = 8   REF   round cap 0   window 8    stops at step cap 30
"""
from tests import interleaved_workloads as I
from tests import wide_window_workloads as W
from tests.golden import specs as S

OFFSET = I.OFFSET
CKEYS = I.CKEYS
CONST, SLOW = I.CONST, I.SLOW
COUNT = 8
FLAG = 16                                    # include/brc.h BRC_FLAG_WIDE_LIFE
STEP_CAP = I.STEP_CAP
STEPCAP_AT = 30


class Batch:
    """name; specs; byz (the silent replicas); q (key window); wide_windows; proposals ("philox" | "loaded");
    stepcap (the batch is meant to stop at its step cap)."""

    def __init__(self, name, make, count=COUNT, byz=(), q=8, wide_windows=False, proposals="philox", stepcap=False,
                 specs_of=None):
        self.name, self._make, self.count, self.byz, self.q = name, make, count, list(byz), q
        self.wide_windows, self.proposals, self.stepcap, self._specs_of = wide_windows, proposals, stepcap, specs_of
        self.nv = 1
        self._specs = None

    @property
    def specs(self):
        if self._specs is None:
            if self._specs_of is not None:
                self._specs = self._specs_of.specs
            else:
                self._specs = [dict(self._make(OFFSET + i, i), name="%s/%d" % (self.name, i)) for i in range(self.count)]
        return self._specs


def _ids(n, g, byz):
    """Loaded proposals: value ids 1 .. 3, a majority of one of them (so that a round can decide)."""
    import random
    rng = random.Random(0x11FE0000 + g)
    top = 1 + g % 3
    return [0 if d in byz else (top if rng.random() < 0.8 else 1 + rng.randrange(3)) for d in range(n)]


def _build():
    out = []

    def add(name, make, **kw):
        out.append(Batch(name, make, **kw))

    add("wl-128-ref-d8", lambda g, i: S.cons_spec(70, 23, 0x11FE0070, SLOW, 8, g, round_cap=2, step_cap=STEP_CAP))
    add("wl-256-ref-byz", lambda g, i: S.cons_spec(130, 43, 0x11FE0130, SLOW, 5, g, round_cap=2, byzantine=[7, 129],
                                                   step_cap=STEP_CAP), byz=[7, 129])
    add("wl-256-spec-c2", lambda g, i: S.spec_cons_spec(130, 43, 0x11FE0131, CONST, 2, g, round_cap=3, window=8, dconst=2,
                                                        step_cap=STEP_CAP))
    add("wl-128-beb-d4", lambda g, i: S.beb_cons_spec(100, 33, 0x11FE0100, SLOW, 4, g, round_cap=1, step_cap=STEP_CAP))
    add("wl-256-ref-full", lambda g, i: S.cons_spec(256, 85, 0x11FE0256, SLOW, 8, g, round_cap=1, step_cap=STEP_CAP), count=2)
    add("wl-128-loaded", lambda g, i: S.cons_spec(90, 29, 0x11FE0090, SLOW, 6, g, round_cap=1, proposals=_ids(90, g, ()),
                                                  step_cap=STEP_CAP), proposals="loaded")
    add("wl-128-ref-q16", None, byz=W.BYZ70, q=16, wide_windows=True, specs_of=W.by_name()["ww-128-ref-q16"])
    add("wl-128-ref-d1", lambda g, i: S.cons_spec(70, 23, 0x11FE0071, SLOW, 1, g, round_cap=2, step_cap=STEP_CAP))
    add("wl-128-stepcap", lambda g, i: S.cons_spec(70, 23, 0x11FE0072, SLOW, 8, g, round_cap=0, step_cap=STEPCAP_AT),
        stepcap=True)
    assert len({b.name for b in out}) == len(out)
    return out


_BATCHES = None
_ORACLE = {}


def batches():
    global _BATCHES
    if _BATCHES is None:
        _BATCHES = _build()
    return _BATCHES


def by_name():
    return {b.name: b for b in batches()}


Q16 = "wl-128-ref-q16"                       # run at window 8 as well: BRC_OVERFLOW on both kernels
RESET = "wl-256-ref-byz"                     # brc_reset / brc_reset_at
BIG = "wl-256-ref-byz"                       # its configuration at 512 instances
BIG_COUNT, BIG_SAMPLED = 512, (0, 1, 63, 64, 200, 383, 510, 511)


def oracle_all():
    """Every batch's oracle runs through one pool, longest first (a pool per batch would idle behind the n = 256
    runs); the window-16 batch shares wide_window_workloads' runs.  Returns the wall-clock seconds spent."""
    import concurrent.futures
    import time
    t0 = time.perf_counter()
    todo = [(b, i, sp) for b in batches() if b._specs_of is None and b.name not in _ORACLE for i, sp in enumerate(b.specs)]
    todo.sort(key=lambda x: -x[2]["n"] ** 2 * max(1, x[2]["round_cap"]))
    with concurrent.futures.ThreadPoolExecutor(8) as ex:
        got = list(ex.map(lambda x: I.oracle_run(x[2]), todo))
    for (b, i, _sp), r in zip(todo, got):
        _ORACLE.setdefault(b.name, {})[i] = r
    for b in batches():
        if b._specs_of is not None:
            W.oracle_results(b._specs_of)
    return time.perf_counter() - t0


def oracle_results(batch):
    """{local id: (result, per replica [(round, t, value id) of every decide event], deliver count)}, computed once per
    batch in this process (interleaved_workloads.oracle_run; the window-16 batch shares wide_window_workloads' runs)."""
    import concurrent.futures
    if batch._specs_of is not None:
        return W.oracle_results(batch._specs_of)
    if batch.name not in _ORACLE:
        with concurrent.futures.ThreadPoolExecutor(min(8, len(batch.specs))) as ex:
            _ORACLE[batch.name] = dict(enumerate(ex.map(I.oracle_run, batch.specs)))
    return _ORACLE[batch.name]


def big_specs():
    """The BIG batch's configuration over BIG_COUNT consecutive instances."""
    b = by_name()[BIG]
    return [dict(b._make(OFFSET + i, i), name="wl-big/%d" % i) for i in range(BIG_COUNT)]


def big_oracle():
    """{local id: oracle_run} of the sampled instances of the 512-instance batch."""
    import concurrent.futures
    if "big" not in _ORACLE:
        specs = big_specs()
        with concurrent.futures.ThreadPoolExecutor(8) as ex:
            _ORACLE["big"] = dict(zip(BIG_SAMPLED, ex.map(I.oracle_run, [specs[i] for i in BIG_SAMPLED])))
    return _ORACLE["big"]


def class_sizes(sp):
    """(honest fast replicas, honest slow replicas) of one instance (csrc/schedule.h slow set; no fast class under
    constant delays or D = 1)."""
    from oracle.schedule import Schedule
    n, f = sp["n"], sp["f"]
    hon = [d for d in range(n) if d not in sp["byzantine"]]
    if sp["delay_model"] != SLOW or sp["dmax"] <= 1:
        return 0, len(hon)
    off = Schedule(n, f, sp["seed"], sp["delay_model"], sp["dmax"], sp.get("dconst", 1)).slow_offset(sp["g"])
    slow = [d for d in hon if (d + n - off) % n < f]
    return len(hon) - len(slow), len(slow)


def lds_bytes_life_wide(npad, q, nv, spec):
    """csrc/brc_internal.h lds_bytes_life_wide."""
    nk = npad * q * nv
    cons = (q * npad + 1) // 2 if spec else 4 * (npad // 64) * npad
    return 16 * (nk // 64) + 8 * cons + 4 * nk + 4 * (4 * 32 + 16) + 2 * nk + q * npad
