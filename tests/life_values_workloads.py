"""Workload table of tests/test_gpu_life_values.py (GPU) and tests/test_life_values_workloads.py (its preconditions, on
the oracle alone): three-bit consensus value ids (seven proposal strings besides "-1") on the wide key-lifetime kernel
(csrc/brc_life_wide.h V8) of an engine created with BRC_FLAG_WIDE_LIFE | BRC_FLAG_LIFE_VALUES, n in 65..256 under
constant and slow-set delays.

A batch is COUNT = 3 instances (2 at n = 256), consecutive global ids from 777, one configuration, one workgroup per
instance, ``values = VALUES8``.  The proposals are loaded (brc_load_proposals); nothing is injected.  f is small against
n: with f = n / 3 the reference's windows (n - f + 1 deliveries, 2 |hosts| > n + f) end in "-1" whatever is proposed.

  lv-128-n65-maj    n = 65   f = 5   slow-set D = 8  REF  cap 1  window 8      one replica in the second wave; a majority
                                                                             of one id in 4 .. 7, by instance
  lv-128-n70-maj    n = 70   f = 5   slow-set D = 8  REF  cap 1  window 8      the same at n = 70
  lv-128full-eight  n = 128  f = 10  slow-set D = 4  REF  cap 1  window 8      all eight ids in one window (`order` full)
  lv-256-c3         n = 130  f = 8   constant D = 3  REF  cap 1  window 8      NPAD 256
  lv-128full-beb    n = 128  f = 10  slow-set D = 8  BEB  cap 1  window 8
  lv-128-cap3       n = 70   f = 5   slow-set D = 4  REF  cap 3  window 8      decided ids >= 4 go back through the send
                                                                             queue and the slot value into later phases
  lv-128-q16        n = 70   f = 5   slow-set D = 8  REF  cap 5  window 16     with BRC_FLAG_WIDE_WINDOWS
  lv-128-masks      n = 70   f = 5   slow-set D = 8  REF  cap 1  window 8      a mask per instance (brc_load_byzantine)
  lv-128-pat-n70    n = 70   f = 5   slow-set D = 8  REF  cap 1  window 4 x 2  BRC_FLAG_LIFE_PATTERN: equivocators 5, 66
  lv-128-pat-f0     n = 65   f = 0   slow-set D = 4  REF  cap 1  window 4 x 2  ... one even equivocator (32): both of its
                                                                             keys deliver, so a window holds the pattern's
                                                                             ids 1 and 2 beside ids above 3
  lv-256-full       n = 256  f = 10  slow-set D = 8  REF  cap 1  window 8      2 instances, no oracle run (about a minute
                                                                             each): held to the step kernel only

fold (wide_values_workloads) is a spec with every value id taken ``& 3`` -- what a kernel that kept two bits would run.
"""
import random

from tests import interleaved_workloads as I
from tests import wide_values_workloads as V
from tests.golden import specs as S

OFFSET = I.OFFSET
CKEYS = I.CKEYS
CONST, SLOW = I.CONST, I.SLOW
COUNT = 3
FLAG_LIFE, FLAG_PATTERN, FLAG = 16, 32, 128  # include/brc.h BRC_FLAG_WIDE_LIFE, _LIFE_PATTERN, _LIFE_VALUES
STEP_CAP = I.STEP_CAP
majority, fold = V.majority, V.fold
BYZ65, BYZ70, BYZ128, BYZ130, BYZ256 = [5, 33], V.BYZ70, V.BYZ128, V.BYZ130, [7, 100, 255]
MASKS70 = ([], [5, 66, 69], [0, 1, 64, 68])


class Batch:
    """name; specs; q, nv (key window, variants); wide_windows; pattern (BRC_FLAG_LIFE_PATTERN: the specs carry the
    equivocation pattern as actions); load_masks (the instances' Byzantine lists differ: brc_load_byzantine), cfg_byz
    (the configuration's own mask then); oracle (False: no oracle run)."""

    def __init__(self, name, make, count=COUNT, q=8, nv=1, wide_windows=False, pattern=False, load_masks=False,
                 cfg_byz=(), oracle=True):
        self.name, self._make, self.count, self.q, self.nv = name, make, count, q, nv
        self.wide_windows, self.pattern, self.load_masks, self.cfg_byz = wide_windows, pattern, load_masks, list(cfg_byz)
        self.oracle = oracle
        self._specs = None

    @property
    def specs(self):
        if self._specs is None:
            self._specs = [dict(self._make(OFFSET + i, i), name="%s/%d" % (self.name, i), values=S.VALUES8)
                           for i in range(self.count)]
        return self._specs


def rest(m):
    return [v for v in range(8) if v != m]


def _spec(n, f, seed, model, dmax, g, props, byz, cap=1, beb=False, dconst=1, nv=1, pattern=False):
    mk = S.beb_cons_spec if beb else S.cons_spec
    byz = sorted(byz)
    return mk(n, f, seed, model, dmax, g, round_cap=cap, proposals=props, byzantine=byz, nv=nv, dconst=dconst,
              extra=S.equivocation_actions(n, byz, nv=nv) if pattern else (), step_cap=STEP_CAP)


def _build():
    out = []

    def add(name, make, **kw):
        out.append(Batch(name, make, **kw))

    top = lambda g, i: 4 + (g + i) % 4                                    # noqa: E731
    add("lv-128-n65-maj", lambda g, i: _spec(65, 5, 0x17A10065, SLOW, 8, g, majority(65, g, top(g, i), 52, rest(top(g, i))), BYZ65))
    add("lv-128-n70-maj", lambda g, i: _spec(70, 5, 0x17A10070, SLOW, 8, g, majority(70, g, top(g, i), 56, rest(top(g, i))), BYZ70))
    add("lv-128full-eight", lambda g, i: _spec(128, 10, 0x3B170128, SLOW, 4, g, majority(128, g, 4, 93, rest(4)), BYZ128))
    add("lv-256-c3", lambda g, i: _spec(130, 8, 0x17A10130, CONST, 3, g, majority(130, g, 5 + (g + i) % 3, 100, rest(5 + (g + i) % 3)),
                                        BYZ130, dconst=3))
    add("lv-128full-beb", lambda g, i: _spec(128, 10, 0x17A10128, SLOW, 8, g, majority(128, g, 5 + (g + i) % 3, 100, rest(5 + (g + i) % 3)),
                                             BYZ128, beb=True))
    add("lv-128-cap3", lambda g, i: _spec(70, 5, 0x17A13070, SLOW, 4, g, majority(70, g, top(g, i), 56, rest(top(g, i))), BYZ70, cap=3))
    add("lv-128-q16", lambda g, i: _spec(70, 5, 0x17A15070, SLOW, 8, g, majority(70, g, top(g, i), 56, rest(top(g, i))), BYZ70, cap=5),
        q=16, wide_windows=True)
    add("lv-128-masks", lambda g, i: _spec(70, 5, 0x17A16070, SLOW, 8, g, majority(70, g, top(g, i), 56, rest(top(g, i))), MASKS70[i]),
        load_masks=True, cfg_byz=[3])
    add("lv-128-pat-n70", lambda g, i: _spec(70, 5, 0x17A17070, SLOW, 8, g, majority(70, g, 5 + (g + i) % 3, 56, rest(5 + (g + i) % 3)),
                                             [5, 66], nv=2, pattern=True), q=4, nv=2, pattern=True)
    add("lv-128-pat-f0", lambda g, i: _spec(65, 0, 0x17A17065, SLOW, 4, g, majority(65, g, 5 + (g + i) % 3, 48, rest(5 + (g + i) % 3)),
                                            [32], nv=2, pattern=True), q=4, nv=2, pattern=True)
    add("lv-256-full", lambda g, i: _spec(256, 10, 0x17A10256, SLOW, 8, g, majority(256, g, top(g, i), 200, rest(top(g, i))), BYZ256),
        count=2, oracle=False)
    assert len({b.name for b in out}) == len(out)
    return out


_BATCHES = None
_ORACLE = {}
_SECONDS = {}

EIGHT = "lv-128full-eight"
CAP3 = "lv-128-cap3"
RESET = "lv-256-c3"                          # brc_reset / brc_reset_at
OTHER = "lv-128-n70-maj"                     # (the reset test loads another batch's proposals in between)
BINARY = ("lv-128-n70-maj", "lv-256-c3")     # their configurations under binary Philox proposals
NO_ORACLE = "lv-256-full"
SIBLING = {"lv-256-full": "lv-256-c3"}       # the batch that stands in for one without an oracle run
BIG = "lv-128-n70-maj"                       # its configuration at 256 instances
BIG_COUNT, BIG_SAMPLED = 256, (0, 85, 170, 255)


def batches():
    global _BATCHES
    if _BATCHES is None:
        _BATCHES = _build()
    return _BATCHES


def by_name():
    return {b.name: b for b in batches()}


def _timed_run(sp):
    import time
    t0 = time.perf_counter()
    r = I.oracle_run(sp)
    return r, time.perf_counter() - t0


def oracle_results(batch):
    """{local id: (result, per replica [(round, t, value id) of every decide event], deliver count)}, computed once per
    batch in this process (interleaved_workloads.oracle_run); oracle_seconds(batch): each run's wall-clock time."""
    import concurrent.futures
    assert batch.oracle, batch.name
    if batch.name not in _ORACLE:
        with concurrent.futures.ThreadPoolExecutor(len(batch.specs)) as ex:
            got = list(ex.map(_timed_run, batch.specs))
        _ORACLE[batch.name] = {i: r for i, (r, _s) in enumerate(got)}
        _SECONDS[batch.name] = [s for (_r, s) in got]
    return _ORACLE[batch.name]


def oracle_seconds(batch):
    oracle_results(batch)
    return _SECONDS[batch.name]


def big_specs():
    """The BIG batch's configuration over BIG_COUNT consecutive instances."""
    b = by_name()[BIG]
    return [dict(b._make(OFFSET + i, i), name="lv-big/%d" % i, values=S.VALUES8) for i in range(BIG_COUNT)]


def big_oracle():
    """{local id: oracle_run} of the sampled instances of the 256-instance batch."""
    import concurrent.futures
    if "big" not in _ORACLE:
        specs = big_specs()
        with concurrent.futures.ThreadPoolExecutor(len(BIG_SAMPLED)) as ex:
            _ORACLE["big"] = dict(zip(BIG_SAMPLED, ex.map(I.oracle_run, [specs[i] for i in BIG_SAMPLED])))
    return _ORACLE["big"]


def binary_specs(name):
    """The batch's configuration with Philox-drawn binary proposals (ids 1 and 2), as an unflagged engine runs it."""
    b = by_name()[name]
    out = []
    for i, sp in enumerate(b.specs):
        mk = S.beb_cons_spec if sp["mode"].startswith("beb") else S.cons_spec
        out.append(dict(mk(sp["n"], sp["f"], sp["seed"], sp["delay_model"], sp["dmax"], sp["g"], round_cap=sp["round_cap"],
                           byzantine=sp["byzantine"], dconst=sp["dconst"], step_cap=STEP_CAP), name="%s-binary/%d" % (name, i)))
    return out


def drawn_ids(n, count, seed):
    """Proposals drawn uniformly over ids 0 .. 7 (the timing run of the GPU test): [instance][replica]."""
    rng = random.Random(seed)
    return [[rng.randrange(8) for _ in range(n)] for _ in range(count)]


def lds_bytes_life_wide(npad, q, nv, spec, pat=False, v8=False):
    """csrc/brc_layout.h lds_bytes_life_wide."""
    nk = npad * q * nv
    nkw = nk // 64
    cons = (q * npad + 1) // 2 if spec else 4 * (npad // 64) * npad
    return (16 * nkw + 8 * cons + 4 * nk + 4 * (4 * 32 + 16) + 2 * nk + q * npad + (16 * nkw + 64 + 4 * npad if pat else 0) +
            (nk if v8 else 0))
