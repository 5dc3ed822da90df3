"""Workload table of tests/test_gpu_life_windows.py (GPU) and tests/test_life_window_workloads.py
(its preconditions, on the oracle alone): the key-lifetime kernel's instantiations
(csrc/brc_kern_life.hip) that tests/test_gpu_life.py and tests/test_gpu_fullsize.py leave out.

  A  the HBM-metadata forms: key windows 32 / 64 / 128 x REFERENCE / BEB / connection peers, each with
     a round cap at which half the window overflows (the window is in use);
  B  late steps: constant delay 8 keeps the replicas in lock-step, so a run passes step 256 (the class
     delivery code 0x80 | step mod 128 wraps twice, the 16-bit slot stamps and the 32-row rings with it);
  C  the per-link form's 64-row ring (delays above 8) under SPEC and BEB;
  D  SPEC deep into coin rounds, on the step kernel and the lifetime kernel.

A workload: kw (Engine keywords), count (instances), step ("run": the step kernel takes the configuration,
"run64": its first 64 instances only -- connection peers' 40-B cells take 10 MB per instance at 4,096 key
slots -- or "refuse": brc_create refuses it under BRC_KERNEL=step, include/brc.h), half_step (the same for
the half window of part A), t_floor (every sampled instance stops after this step), decides (every honest
replica decides at least round_cap times), extra (sampled ids besides the first and the last).
"""
import json
import random

import numpy as np

from tests.test_gpu_fullsize import _oracle_first_last
from tests.test_gpu_life import COIN, _L, _oracle_spec, _run  # noqa: F401  (re-exported to the two test files)

COUNT, OFFSET = 256, 777


def mk(*parts, **kw):
    out = {}
    for p in parts:
        out.update(p)
    out.update(kw)
    return out


def workloads():
    L = _L()
    SLOW, CONST, UNIF, GEO = L.DELAY_SLOWSET, L.DELAY_CONST, L.DELAY_UNIFORM, L.DELAY_GEOMETRIC
    base = dict(protocol="consensus", step_cap=4000, proposals=L.PROPOSALS_PHILOX)
    n40 = dict(base, n=40, f=13)
    n64 = dict(base, n=64, f=21)
    n50 = dict(base, n=50, f=16)
    conn = dict(peer_mode=L.PEER_CONNECTION)
    beb = dict(mode=L.MODE_BEB)
    spec = dict(mode=L.MODE_SPEC, coin_seed=COIN)
    loaded = dict(proposals=L.PROPOSALS_LOADED)
    W = {}

    def add(name, kw, step="run", half_step=None, t_floor=0, decides=False, extra=2, count=COUNT):
        W[name] = dict(kw=kw, count=count, step=step, half_step=half_step, t_floor=t_floor, decides=decides,
                       extra=extra)

    # ---- A.  round_cap: the smallest at which the half window overflows, bisected on an MI355X (256 instances
    # from global id 777, lifetime kernel); the tested window overflows nowhere at it.  Constant delays fill a
    # window at Q = 32 only: in lock-step the half window of Q = 64 / 128 and SENDQ_MAX (brc_internal.h: 32
    # SENDs of one replica in one step) are passed in the same step, so no cap separates the two windows
    # (probed: delay 2 and 3, 2 / 8 / 10 silent replicas); part B runs Q = 32 / 64 under a constant delay.
    add("a32-ref-n64-byz", mk(n64, seed=0xA3201, delay_model=SLOW, delay_max=8, key_window=32, round_cap=9,   # half 76
                              byzantine=[0, 63]), half_step="run", decides=True)
    add("a32-beb-slow5-loaded", mk(n40, beb, loaded, seed=0xA3202, delay_model=SLOW, delay_max=5, key_window=32,
                                   round_cap=10, byzantine=[3, 39]), half_step="run")                          # half 49
    add("a32-conn-const2", mk(n40, conn, seed=0xA3203, delay_model=CONST, delay_max=3, delay_const=2, key_window=32,
                              round_cap=27, byzantine=[0, 39]), half_step="run")                               # half 256
    add("a64-ref-nv2-byz", mk(n40, seed=0xA6401, delay_model=SLOW, delay_max=8, key_window=64, variants=2,
                              round_cap=19, byzantine=[0, 39]), step="refuse", half_step="refuse")             # half 86
    add("a64-beb-n64-slow5-loaded", mk(n64, beb, loaded, seed=0xA6402, delay_model=SLOW, delay_max=5, key_window=64,
                                       round_cap=18), step="refuse", half_step="run")                          # half 256
    add("a64-conn-slow5-loaded", mk(n40, conn, loaded, seed=0xA6403, delay_model=SLOW, delay_max=5, key_window=64,
                                    round_cap=25, byzantine=[3, 39]), step="run64", half_step="run")           # half 52
    add("a128-ref-slow8-loaded", mk(n40, loaded, seed=0xA12801, delay_model=SLOW, delay_max=8, key_window=128,
                                    round_cap=39, byzantine=[0, 39]), step="refuse", half_step="refuse")       # half 91
    add("a128-beb-n64-slow5", mk(n64, beb, seed=0xA12802, delay_model=SLOW, delay_max=5, key_window=128,
                                 round_cap=39, byzantine=[0, 63]), step="refuse", half_step="refuse", extra=1)  # half 77
    add("a128-conn-slow8", mk(n40, conn, seed=0xA12803, delay_model=SLOW, delay_max=8, key_window=128,
                              round_cap=39, byzantine=[0, 39]), step="refuse", half_step="run64")              # half 78

    # ---- B.  constant delay 8 (lock-step): past step 256; one slow-set SPEC run past step 128 whose two
    # receiver classes deliver at different late steps
    late = mk(n40, delay_model=CONST, delay_max=8, delay_const=8)
    quiet = [0, 39] + list(range(10, 20))
    for q in (8, 32, 64):
        big = "refuse" if q > 32 else "run"
        add("b-ref-q%d" % q, mk(late, seed=0xB001, key_window=q, round_cap=7, byzantine=quiet), step=big, t_floor=256,
            decides=True)
        # BEB: with a leftover delivery per phase the reference's phase leakage compounds (round cap 2,000 ends at
        # step 168, oracle-measured); f - 1 silent replicas leave exactly n - f + 1 honest ones, so a phase ends
        # on its last delivery: 16 steps per round
        add("b-beb-q%d" % q, mk(late, beb, seed=0xB002, key_window=q, round_cap=20,
                                byzantine=quiet), step=big, t_floor=256, decides=True)
        add("b-conn-q%d" % q, mk(late, conn, seed=0xB003, key_window=q, round_cap=7, byzantine=quiet),
            step="run64" if q > 32 else "run", t_floor=256, decides=True)
    for q in (4, 8):
        add("b-spec-q%d" % q, mk(late, spec, seed=0xB004, key_window=q, round_cap=8), t_floor=256, decides=True)
    add("b-spec-slow8-byz", mk(n40, spec, seed=0xB005, delay_model=SLOW, delay_max=8, key_window=8, round_cap=24,
                                 byzantine=[3, 39]), t_floor=128, decides=True)

    # ---- C.  per-link form, delays above 8 (64-row ring, PB = 1 pending masks): SPEC and BEB
    add("c-spec-geo16-n64", mk(n64, spec, seed=0xC001, delay_model=GEO, delay_max=16, key_window=8, round_cap=2))
    add("c-spec-unif12-n50", mk(n50, spec, seed=0xC002, delay_model=UNIF, delay_max=12, key_window=8, round_cap=3))
    add("c-spec-geo16-n50-byz", mk(n50, spec, seed=0xC003, delay_model=GEO, delay_max=16, key_window=8, round_cap=3,
                                     byzantine=[0, 49, 17]))
    add("c-beb-geo16-n50", mk(n50, beb, seed=0xC004, delay_model=GEO, delay_max=16, key_window=8, round_cap=2))
    add("c-beb-unif12-n64", mk(n64, beb, seed=0xC005, delay_model=UNIF, delay_max=12, key_window=8, round_cap=2))
    add("c-beb-geo16-n64-q16", mk(n64, beb, seed=0xC006, delay_model=GEO, delay_max=16, key_window=16, round_cap=3))

    # ---- D.  SPEC deep into coin rounds (slow-set D = 8, window 8): bench.py times the step kernel there
    add("d-spec-n64-r16", mk(n64, spec, seed=0x5EED0004, delay_model=SLOW, delay_max=8, key_window=8, round_cap=16),
        decides=True)
    add("d-spec-n40-byz-r32", mk(n40, spec, seed=0xD002, delay_model=SLOW, delay_max=8, key_window=8, round_cap=32,
                                   byzantine=[0, 39, 20]), decides=True)
    return W


# Part A: (round cap, instances of the 256 stopped by BRC_OVERFLOW at half the window), as probed
PROBED = {
    "a32-ref-n64-byz": (9, 76),
    "a32-beb-slow5-loaded": (10, 49),
    "a32-conn-const2": (27, 256),
    "a64-ref-nv2-byz": (19, 86),
    "a64-beb-n64-slow5-loaded": (18, 256),
    "a64-conn-slow5-loaded": (25, 52),
    "a128-ref-slow8-loaded": (39, 91),
    "a128-beb-n64-slow5": (39, 77),
    "a128-conn-slow8": (39, 78),
}


def part(prefix):
    return sorted(k for k in workloads() if k.startswith(prefix))


def loaded_props(w):
    """Loaded proposals (value ids 0..3) of a workload's batch, or None."""
    if w["kw"].get("proposals") != _L().PROPOSALS_LOADED:
        return None
    return np.random.RandomState(5).randint(0, 4, size=(w["count"], w["kw"]["n"])).astype(np.int8)


def sample_ids(name, w):
    """The first and the last instance of the batch and `extra` seeded draws between them."""
    rng = random.Random("life-windows/" + name.rsplit("-q", 1)[0])     # one draw for the windows of one workload
    return [0, w["count"] - 1] + sorted(rng.sample(range(1, w["count"] - 1), w["extra"]))


_ORACLE = {}     # oracle results, shared by the workloads that differ in the engine's window only


def oracle_sample(name, w):
    """{id: (result, first decision, last value, decide count per replica)} of the sampled ids; the
    oracle runs once per distinct spec (at most 8 threads)."""
    props = loaded_props(w)
    ids = sample_ids(name, w)
    specs = [_oracle_spec(w["kw"], OFFSET + i, None if props is None else props[i]) for i in ids]
    keys = [json.dumps(sp, sort_keys=True, default=int) for sp in specs]
    todo = [j for j, k in enumerate(keys) if k not in _ORACLE]
    if todo:
        for j, out in zip(todo, _oracle_first_last([specs[j] for j in todo])):
            _ORACLE[keys[j]] = out
    return {i: _ORACLE[k] for i, k in zip(ids, keys)}
