"""The key-lifetime kernel's instantiations (csrc/brc_kern_life.hip) that no other test runs against
anything: the HBM-metadata forms (key windows 32 / 64 / 128) under BEB and connection peers and away from
the one cfg4 configuration, every form past step 256 (the 7-bit class delivery code, the 16-bit slot
stamps and the step rings through two wraps), the per-link form's 64-row ring under SPEC and BEB, and
SPEC deep into coin rounds on both kernels.  The workloads are tests/life_window_workloads.py's;
tests/test_life_window_workloads.py checks on the oracle alone that they reach the steps and decision
counts asserted here.

Every workload runs on the lifetime kernel (BRC_KERNEL=life), on the step kernel where the engine takes
the configuration there -- every output must match -- or else brc_create must refuse it as include/brc.h
documents, and sampled global ids (the first, the last, seeded draws) are compared with the C oracle:
counters, every honest replica's first decision, last decided value and decide count; a silent Byzantine
replica records nothing.
"""
import os

import pytest

from tests import life_window_workloads as T
from tests.test_gpu_life import _L, _run

pytestmark = pytest.mark.gpu

IKEYS = ("status", "t_stop", "msgs_sent", "arrivals", "cell_steps", "deliveries", "decided")
CKEYS = ("status", "t_stop", "msgs_sent", "arrivals", "cell_steps")
W = T.workloads()


def _props(w, count):
    p = T.loaded_props(w)
    return None if p is None else p[:count]


def _assert_same(name, life, step):
    """Two runs of one batch: every instance, every replica record, the histograms and the statistics."""
    assert len(life["inst"]) == len(step["inst"])
    for i, (a, b) in enumerate(zip(life["inst"], step["inst"])):
        for k in IKEYS:
            assert a[k] == b[k], (name, i, k, a[k], b[k])
    for i, (a, b) in enumerate(zip(life["reps"], step["reps"])):
        assert a == b, (name, i)
    assert life["hist"] == step["hist"], name
    assert life["dec"] == step["dec"], name
    for k, v in step["stats"].items():
        if k not in ("lane_loads", "max_t"):
            assert life["stats"][k] == v, (name, k, life["stats"][k], v)


def _assert_step_refuses(name, kw, w):
    """include/brc.h: sender peers with Q * NV > 32 (connection peers with Q * NV = 128) at n in 33..64 run
    on the lifetime kernel only -- BRC_KERNEL=step is refused at brc_create, or at the run."""
    from byzantinerandomizedconsensus_amd.engine import Engine
    L = _L()
    assert kw["key_window"] * kw.get("variants", 1) > (64 if kw.get("peer_mode") == L.PEER_CONNECTION else 32), name
    err = eng = None
    old = os.environ.pop("BRC_KERNEL", None)
    os.environ["BRC_KERNEL"] = "step"
    try:
        eng = Engine(instances=4, instance_offset=T.OFFSET, **kw)
    except L.EngineError as e:
        err = e
    finally:
        os.environ.pop("BRC_KERNEL", None)
        if old is not None:
            os.environ["BRC_KERNEL"] = old
    if eng is not None:
        with eng:
            props = _props(w, 4)
            if props is not None:
                eng.load_proposals(props)
            try:
                eng.run()
            except L.EngineError as e:
                err = e
    assert err is not None, (name, "the step kernel took a lifetime-only configuration")
    assert err.code in (L.E_INVALID, L.E_UNSUPPORTED), (name, err.code)


def _both_kernels(name, w, kw, how, life):
    """`life`: the lifetime kernel's run of the whole batch.  The step kernel's run must equal it (how =
    "run"), or equal the lifetime kernel on the first 64 instances ("run64"), or be refused ("refuse")."""
    if how == "refuse":
        _assert_step_refuses(name, kw, w)
        return None
    count = w["count"] if how == "run" else 64
    step = _run(kw, count, T.OFFSET, "step", _props(w, count))
    if count != w["count"]:
        whole = life
        life = _run(kw, count, T.OFFSET, "life", _props(w, count))
        assert life["inst"] == whole["inst"][:count] and life["reps"] == whole["reps"][:count], name
    _assert_same(name, life, step)
    return step


def _assert_oracle(name, w, run):
    kw = w["kw"]
    byz = kw.get("byzantine", ())
    for i, (exp, first, last, count) in T.oracle_sample(name, w).items():
        r = run["inst"][i]
        print(name, "id", T.OFFSET + i, "oracle", {k: exp[k] for k in CKEYS}, "engine", {k: r[k] for k in CKEYS})
        assert exp["t_stop"] > w["t_floor"], (name, i, exp["t_stop"])     # the workload reaches the late steps
        for k in CKEYS:
            assert r[k] == exp[k], (name, i, k, r[k], exp[k])
        for d, rep in enumerate(run["reps"][i]):
            if d in byz:
                assert rep["decide_count"] == 0 and rep["round"] == 0 and rep["value_count"] == 0, (name, i, d, rep)
                assert d not in first, (name, i, d)
                continue
            assert rep["decide_count"] == count.get(d, 0), (name, i, d, rep["decide_count"], count.get(d, 0))
            if w["decides"]:
                assert rep["decide_count"] >= kw["round_cap"], (name, i, d, rep["decide_count"])
            if d in first:
                got = (rep["first_decide_round"], rep["first_decide_t"], rep["first_decide_value"])
                assert got == first[d], (name, i, d, got, first[d])
                assert rep["last_decide_value"] == last[d], (name, i, d)


def _check(name):
    w = W[name]
    kw = w["kw"]
    life = _run(kw, w["count"], T.OFFSET, "life", _props(w, w["count"]))     # asserts last_kernel() == "life"
    st = life["stats"]
    print(name, "life", {k: st[k] for k in ("done", "quiescent", "overflow", "max_t")})
    assert st["running"] == 0 and st["overflow"] == 0, (name, st)
    assert st["max_t"] > w["t_floor"], (name, st["max_t"])
    _both_kernels(name, w, kw, w["step"], life)
    _assert_oracle(name, w, life)
    return life


@pytest.mark.parametrize("name", T.part("a"))
def test_hbm_metadata_windows_in_use(name):
    """Part A: key windows 32 / 64 / 128 x REFERENCE / BEB / connection peers, with padding lanes, silent
    Byzantine replicas (lane 0 and the last real lane), two key variants, loaded proposals, constant and
    slow-set delays.  The window is in use: the same batch at half the window overflows somewhere (and,
    where the step kernel takes the half window, it stops the same instances at the same step); at the
    tested window nothing overflows."""
    w = W[name]
    _check(name)
    half = dict(w["kw"], key_window=w["kw"]["key_window"] // 2)
    hl = _run(half, w["count"], T.OFFSET, "life", _props(w, w["count"]))
    print(name, "half window", half["key_window"], "overflow", hl["stats"]["overflow"])
    assert hl["stats"]["overflow"] > 0, (name, hl["stats"])
    assert hl["stats"]["overflow"] == T.PROBED[name][1], (name, hl["stats"]["overflow"])     # as recorded in the table
    if w["half_step"] == "refuse":
        _assert_step_refuses(name, half, w)
        return
    count = w["count"] if w["half_step"] == "run" else 64
    hs = _run(half, count, T.OFFSET, "step", _props(w, count))
    for i, (a, b) in enumerate(zip(hl["inst"], hs["inst"])):
        assert (a["status"], a["t_stop"]) == (b["status"], b["t_stop"]), (name, i, a, b)
    if count == w["count"]:
        assert hs["stats"]["overflow"] == hl["stats"]["overflow"], name


@pytest.mark.parametrize("name", T.part("b"))
def test_late_steps_through_two_wraps(name):
    """Part B: every sampled instance stops after step 256 (the slow-set SPEC run: 128), so the class
    delivery codes 0x80 | step mod 128, the slot stamps and the 32-row rings have wrapped twice."""
    w = W[name]
    assert w["t_floor"] >= 128
    _check(name)


@pytest.mark.parametrize("name", T.part("c"))
def test_per_link_ring64_spec_and_beb(name):
    """Part C: launch_life_pl<true, 16> under SPEC and BEB (uniform D = 12, geometric D = 16)."""
    w = W[name]
    assert w["kw"]["delay_max"] > 8 and w["step"] == "run"
    _check(name)


@pytest.mark.parametrize("name", T.part("d"))
def test_spec_deep_coin_rounds_both_kernels(name):
    """Part D: SPEC to round cap 16 (n = 64) and 32 (n = 40, silent Byzantine replicas) on the step kernel
    -- the one bench.py times on its spec and spec64 legs -- and the lifetime kernel, in full, and both
    against the oracle with at least round_cap decisions per honest replica."""
    w = W[name]
    assert w["step"] == "run" and w["decides"]
    life = _check(name)                       # the step kernel's run equals it in every output
    hist = life["hist"]
    assert hist[0] == 0 and sum(hist) == w["count"], (name, hist)
