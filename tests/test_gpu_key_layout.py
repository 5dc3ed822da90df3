"""The run-time key-slot layout -- key window Q x key variants NV -- on every kernel family, against the C oracle.

Every kernel addresses a key slot as (origin * NV + variant) * Q + (s & (Q - 1)) and folds an origin's Q * NV
consecutive slots in its consensus pass; the other parity tables hold Q and NV still (NV = 4 ran nowhere, NV = 2 at
Q = 4 only).  tests/key_layout_workloads.py has one small batch per (family, mode, Q, NV) cell, with Byzantine origins
that use every variant (specs.variant_actions); tests/test_key_layout_workloads.py checks on the oracle alone that
the variant slots carry arrivals and that a Byzantine key is delivered by every honest replica in each family.

Per case, bit-exact: the event-log-free build equals its event-log twin (every instances_result() field, every
replicas() record, round_histogram, decisions, every stats() field), both equal the oracle on the compared ids, and
the twin's sorted DELIVER / DECIDE / SEND lists equal the oracle's (a = kp is in the event: a delivery booked to the
wrong variant slot shows there).  No instance stops with BRC_OVERFLOW.  (The layouts brc_create refuses are checked
without a device, in tests/test_abi.py.)
"""
import pytest

from tests import key_layout_workloads as K
from tests import state_compare as C

pytestmark = pytest.mark.gpu

CASES = K.cases()
STEP_CASES = [c.name for c in CASES if c.kernel == "step"]
LIFE_CASES = [c.name for c in CASES if c.kernel == "life"]


def _runner():
    from tests import engine_runner
    return engine_runner


def _run(case, event_capacity=0, specs=None):
    """(read_state(), the event log per instance or None) of the case's batch on its kernel."""
    R = _runner()
    specs = case.specs if specs is None else specs
    if specs[0].get("wide_records"):
        from tests import wide_records_runner
        return wide_records_runner.run_flagged(specs, event_capacity, case.key_window)
    if event_capacity:
        return R.run_batch_noevents(specs, event_capacity=event_capacity, with_events=True, **case.open_kw())
    return R.run_batch_noevents(specs, **case.open_kw()), None


def _clean(name, st):
    s = st["stats"]
    assert s["overflow"] == 0 and s["running"] == 0 and s["events_dropped"] == 0, (name, s)


@pytest.mark.parametrize("name", STEP_CASES)
def test_layout_case_equals_twin_oracle_and_event_lists(name):
    case = K.by_name()[name]
    want_events = K.oracle_events(case)              # (fills the oracle cache of state_compare)
    free, _ = _run(case)
    twin, events = _run(case, event_capacity=1 << 21)
    print(name, case.inst, {k: free["stats"][k] for k in ("done", "quiescent", "overflow", "max_t", "cell_steps")})
    _clean(name, free)
    _clean(name, twin)
    vs_twin = C.state_mismatches(free, twin, "event-free vs twin")
    vs_oracle, twin_vs_oracle = C.oracle_mismatches(case, free), C.oracle_mismatches(case, twin)
    assert not vs_twin and not vs_oracle and not twin_vs_oracle, (name, vs_twin[:6], vs_oracle[:6], twin_vs_oracle[:6])
    for i, want in want_events.items():
        for k in ("deliver", "decide", "send"):
            assert events[i][k] == want[k], (name, i, k, len(events[i][k]), len(want[k]),
                                             [x for x in events[i][k] if x not in want[k]][:4],
                                             [x for x in want[k] if x not in events[i][k]][:4])


@pytest.mark.parametrize("name", LIFE_CASES)
def test_lifetime_kernel_equals_step_kernel_and_oracle(name):
    """The key-lifetime kernel takes no injections: the Byzantine replicas are silent and NV shows in the slot stride
    alone.  It equals the oracle on the compared ids, and the step kernel where brc_create gives that one the batch."""
    R = _runner()
    case = K.by_name()[name]
    K.oracle_events(case)
    life, _ = _run(case)                             # (run_batch_noevents asserts last_kernel() == "life")
    _clean(name, life)
    vs_oracle = C.oracle_mismatches(case, life)
    assert not vs_oracle, (name, vs_oracle[:6])
    step_ok = K.accepted(case.specs[0], case.q, kernel="step", proposals="philox") == "step"
    print(name, "step kernel too" if step_ok else "lifetime kernel only", {k: life["stats"][k] for k in ("done", "max_t", "cell_steps")})
    if step_ok:
        step = R.run_batch_noevents(case.specs, **dict(case.open_kw(), kernel="step"))
        # (lane_loads and max_t count a kernel's own work: tests/test_gpu_life.py)
        strip = lambda st: dict(st, stats={k: v for k, v in st["stats"].items() if k not in ("lane_loads", "max_t")})  # noqa: E731
        diff = C.state_mismatches(strip(step), strip(life), "step vs life")
        assert not diff, (name, diff[:8])


# ---- sliced runs and re-keying on NV = 4 -----------------------------------------------------------------------
def _pick(pred):
    found = [c for c in CASES if c.kernel == "step" and c.nv == 4 and c.split in ("even", "skewed") and pred(c)]
    assert found, "no such case in the table"
    return found[0].name


STEPPED = {"packed": _pick(lambda c: c.family == "packed" and c.specs[0]["n"] == 16 and c.consensus and c.specs[0]["dmax"] >= 3),
           "wide": _pick(lambda c: c.family == "wide" and c.specs[0]["dmax"] >= 4 and not c.specs[0].get("wide_records"))}


@pytest.mark.parametrize("label", sorted(STEPPED))
def test_sliced_runs_equal_one_run(label):
    """run(3) until nothing is left running (messages in flight across the launch boundaries): every output equals
    the single run()."""
    R = _runner()
    case = K.by_name()[STEPPED[label]]
    whole, _ = _run(case)
    bound = case.specs[0]["step_cap"] // 3 + 2
    with R.open_batch(case.specs, **case.open_kw()) as eng:
        launches = 0
        while launches < bound:
            launches += 1
            if eng.run(3) == 0:
                break
        assert eng.last_kernel() == "step"
        sliced = R.read_state(eng, case.specs)
    print(label, case.name, "launches", launches, "max_t", whole["stats"]["max_t"])
    diff = C.state_mismatches(whole, sliced, "one run vs slices")
    assert not diff, (label, diff[:8])
    assert 2 <= launches < bound and sliced["stats"]["running"] == 0, (label, launches)


@pytest.mark.parametrize("label", sorted(STEPPED))
def test_reset_at_equals_a_fresh_engine(label):
    """[A, A + count) to the end, reset_at(A + count) with the same actions injected again and a second run,
    reset_at(A) and a third: the second equals a fresh engine created at A + count, the third the first."""
    R = _runner()
    case = K.by_name()[STEPPED[label]]
    moved = [dict(sp, g=sp["g"] + case.count) for sp in case.specs]
    if case.run["proposals"] == "philox":
        # the propose actions are the Philox draws of the instance's global id (never injected): the moved specs'
        # own, for read-out bookkeeping only
        moved = [dict(case._make(K.OFFSET + case.count + i), name=sp["name"]) for i, sp in enumerate(case.specs)]
    fresh_a, _ = _run(case)
    fresh_b, _ = _run(case, specs=moved)
    assert C.state_mismatches(fresh_a, fresh_b, "A vs B"), (label, "the two id ranges give one result: nothing is shown")
    skip = ("propose",) if case.run["proposals"] != "inject" else ()

    def inject(eng):
        inj = []
        for i, sp in enumerate(case.specs):
            inj += R._injections(dict(sp, actions=[a for a in sp["actions"] if a["kind"] not in skip]), i)
        eng.inject(inj)
    with R.open_batch(case.specs, **case.open_kw()) as eng:
        eng.run()
        first = R.read_state(eng, case.specs)
        eng.reset_at(K.OFFSET + case.count)
        inject(eng)
        eng.run()
        assert eng.last_kernel() == "step"
        second = R.read_state(eng, case.specs)
        eng.reset_at(K.OFFSET)
        inject(eng)
        eng.run()
        third = R.read_state(eng, case.specs)
    for got, want, what in ((first, fresh_a, "first run vs fresh engine"), (second, fresh_b, "reset_at(A + count) vs fresh engine"),
                            (third, fresh_a, "reset_at(A) vs fresh engine")):
        diff = C.state_mismatches(want, got, what)
        assert not diff, (label, diff[:8])
