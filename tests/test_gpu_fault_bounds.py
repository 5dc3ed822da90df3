"""Fault bounds off f = (n - 1) // 3 and committees below 4 on every kernel family, against the C oracle.

Each kernel header (brc_step.h, brc_step_wide.h, brc_life.h, brc_life_cell.h, brc_life_wide.h) restates the quorum
comparisons > n - f, 2 * count > n + f, > 2 * f and > f inline, and derives the two-class receiver classes from the
slow set, whose size is f.  tests/fault_bound_workloads.py has one small batch per (family, n, f) shape at
f in {0, (n - 1) // 3 + 1, ceil(n / 2), n - 1}; tests/test_fault_bound_workloads.py checks on the oracle alone that f
matters (under the standard bound at least half of the instances give another result) and that the regimes are real;
the oracle itself is pinned there by the reference fixture tests/golden/fault_bounds/fault_bounds.json.

Per case, bit-exact: the batch without an event log equals the same batch with one (every instances_result() field,
every replicas() record, round_histogram, decisions, every stats() field); both equal the oracle -- on every instance
at n <= 64, on the first, the last and two seeded ids between at n > 64 -- and at n <= 64 the log's ordered
DELIVER / DECIDE / SEND lists equal the oracle's.  The key-lifetime cases (which take no event log) run on their kernel
and on the step kernel (BRC_KERNEL=step; an unflagged engine above 64) and must agree field for field.  The three *-ovf
cases stop instances with BRC_OVERFLOW, which the oracle does not model: there the two builds must agree in every
field, and the instances that did not overflow equal the oracle.  The fixture runs through the C-ABI as
tests/test_gpu_parity.py runs fixtures; two cases run in slices of three steps and after brc_reset_at.
"""
import json
import os

import pytest

from tests import fault_bound_workloads as F
from tests import golden_io
from tests.state_compare import state_mismatches

pytestmark = pytest.mark.gpu

CASES = F.cases()
LOG = 1 << 21


def _runner():
    from tests import engine_runner
    return engine_runner


def _strip(st):
    """lane_loads and max_t count a kernel's own work (tests/test_gpu_life.py)."""
    return dict(st, stats={k: v for k, v in st["stats"].items() if k not in ("lane_loads", "max_t")})


def _flagged(case, specs):
    """The wide key-lifetime engine of a case (BRC_FLAG_WIDE_LIFE, and BRC_FLAG_LIFE_PATTERN with the engine's own
    equivocation pattern), run: read_state()."""
    from byzantinerandomizedconsensus_amd import _lib as L
    from byzantinerandomizedconsensus_amd.engine import Engine
    R = _runner()
    sp0 = specs[0]
    pattern = case.kind == "pattern"
    mode = L.MODE_SPEC if sp0["mode"] == "spec" else L.MODE_BEB if sp0["mode"].startswith("beb") else L.MODE_REFERENCE
    eng = Engine(n=case.n, f=case.f, instances=len(specs), protocol="consensus", seed=sp0["seed"],
                 delay_model=sp0["delay_model"], delay_max=sp0["dmax"], delay_const=sp0.get("dconst", 1),
                 round_cap=sp0["round_cap"], step_cap=sp0["step_cap"], key_window=case.q, variants=case.nv,
                 byzantine=case.cfg_byz if case.masks else (), instance_offset=sp0["g"], mode=mode,
                 coin_seed=sp0.get("coin_seed", 0), proposals=L.PROPOSALS_PHILOX,
                 byz_pattern=L.BYZ_EQUIVOCATE if pattern else L.BYZ_NONE, wide_life=True, life_pattern=pattern)
    with eng:
        if case.masks:
            eng.load_byzantine(R.mask_words(specs))
        assert eng.last_kernel() == "life"
        eng.run()
        assert eng.last_kernel() == "life"
        return R.read_state(eng, specs)


def _step(case, specs, log=False, **kw):
    """The batch on the step kernel: (read_state(), the event log per instance or None)."""
    R = _runner()
    if case.kind == "records":
        from tests import wide_records_runner
        return wide_records_runner.run_flagged(specs, LOG if log else 0, case.key_window)
    okw = case.open_kw(kernel="step", **kw)
    if case.kind == "pattern":
        okw["byz_pattern"] = True
    if log:
        return R.run_batch_noevents(specs, event_capacity=LOG, with_events=True, **okw)
    return R.run_batch_noevents(specs, **okw), None


def oracle_mismatches(case, st, events=None, skip=()):
    """A read_state() result (and the event log per instance) against the oracle on the compared ids; over a whole
    batch also the round histogram and the decision histogram."""
    out = []
    res = {i: r for i, r in F.oracle_results(case).items() if i not in skip}
    for i, (exp, dec, delivers) in res.items():
        r = st["inst"][i]
        out += [("oracle", i, k, r[k], exp[k]) for k in F.CKEYS if r[k] != exp[k]]
        if r["deliveries"] != delivers:
            out.append(("oracle", i, "deliveries", r["deliveries"], delivers))
        hon = [d for d in range(case.n) if d not in case.byz(i)]
        for d in hon:
            rep, mine = st["reps"][i][d], dec.get(d, [])
            if rep["decide_count"] != len(mine):
                out.append(("oracle", i, d, "decide_count", rep["decide_count"], len(mine)))
            if mine:
                got = (rep["first_decide_round"], rep["first_decide_t"], rep["first_decide_value"])
                if got != mine[0] or rep["last_decide_value"] != mine[-1][2]:
                    out.append(("oracle", i, d, "decisions", got, rep["last_decide_value"], mine[0], mine[-1][2]))
        want = case.consensus and all(d in dec for d in hon)
        if bool(r["decided"]) != want:
            out.append(("oracle", i, "decided", r["decided"], want))
        if events is not None and case.n <= 64:
            out += [("oracle", i, k + " events", len(events[i][k]), len(exp["events"][k]))
                    for k in ("deliver", "decide", "send") if events[i][k] != exp["events"][k]]
    if case.consensus and len(res) == case.count:
        hist, counts, undecided, dis = F.expected_read_side(case, res)
        labels = case.specs[0]["values"]
        want = {labels[v]: counts.get(v, 0) for v in range(len(labels) if len(labels) == 8 else 4)}
        want["undecided"] = undecided
        if st["hist"] != hist:
            out.append(("oracle", "round_histogram", st["hist"], hist))
        if st["dec"] != (want, dis):
            out.append(("oracle", "decisions", st["dec"], (want, dis)))
    return out


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_case_equals_twin_oracle_and_event_lists(name):
    case = F.by_name()[name]
    specs = case.specs
    free, _ = _step(case, specs)
    twin, events = _step(case, specs, log=True)
    st = free["stats"]
    print(name, case.inst, {k: st[k] for k in ("done", "quiescent", "stepcap", "overflow", "decided", "max_t", "cell_steps")})
    assert st["running"] == 0 and twin["stats"]["events_dropped"] == 0, (name, st)
    vs_twin = state_mismatches(free, twin, "event-free vs twin")
    assert not vs_twin, (name, vs_twin[:8])
    skip = ()
    if case.overflow:
        skip = [i for i, r in enumerate(free["inst"]) if r["status"] == "overflow"]
        assert skip and st["overflow"] == len(skip) == twin["stats"]["overflow"], (name, st)
    else:
        assert st["overflow"] == 0, (name, st)
    vs_oracle = oracle_mismatches(case, free, skip=skip)
    twin_vs_oracle = oracle_mismatches(case, twin, events, skip=skip)
    assert not vs_oracle and not twin_vs_oracle, (name, vs_oracle[:8], twin_vs_oracle[:8])
    if case.kind in ("life", "wide_life", "pattern"):
        if case.kind == "life":
            life = _runner().run_batch_noevents(specs, **case.open_kw(kernel="life"))
        else:
            life = _flagged(case, specs)
        diff = state_mismatches(_strip(free), _strip(life), "step kernel vs lifetime kernel") + oracle_mismatches(case, life)
        assert not diff, (name, diff[:8])


def test_fixture_through_the_c_abi():
    """The reference's own results at off-standard fault bounds (tests/golden/fault_bounds), as
    tests/test_gpu_parity.py::test_engine_matches_reference_fixtures runs the other fixtures."""
    with open(os.path.join(golden_io.GOLDEN, "fault_bounds", "fault_bounds.json")) as fh:
        cases = json.load(fh)["cases"]
    got = _runner().run_specs([c["spec"] for c in cases])
    for i, (c, r) in enumerate(zip(cases, got)):
        golden_io.assert_matches(c["result"], r, "fault_bounds[%d]" % i)
        assert r["cell_steps"] == c["cell_steps"], (i, r["cell_steps"], c["cell_steps"])


def _moved(case):
    """The case's specs at the next id range, the masks staying with the engine-local instance."""
    return [dict(case.make_f(F.OFFSET + case.count + i, byz=case.byz(i)), name=sp["name"]) for i, sp in enumerate(case.specs)]


@pytest.mark.parametrize("label", sorted(F.SLICED))
def test_sliced_runs_equal_one_run(label):
    """run(3) until nothing is left running (three steps are fewer than the slow delay: messages are in flight across
    the launch boundaries): every output equals the single run()."""
    R = _runner()
    case = F.by_name()[F.SLICED[label]]
    assert case.dmax > 3 and case.f != F.standard(case.n)
    whole, _ = _step(case, case.specs)
    bound = case.specs[0]["step_cap"] // 3 + 2
    with R.open_batch(case.specs, **case.open_kw()) as eng:
        launches = 0
        while launches < bound:
            launches += 1
            if eng.run(3) == 0:
                break
        assert eng.last_kernel() == "step"
        sliced = R.read_state(eng, case.specs)
    diff = state_mismatches(whole, sliced, "one run vs slices")
    assert not diff, (label, diff[:8])
    assert 2 <= launches < bound and sliced["stats"]["running"] == 0, (label, launches)


@pytest.mark.parametrize("label", sorted(F.SLICED))
def test_reset_at_equals_a_fresh_engine(label):
    """Run, brc_reset_at(777 + count), run again: the second run equals a fresh engine created at that offset (the
    loaded masks stay), and differs from the first."""
    R = _runner()
    case = F.by_name()[F.SLICED[label]]
    moved = _moved(case)
    fresh_a, _ = _step(case, case.specs)
    fresh_b, _ = _step(case, moved)
    assert state_mismatches(fresh_a, fresh_b, "A vs B"), (label, "the two id ranges give one result: nothing is shown")
    with R.open_batch(case.specs, **case.open_kw()) as eng:
        eng.run()
        first = R.read_state(eng, case.specs)
        eng.reset_at(F.OFFSET + case.count)
        eng.run()
        assert eng.last_kernel() == "step"
        second = R.read_state(eng, moved)
    for got, want, what in ((first, fresh_a, "first run vs fresh engine"), (second, fresh_b, "reset_at vs fresh engine")):
        diff = state_mismatches(want, got, what)
        assert not diff, (label, diff[:8])
