"""The lean typed step kernels' unwritten rows (csrc/brc_step.h BRC_FRESH_SEND: a new key's cell row is first written
by its first SEND key-step, or by whatever else touches it before) against the EV = true twin of the same
instantiation -- no typed list there, rows written when the slot is allocated -- and the C oracle.  Cases:
tests/fresh_send_workloads.py; what each contains is proved by tests/test_fresh_send_workloads.py.

Per case, bit-exact, every instance: every instances_result() field, every replicas() record, round_histogram,
decisions and every stats() field (cell_steps, arrivals, deliveries, msgs_sent, lane_loads = wave-key-steps x 64 among
them) equal the twin's, and status, t_stop, msgs_sent, arrivals, cell_steps, deliveries and every honest replica's
decisions equal the oracle's.
"""
import pytest

from tests import fresh_send_workloads as W
from tests import state_compare as N

pytestmark = pytest.mark.gpu

CASES = W.cases()


def _runner():
    from tests import engine_runner
    return engine_runner


def _check(case, free, twin):
    vs_twin = N.state_mismatches(free, twin, "unwritten rows vs rows written at allocation")
    vs_oracle = N.oracle_mismatches(case, free)
    assert not vs_twin and not vs_oracle, (case.name, vs_twin[:6], vs_oracle[:6])


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_fresh_rows_equal_twin_and_oracle(name):
    case = W.by_name()[name]
    R = _runner()
    free = R.run_batch_noevents(case.specs, **case.open_kw())          # asserts last_kernel() == "step"
    twin = R.run_batch_noevents(case.specs, event_capacity=1 << 21, **case.open_kw())
    st = free["stats"]
    print(name, {k: st[k] for k in ("done", "quiescent", "stepcap", "overflow", "max_t", "cell_steps", "lane_loads")})
    assert st["running"] == 0 and st["overflow"] == 0 and st["cell_steps"] > 0, (name, st)
    _check(case, free, twin)


@pytest.mark.parametrize("name", W.SLICED)
def test_one_step_slices_equal_one_run(name):
    """run(1) until nothing is left running: a launch boundary after every step, so one falls between every slot's
    allocation and its first SEND landing (the exit writes the rows still unwritten; the next launch finds none)."""
    case = W.by_name()[name]
    R = _runner()
    whole = R.run_batch_noevents(case.specs, **case.open_kw())
    with R.open_batch(case.specs, **case.open_kw()) as eng:
        launches = 0
        while launches < 4000:
            launches += 1
            if eng.run(1) == 0:
                break
        assert eng.last_kernel() == "step"
        sliced = R.read_state(eng, case.specs)
    diff = N.state_mismatches(whole, sliced, "one run vs one-step slices")
    assert launches >= 4 and not diff, (name, launches, diff[:8])
    assert not N.oracle_mismatches(case, sliced)


@pytest.mark.parametrize("name", W.INTERLEAVED)
def test_injection_between_slices(name):
    """The Byzantine ECHOs / READYs of step 1, for keys whose SEND is still in flight, stay on the host until every
    instance stands at step 1 (its fast origins' SENDs land there, so run(1) stops there) and go in between two
    one-step slices with t equal to the item's step: the exit of the slice before wrote the rows, and step 1 is
    entered again for the actions alone."""
    case = W.by_name()[name]
    R = _runner()
    whole = R.run_batch_noevents(case.specs, **case.open_kw())
    trace = {}
    marks = {i: {1} for i in range(case.count)}
    st, _ = R.run_batch_interleaved(case.specs, R.at_now(marks), trace=trace, **case.open_kw())
    assert len(trace["at_now"]) == case.count and trace["pieces"] >= 2 and trace["slices"] >= 4, trace
    diff = N.state_mismatches(whole, st, "one shot vs injected between slices")
    assert not diff, (name, diff[:8])


@pytest.mark.parametrize("name", W.LATE)
def test_late_steps(name):
    """Every action W.LATE_T0 steps later (tests/time_axis_workloads.shift).  The step loop moves the epoch on entering
    a step, before that step's actions: in the early and reuse cases step T0 jumps ~60,000 steps with every slot still
    empty, and the keys allocated there are within C32_REBASE of the new epoch until they are written.  The declared
    case is the one that puts an unwritten slot in front of rebase(): its key is declared at T0 and the next step the
    kernel visits after the first burst is T0 + 120, more than C32_REBASE later, which moves the epoch again with
    that slot still unwritten (rebase() skips it; its SEND then lands on the fresh row)."""
    from tests import time_axis_workloads as TA
    base = W.by_name()[name]
    case = W.Case(base.name + "-late", base.inst, None, base.count, base.run, base.key_window, consensus=base.consensus)
    case._specs = [dict(TA.shift(sp, W.LATE_T0), name=sp["name"] + "-late") for sp in base.specs]
    R = _runner()
    free = R.run_batch_noevents(case.specs, **case.open_kw())
    twin = R.run_batch_noevents(case.specs, event_capacity=1 << 21, **case.open_kw())
    assert free["stats"]["max_t"] > W.LATE_T0 and free["stats"]["stepcap"] == 0
    _check(case, free, twin)


@pytest.mark.parametrize("name", [c.name for c in W.mask_cases()])
def test_per_instance_byzantine_masks(name):
    """Every instance under its own Byzantine mask (brc_load_byzantine over a configuration mask equal to none of
    them): the fresh store's hit lanes come from the wave's own honest mask.  Against the EV twin, every field, and
    the oracle, every instance, honest meaning honest under the instance's own mask (tests/test_gpu_byz_masks.py's
    comparison)."""
    from tests.test_gpu_byz_masks import oracle_mismatches
    case = next(c for c in W.mask_cases() if c.name == name)
    R = _runner()
    free = R.run_batch_noevents(case.specs, **case.open_kw())          # asserts last_kernel() == "step"
    twin = R.run_batch_noevents(case.specs, event_capacity=1 << 21, **case.open_kw())
    st = free["stats"]
    print(name, case.inst, {k: st[k] for k in ("done", "quiescent", "overflow", "decided", "max_t", "cell_steps")})
    assert st["running"] == 0 and st["overflow"] == 0, (name, st)
    vs_twin = N.state_mismatches(free, twin, "unwritten rows vs rows written at allocation")
    vs_oracle = oracle_mismatches(case, free)
    assert not vs_twin and not vs_oracle, (name, vs_twin[:6], vs_oracle[:6])
    assert all(not free["inst"][i]["decided"] and free["inst"][i]["status"] == "quiescent" for i in case.stalled())


@pytest.mark.parametrize("name", ["fresh-ref-cut", "fresh-spec-cut"])
def test_cut_run_reset_and_second_run(name):
    """A run stopped by the step cap with SENDs in flight (rows unwritten at the stop), then brc_reset and the same
    run again on the same engine: both equal the oracle and each other."""
    case = W.by_name()[name]
    R = _runner()
    with R.open_batch(case.specs, **case.open_kw()) as eng:
        eng.run()
        assert eng.last_kernel() == "step"
        first = R.read_state(eng, case.specs)
        eng.reset()
        eng.run()
        second = R.read_state(eng, case.specs)
    assert first["stats"]["stepcap"] == case.count, first["stats"]
    diff = N.state_mismatches(first, second, "first run vs the run after brc_reset")
    assert not diff, (name, diff[:8])
    assert not N.oracle_mismatches(case, first)
