"""The lean step kernels' type-sorted key list (csrc/brc_step.h BRC_TYPED: one list segment and one straight-line
pair body per message-type class, event-log-free builds only) against the single mixed list -- still compiled as
the EV = true twin of every instantiation -- and the C oracle.  Cases: tests/typed_list_workloads.py.

Per case, bit-exact: every instances_result() field, every replicas() record, round_histogram, decisions and every
stats() field (cell_steps, arrivals, deliveries, msgs_sent, lane_loads among them) equal the twin's, and status,
t_stop, msgs_sent, arrivals, cell_steps, deliveries and every honest replica's decisions equal the oracle's.
"""
import pytest

from tests import state_compare as N
from tests import typed_list_workloads as W

pytestmark = pytest.mark.gpu

CASES = W.cases()


def _runner():
    from tests import engine_runner
    return engine_runner


def _check(case, free, twin):
    vs_twin = N.state_mismatches(free, twin, "typed list vs mixed list")
    vs_oracle = N.oracle_mismatches(case, free)
    assert not vs_twin and not vs_oracle, (case.name, vs_twin[:6], vs_oracle[:6])


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_typed_list_equals_mixed_list_and_oracle(name):
    case = W.by_name()[name]
    R = _runner()
    free = R.run_batch_noevents(case.specs, **case.open_kw())          # asserts last_kernel() == "step"
    twin = R.run_batch_noevents(case.specs, event_capacity=1 << 21, **case.open_kw())
    st = free["stats"]
    print(name, {k: st[k] for k in ("done", "quiescent", "overflow", "max_t", "cell_steps", "lane_loads")})
    assert st["running"] == 0 and st["cell_steps"] > 0, (name, st)
    _check(case, free, twin)


@pytest.mark.parametrize("name", ["typed-ref-slow8-cap3", "typed-spec-slow8-cap3", "typed-ref-unif4-cap3"])
def test_sliced_runs_equal_one_run(name):
    """run(2) until nothing is left running (messages in flight across every launch) equals the single run()."""
    case = W.by_name()[name]
    R = _runner()
    whole = R.run_batch_noevents(case.specs, **case.open_kw())
    with R.open_batch(case.specs, **case.open_kw()) as eng:
        launches = 0
        while launches < 4000:
            launches += 1
            if eng.run(2) == 0:
                break
        assert eng.last_kernel() == "step"
        sliced = R.read_state(eng, case.specs)
    diff = N.state_mismatches(whole, sliced, "one run vs slices")
    assert launches >= 2 and not diff, (name, launches, diff[:8])


@pytest.mark.parametrize("mode", ["ref", "spec"])
def test_injection_at_the_current_step(mode):
    """The merge case's Byzantine ECHO injected with t equal to the item's step (the step is entered again: its
    SEND arrivals must not land twice, its list is built a second time) equals the one-shot injection."""
    case = W.by_name()["typed-%s-merge" % mode]
    R = _runner()
    whole = R.run_batch_noevents(case.specs, **case.open_kw())
    trace = {}
    marks = {i: {6} for i in range(case.count)}
    st, _ = R.run_batch_interleaved(case.specs, R.at_now(marks), trace=trace, **case.open_kw())
    assert len(trace["at_now"]) == case.count, trace
    diff = N.state_mismatches(whole, st, "one shot vs injected at the current step")
    assert not diff, (mode, diff[:8])
