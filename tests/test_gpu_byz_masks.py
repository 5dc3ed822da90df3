"""Per-instance Byzantine masks (brc_load_byzantine, include/brc.h) on every kernel against the C oracle.

Every other parity test passes one byzantine= list through brc_config, so all instances of a batch -- and all
segments of a wave on the packed kernels -- share one mask.  tests/byz_mask_workloads.py has small batches whose
instances carry different masks (its docstring has the rules; tests/test_byz_mask_workloads.py checks on the
oracle alone that the masks matter: under its neighbour's mask an instance gives another result).  The engine is
created with a configuration mask that equals none of the loaded ones, which replace it.

Per case, bit-exact: the batch without an event log equals the same batch with one (every field), both equal the
oracle on EVERY instance (status, t_stop, msgs_sent, arrivals, cell_steps, deliveries, decided, every honest
replica's first decision, last value and decide count -- honest under the instance's own mask), the event log's
ordered DELIVER / DECIDE / SEND lists equal the oracle's, and round_histogram(66), decisions() and the
disagreement count equal the values derived from the oracle's decide events.  The key-lifetime cases also run on
the lifetime kernel, which must equal the step kernel.  Three cases are re-keyed with reset_at without reloading
the masks and must equal a fresh engine at the new offset with the same masks loaded.
"""
import pytest

from tests import byz_mask_workloads as B
from tests.test_gpu_step_noevent import state_mismatches

pytestmark = pytest.mark.gpu

CASES = B.cases()


def _runner():
    from tests import engine_runner
    return engine_runner


def oracle_mismatches(case, st, events=None):
    """A read_state() result (and the event log per instance) against the oracle, every instance."""
    out = []
    for i, (exp, dec, delivers) in B.oracle_results(case, events=True).items():
        r = st["inst"][i]
        out += [("oracle", i, k, r[k], exp[k]) for k in B.CKEYS if r[k] != exp[k]]
        if r["deliveries"] != delivers:
            out.append(("oracle", i, "deliveries", r["deliveries"], delivers))
        hon = B.honest(case, i)
        for d in hon:
            rep, mine = st["reps"][i][d], dec.get(d, [])
            if rep["decide_count"] != len(mine):
                out.append(("oracle", i, d, "decide_count", rep["decide_count"], len(mine)))
            if mine:
                got = (rep["first_decide_round"], rep["first_decide_t"], rep["first_decide_value"])
                if got != mine[0]:
                    out.append(("oracle", i, d, "first decision", got, mine[0]))
                if rep["last_decide_value"] != mine[-1][2]:
                    out.append(("oracle", i, d, "last value", rep["last_decide_value"], mine[-1][2]))
        want = case.consensus and all(d in dec for d in hon)
        if bool(r["decided"]) != want:
            out.append(("oracle", i, "decided", r["decided"], want))
        if events is not None:
            out += [("oracle", i, k + " events", len(events[i][k]), len(exp["events"][k]))
                    for k in ("deliver", "decide", "send") if events[i][k] != exp["events"][k]]
    return out


def read_side_mismatches(case, st):
    if not case.consensus:
        return [("read side", k, st[k]) for k in ("hist", "dec") if st[k] is not None]
    hist, counts, undecided, dis = B.expected_read_side(case)
    labels = case.specs[0]["values"]
    want = {labels[v]: counts.get(v, 0) for v in range(len(labels) if len(labels) == 8 else 4)}
    want["undecided"] = undecided
    out = []
    if st["hist"] != hist:
        out.append(("round_histogram", st["hist"], hist))
    if st["dec"] != (want, dis):
        out.append(("decisions", st["dec"], (want, dis)))
    return out


def life_mismatches(life, step):
    """The lifetime kernel against the step kernel: everything but the two statistics that describe the kernel's
    own work (lane_loads, max_t; tests/test_gpu_life.py)."""
    strip = lambda st: dict(st, stats={k: v for k, v in st["stats"].items() if k not in ("lane_loads", "max_t")})  # noqa: E731
    return state_mismatches(strip(step), strip(life), "step kernel vs lifetime kernel")


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_loaded_masks_equal_the_oracle(name):
    R = _runner()
    case = B.by_name()[name]
    free = R.run_batch_noevents(case.specs, **case.open_kw())
    twin, events = R.run_batch_noevents(case.specs, event_capacity=1 << 21, with_events=True, **case.open_kw())
    st = free["stats"]
    print(name, case.inst, {k: st[k] for k in ("done", "quiescent", "overflow", "decided", "max_t", "cell_steps")})
    assert st["running"] == 0 and twin["stats"]["events_dropped"] == 0, (name, st)
    vs_twin = state_mismatches(free, twin, "event-free vs twin")
    vs_oracle = oracle_mismatches(case, free)
    twin_vs_oracle = oracle_mismatches(case, twin, events)
    assert not vs_twin and not vs_oracle and not twin_vs_oracle, (name, vs_twin[:6], vs_oracle[:6], twin_vs_oracle[:6])
    read = read_side_mismatches(case, free) + read_side_mismatches(case, twin)
    assert not read, (name, read)
    if case.stalled():
        assert free["hist"][0] >= len(case.stalled()) and free["dec"][0]["undecided"] > 0
        assert all(not free["inst"][i]["decided"] and free["inst"][i]["status"] == "quiescent" for i in case.stalled())
    if case.kernel == "life":
        life = R.run_batch_noevents(case.specs, **case.open_kw(kernel="life"))
        diff = life_mismatches(life, free) + oracle_mismatches(case, life) + read_side_mismatches(case, life)
        assert not diff, (name, diff[:8])


REKEYED = {"packed": "p16-ref-n13-slow8", "lean": "n64-lean-ref-slow8", "wide": "w128-ref-n70-slow8"}


@pytest.mark.parametrize("label", sorted(REKEYED))
def test_reset_at_keeps_the_loaded_masks(label):
    """Run, reset_at(777 + count) and run again without reloading: brc_reset_at keeps the loaded masks (indexed
    by the engine-local instance), so the second run equals a fresh engine created at the new offset with the same
    masks loaded -- and differs from the first."""
    R = _runner()
    case = B.by_name()[REKEYED[label]]
    moved = [dict(sp, g=sp["g"] + case.count) for sp in case.specs]
    fresh_a = R.run_batch_noevents(case.specs, **case.open_kw())
    fresh_b = R.run_batch_noevents(moved, **case.open_kw())
    assert state_mismatches(fresh_a, fresh_b, "A vs B"), (label, "the two id ranges give one result: nothing is shown")
    with R.open_batch(case.specs, **case.open_kw()) as eng:
        eng.run()
        first = R.read_state(eng, case.specs)
        eng.reset_at(B.OFFSET + case.count)
        eng.run()
        assert eng.last_kernel() == "step"
        second = R.read_state(eng, case.specs)
    for got, want, what in ((first, fresh_a, "first run vs fresh engine"), (second, fresh_b, "reset_at vs fresh engine")):
        diff = state_mismatches(want, got, what)
        assert not diff, (label, diff[:8])
