"""The event-log-free builds of the step kernels -- brc_step<NPAD, DM, false, MODE, NLR> and
brc_step_wide<NPAD, DM, false, MODE, WV>, the ones bench.py and configs.py time -- against their EV = true
twins and the C oracle.  tests/engine_runner.run_batch asks for an event log, so the parity tests built on it
(test_gpu_parity, _wide, _spec, _beb, _workloads, _lean_pairs and the fixtures) launch only the EV = true
builds, which get 256 VGPRs by their launch bounds; the EV = false builds are held to 128-168 VGPRs and spill,
the WV = 4 wide kernels exist only without an event log, and the lean key loop skips the slot-metadata read
there.  tests/step_noevent_workloads.py has one small batch per compiled EV = false instantiation (104 reachable
of 108, plus BRB at n = NPAD on the wide kernels); tests/test_step_noevent_workloads.py checks on the oracle alone
that each of them does real work.

Per case, bit-exact: the batch without an event log equals the same batch, same inputs, with one (every
instances_result() field, every replicas() record, round_histogram, decisions, every stats() field), and equals
the oracle on every instance (n <= 32) or on the first, the last and a seeded id: status, t_stop, msgs_sent,
arrivals, cell_steps, deliveries, and every honest replica's first decision, last decided value and decide count.

`deliveries` counts BRB deliveries at honest replicas (brc_step.h st_del: one per (replica, key) cell that
delivers), which is the oracle's deliver-event count.

On six representative cases the same build also runs in slices of three steps (state carried across launches
with messages in flight) and is re-keyed with reset_at; both must reproduce a single run of a fresh engine.
"""
import pytest

from tests import step_noevent_workloads as T

pytestmark = pytest.mark.gpu

CASES = T.cases()
CKEYS = ("status", "t_stop", "msgs_sent", "arrivals", "cell_steps")


def _runner():
    from tests import engine_runner
    return engine_runner


def state_mismatches(a, b, what):
    """Differences between two read_state() results of one batch: nothing is left out."""
    out = []
    if len(a["inst"]) != len(b["inst"]):
        return [(what, "instances", len(a["inst"]), len(b["inst"]))]
    for i, (x, y) in enumerate(zip(a["inst"], b["inst"])):
        out += [(what, "inst", i, k, x[k], y[k]) for k in x if x[k] != y[k]]
    for i, (x, y) in enumerate(zip(a["reps"], b["reps"])):
        for d, (p, q) in enumerate(zip(x, y)):
            out += [(what, "replica", i, d, k, p[k], q[k]) for k in p if p[k] != q[k]]
    if a["hist"] != b["hist"]:
        out.append((what, "round_histogram", a["hist"], b["hist"]))
    if a["dec"] != b["dec"]:
        out.append((what, "decisions", a["dec"], b["dec"]))
    out += [(what, "stats", k, v, b["stats"][k]) for k, v in a["stats"].items() if v != b["stats"][k]]
    return out


def oracle_mismatches(case, st):
    out = []
    byz = set(case.specs[0]["byzantine"])
    for i, (exp, dec, delivers) in T.oracle_results(case).items():
        r = st["inst"][i]
        out += [("oracle", i, k, r[k], exp[k]) for k in CKEYS if r[k] != exp[k]]
        if r["deliveries"] != delivers:
            out.append(("oracle", i, "deliveries", r["deliveries"], delivers))
        for d, rep in enumerate(st["reps"][i]):
            if d in byz:
                continue
            mine = dec.get(d, [])
            if rep["decide_count"] != len(mine):
                out.append(("oracle", i, d, "decide_count", rep["decide_count"], len(mine)))
            if mine:
                got = (rep["first_decide_round"], rep["first_decide_t"], rep["first_decide_value"])
                if got != mine[0]:
                    out.append(("oracle", i, d, "first decision", got, mine[0]))
                if rep["last_decide_value"] != mine[-1][2]:
                    out.append(("oracle", i, d, "last value", rep["last_decide_value"], mine[-1][2]))
        want = all(d in dec for d in range(case.specs[0]["n"]) if d not in byz) and case.consensus
        if bool(r["decided"]) != want:
            out.append(("oracle", i, "decided", r["decided"], want))
    return out


def check_case(case):
    """(event-free state, mismatches event-free vs twin, event-free vs oracle, twin vs oracle)."""
    R = _runner()
    free = R.run_batch_noevents(case.specs, **case.open_kw())
    twin = R.run_batch_noevents(case.specs, event_capacity=1 << 21, **case.open_kw())
    return free, state_mismatches(free, twin, "event-free vs twin"), oracle_mismatches(case, free), oracle_mismatches(case, twin)


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_event_free_build_equals_twin_and_oracle(name):
    case = T.by_name()[name]
    free, vs_twin, vs_oracle, twin_vs_oracle = check_case(case)
    st = free["stats"]
    print(name, case.inst, {k: st[k] for k in ("done", "quiescent", "overflow", "max_t", "cell_steps")})
    assert st["running"] == 0 and st["events_dropped"] == 0, (name, st)
    # a difference places itself: the twin alone matching the oracle is a defect of the event-free build,
    # both missing it a protocol defect
    assert not vs_twin and not vs_oracle, (name, vs_twin[:6], vs_oracle[:6], "twin vs oracle", twin_vs_oracle[:6])


# ---- stepped runs and re-keying on the event-free build ------------------------------------------------
def _pick(pred):
    found = [c for c in CASES if c.consensus and c.specs[0]["dmax"] > 3 and pred(c, c.specs[0])]
    assert found, "no such case in the table"
    return found[0].name


STEPPED = {
    "packed-ref-n7": _pick(lambda c, sp: c.inst[:2] == ("step", 8) and c.inst[3] == T.REF and sp["n"] == 7),
    "packed-spec-n16": _pick(lambda c, sp: c.inst[:2] == ("step", 16) and c.inst[3] == T.SPEC and sp["n"] == 16),
    "packed-conn-n16": _pick(lambda c, sp: c.inst[:2] == ("step", 16) and c.inst[3] == T.CONN and sp["n"] == 16),
    "lean-n64-slowset": _pick(lambda c, sp: c.inst[:2] == ("step", 64) and c.inst[4] == 2 and sp["n"] == 64 and
                              sp["delay_model"] == T.SLOW and sp["dmax"] <= 8),
    "wide128-wv4": _pick(lambda c, sp: c.inst[:2] == ("wide", 128) and c.inst[4] == 4 and sp["delay_model"] == T.SLOW),
    "wide256-uniform": _pick(lambda c, sp: c.inst[:2] == ("wide", 256) and c.inst[4] == 0 and sp["delay_model"] == T.UNIF),
}
REKEYED = dict(STEPPED, **{"packed-loaded": _pick(lambda c, sp: c.inst[1] < 64 and c.run["proposals"] == "loaded")})


@pytest.mark.parametrize("label", sorted(STEPPED))
def test_sliced_runs_equal_one_run(label):
    """run(3) until nothing is left running: three steps are fewer than the largest delay, so messages are in
    flight across every launch boundary; every output equals the single run()."""
    R = _runner()
    case = T.by_name()[STEPPED[label]]
    assert case.specs[0]["dmax"] > 3
    whole = R.run_batch_noevents(case.specs, **case.open_kw())
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
    diff = state_mismatches(whole, sliced, "one run vs slices")
    assert not diff, (label, diff[:8])
    # max_steps counts processed steps (the kernels jump over steps without arrivals): several launches each
    assert 2 <= launches < bound and sliced["stats"]["running"] == 0, (label, launches)


@pytest.mark.parametrize("label", sorted(REKEYED))
def test_reset_at_equals_a_fresh_engine(label):
    """[A, A + count) to the end, reset_at(A + count) and a second run, reset_at(A) and a third: the second
    equals a fresh engine created at A + count (stale cells, generation tags, the lean rows rewritten), the
    third the first.  Loaded proposals are indexed by the engine-local instance and stay across reset_at
    (include/brc.h), so the fresh engine loads the same ones."""
    R = _runner()
    case = T.by_name()[REKEYED[label]]
    moved = [dict(sp, g=sp["g"] + case.count) for sp in case.specs]      # the same inputs, re-keyed
    fresh_a = R.run_batch_noevents(case.specs, **case.open_kw())
    fresh_b = R.run_batch_noevents(moved, **case.open_kw())
    assert state_mismatches(fresh_a, fresh_b, "A vs B"), (label, "the two id ranges give one result: nothing is shown")
    with R.open_batch(case.specs, **case.open_kw()) as eng:
        eng.run()
        first = R.read_state(eng, case.specs)
        eng.reset_at(T.OFFSET + case.count)
        eng.run()
        assert eng.last_kernel() == "step"
        second = R.read_state(eng, case.specs)
        eng.reset_at(T.OFFSET)
        eng.run()
        assert eng.last_kernel() == "step"
        third = R.read_state(eng, case.specs)
    for got, want, what in ((first, fresh_a, "first run vs fresh engine"), (second, fresh_b, "reset_at(A + count) vs fresh engine"),
                            (third, fresh_a, "reset_at(A) vs fresh engine")):
        diff = state_mismatches(want, got, what)
        assert not diff, (label, diff[:8])
