"""GPU: the time axis on every kernel family, against the C oracle -- runs stopped by the step cap (BRC_STEPCAP) and
runs at late steps, up to STEP_LIMIT.  tests/time_axis_workloads.py has the table (one small batch per family, the
caps derived from the oracle's uncapped run, the late forms shift / two_bursts / cut);
tests/test_time_axis_workloads.py proves its preconditions on the oracle alone.

Per case and cap (or late form), without an event log and with one, bit-exact: every instance equals the oracle in
status, t_stop, msgs_sent, arrivals, cell_steps, deliveries, decided, every honest replica's record and the ordered
DELIVER / DECIDE / SEND lists (no event past the cap); the two builds equal each other in every read_state() field;
stats()["stepcap"], round_histogram (a partially decided instance counts in hist[0]), decisions() and the
disagreement count equal the values derived from the oracle.
"""
import pytest

from tests import time_axis_workloads as W
from tests.state_compare import state_mismatches

pytestmark = pytest.mark.gpu

LOG = 1 << 20
STEP = W.step_cases()
CAP_LABELS = ("zero", "one", "mid", "gap", "last-1", "last")


def _runner():
    from tests import engine_runner, wide_records_runner
    return engine_runner, wide_records_runner


def _L():
    from byzantinerandomizedconsensus_amd import _lib
    return _lib


def open_case(case, specs, cap=0, inject=True):
    """The engine of one batch as the case's family creates it, the specs' actions injected (inject), not yet run."""
    R, F = _runner()
    if not case.flagged:
        return R.open_batch(specs if inject else R._unfed(specs), cap, key_window=case.key_window)
    from byzantinerandomizedconsensus_amd.engine import Engine
    eng = Engine(wide_records=case.wide_records, wide_values=case.wide_values, **F.engine_kw(specs, cap, case.key_window))
    try:
        if inject:
            eng.inject(F.injections(specs))
    except Exception:
        eng.close()
        raise
    return eng


def read(eng, specs, cap):
    R, _F = _runner()
    st = R.read_state(eng, specs)
    ev = None if not cap else [R.sort_result({"events": e})["events"] for e in R.instance_events(eng.events(), specs)]
    return st, ev


def run_case(case, specs, cap):
    with open_case(case, specs, cap) as eng:
        assert eng.run() == 0
        assert eng.last_kernel() == "step"
        return read(eng, specs, cap)


def oracle_mismatches(case, tag, specs, st, events=None, step_cap=None):
    out = []
    results = W.oracle_results(tag, specs)
    hon = [d for d in range(specs[0]["n"]) if d not in case.byz]
    for i, (exp, dec, delivers) in enumerate(results):
        r = st["inst"][i]
        out += [("oracle", i, k, r[k], exp[k]) for k in W.CKEYS if r[k] != exp[k]]
        if r["deliveries"] != delivers:
            out.append(("oracle", i, "deliveries", r["deliveries"], delivers))
        for d in hon:
            rep, mine = st["reps"][i][d], dec.get(d, [])
            if rep["decide_count"] != len(mine):
                out.append(("oracle", i, d, "decide_count", rep["decide_count"], len(mine)))
            if mine:
                got = (rep["first_decide_round"], rep["first_decide_t"], rep["first_decide_value"])
                if got != mine[0] or rep["last_decide_value"] != mine[-1][2]:
                    out.append(("oracle", i, d, "decisions", got, rep["last_decide_value"], mine[0], mine[-1][2]))
        if bool(r["decided"]) != (case.consensus and all(d in dec for d in hon)):
            out.append(("oracle", i, "decided", r["decided"]))
        if events is not None:
            out += [("oracle", i, k + " events", len(events[i][k]), len(exp["events"][k]))
                    for k in ("deliver", "decide", "send") if events[i][k] != exp["events"][k]]
            if step_cap is not None:
                out += [("event past the cap", i, k, e) for k in ("deliver", "decide", "send") for e in events[i][k] if e[0] > step_cap]
    hist, counts, undecided, dis, stepcap = W.expected_read_side(case, results)
    if st["stats"]["stepcap"] != stepcap:
        out.append(("oracle", "stats.stepcap", st["stats"]["stepcap"], stepcap))
    for k in ("done", "quiescent"):
        want = sum(exp["status"] == k for (exp, _dec, _d) in results)
        if st["stats"][k] != want:
            out.append(("oracle", "stats." + k, st["stats"][k], want))
    if st["stats"]["running"] or st["stats"]["overflow"] or st["stats"]["events_dropped"]:
        out.append(("stats", st["stats"]))
    if case.consensus:
        labels = specs[0]["values"] if len(specs[0]["values"]) == 8 else specs[0]["values"][:4]
        want = {lab: counts.get(v, 0) for v, lab in enumerate(labels)}
        want["undecided"] = undecided
        if st["hist"] != hist:
            out.append(("oracle", "round_histogram", st["hist"], hist))
        if st["dec"] != (want, dis):
            out.append(("oracle", "decisions", st["dec"], (want, dis)))
    return out


def both_builds_equal_oracle(case, tag, specs, step_cap=None):
    """The batch without an event log and with one: each against the oracle, and against each other."""
    plain, _ = run_case(case, specs, 0)
    logged, ev = run_case(case, specs, LOG)
    print(tag, [{k: r[k] for k in W.CKEYS} for r in logged["inst"]])
    a = oracle_mismatches(case, tag, specs, plain, None, step_cap)
    b = oracle_mismatches(case, tag, specs, logged, ev, step_cap)
    c = state_mismatches(plain, logged, "EV = false vs EV = true")
    assert not a and not b and not c, (tag, "no log", a[:8], "log", b[:8], "builds", c[:8])
    return plain, logged, ev


# ---- capped runs ---------------------------------------------------------------------------------------------------
CAPPED = [(c.name, lab) for c in STEP for lab in CAP_LABELS if lab != "gap" or c.gap]


@pytest.mark.parametrize("name,lab", CAPPED, ids=["%s-%s" % p for p in CAPPED])
def test_capped_run_equals_oracle(name, lab):
    case = W.by_name()[name]
    caps, ref, t_last = W.caps(case)
    cap = caps[lab]
    specs = W.capped_specs(case, cap)
    plain, _logged, _ev = both_builds_equal_oracle(case, (name, lab), specs, step_cap=cap)
    want = W.oracle_results((name, lab), specs)[ref][0]["status"]
    assert plain["inst"][ref]["status"] == want and (want == "stepcap") == (lab != "last"), (name, lab, want)


# ---- mixed items on the packed kernels -------------------------------------------------------------------------------
@pytest.mark.parametrize("m", W.mixed(), ids=lambda m: m.name)
def test_mixed_item_under_one_cap(m):
    """Instances of ONE wave item that end differently under one cap (time_axis_workloads.mixed): the STEPCAP exit
    stamps only the segments the oracle stops by the cap.  p16-bound: a segment whose quiet bound could exceed its
    last real arrival, beside a sibling that carries the item past the cap."""
    plain, _logged, _ev = both_builds_equal_oracle(m, (m.name, "mixed"), m.specs, step_cap=m.cap)
    assert {i: r["status"] for i, r in enumerate(plain["inst"])} == m.want


# ---- sliced runs, refusals, reset --------------------------------------------------------------------------------------
SLICED = [(n, lab, k) for n in W.SLICED for lab in ("mid", "gap", "last-1") for k in (1, 3)]


@pytest.mark.parametrize("name,lab,k", SLICED, ids=["%s-%s-run%d" % p for p in SLICED])
def test_sliced_capped_run_equals_oneshot(name, lab, k):
    """run(k) until nothing is running (k = 1: a slice boundary falls on every step, the cap included) equals the
    one-shot run in every field; a further brc_run changes nothing; brc_inject with t > step_cap is BRC_E_INVALID,
    into a STEPCAP instance BRC_E_STATE, and both leave every output as it was."""
    L = _L()
    case = W.by_name()[name]
    cap = W.caps(case)[0][lab]
    specs = W.capped_specs(case, cap)
    whole, whole_ev = run_case(case, specs, LOG)
    allm = (1 << specs[0]["n"]) - 1
    with open_case(case, specs, LOG) as eng:
        slices = 1
        while eng.run(k):
            slices += 1
            assert slices <= cap + 3, "more slices than steps"
        got, got_ev = read(eng, specs, LOG)
        assert slices >= 2                         # brc_run calls: the run did not fit one slice
        assert eng.run() == 0 and eng.run(1) == 0
        again, again_ev = read(eng, specs, LOG)
        hit = [i for i, r in enumerate(got["inst"]) if r["status"] == "stepcap"]
        assert hit
        with pytest.raises(L.EngineError) as err:
            eng.inject([dict(t=cap + 1, kind=L.INJ_SEND, instance=hit[0], node=1, kp=1, s=1, value=0, dst=allm)])
        assert err.value.code == L.E_INVALID
        open_ = [i for i, r in enumerate(got["inst"]) if r["status"] == "quiescent"]
        if open_:                                  # ... also into an instance that would take an injection
            with pytest.raises(L.EngineError) as err:
                eng.inject([dict(t=cap + 1, kind=L.INJ_SEND, instance=open_[0], node=1, kp=1, s=1, value=0, dst=allm)])
            assert err.value.code == L.E_INVALID
        for i in hit:
            with pytest.raises(L.EngineError) as err:
                eng.inject([dict(t=cap, kind=L.INJ_SEND, instance=i, node=1, kp=1, s=1, value=0, dst=allm)])
            assert err.value.code == L.E_STATE
        assert eng.run() == 0
        after, after_ev = read(eng, specs, LOG)
    a = state_mismatches(whole, got, "one-shot vs run(%d)" % k)
    b = state_mismatches(got, again, "before vs after a further brc_run")
    c = state_mismatches(got, after, "before vs after the refused injections")
    assert not a and not b and not c, (a[:8], b[:8], c[:8])
    assert whole_ev == got_ev == again_ev == after_ev
    assert not oracle_mismatches(case, (name, lab), specs, got, got_ev, cap)


@pytest.mark.parametrize("name", W.SLICED)
def test_reset_after_capped_run_equals_fresh_engine(name):
    case = W.by_name()[name]
    R, F = _runner()
    caps = W.caps(case)[0]
    specs = W.capped_specs(case, caps["mid"])
    moved = [dict(sp, g=sp["g"] + case.count) for sp in specs]
    inj = F.injections
    fresh_a, _ = run_case(case, specs, 0)
    fresh_b, _ = run_case(case, moved, 0)
    with open_case(case, specs) as eng:
        assert eng.run() == 0
        first, _ = read(eng, specs, 0)
        eng.reset()
        eng.inject(inj(specs))
        assert eng.run() == 0
        second, _ = read(eng, specs, 0)
        eng.reset_at(W.OFFSET + case.count)
        eng.inject(inj(moved))
        assert eng.run() == 0
        third, _ = read(eng, moved, 0)
    assert first["stats"]["stepcap"] > 0
    assert not state_mismatches(fresh_a, first, "fresh vs first")
    assert not state_mismatches(fresh_a, second, "fresh vs after reset()")
    assert not state_mismatches(fresh_b, third, "fresh at the new offset vs after reset_at()")
    if specs[0]["delay_model"] != W.CONST:          # (one constant delay: the schedule does not depend on the id)
        assert state_mismatches(second, third, "A vs B"), "the two id ranges give one result: nothing is shown"
    assert not oracle_mismatches(case, (name, "mid-moved"), moved, third)


# ---- the key-lifetime kernel -------------------------------------------------------------------------------------------
LIFE = [(c.name, lab) for c in W.cases() if c.life for lab in CAP_LABELS if lab != "gap" or c.gap]


@pytest.mark.parametrize("name,lab", LIFE, ids=["%s-%s" % p for p in LIFE])
def test_lifetime_kernel_capped_equals_step_kernel_and_oracle(name, lab):
    R, _F = _runner()
    case = W.by_name()[name]
    cap = W.caps(case)[0][lab]
    specs = W.capped_specs(case, cap)
    life = R.run_batch_noevents(specs, proposals="philox", key_window=case.key_window, kernel="life")
    step = R.run_batch_noevents(specs, proposals="philox", key_window=case.key_window, kernel="step")
    print(name, lab, cap, [{k: r[k] for k in W.CKEYS} for r in life["inst"]])
    a = oracle_mismatches(case, (name, lab), specs, life)
    b = oracle_mismatches(case, (name, lab), specs, step)
    # (t_now, lane_loads and max_t describe the kernel's own stepping: the lifetime kernel has no item step)
    c = [x for x in state_mismatches(step, life, "step vs life") if x[3] != "t_now" and x[2] not in ("lane_loads", "max_t")]
    assert not a and not b and not c, (name, lab, "life", a[:8], "step", b[:8], "step vs life", c[:8])


# ---- late runs -------------------------------------------------------------------------------------------------------------
def _late_params():
    out = []
    for c in STEP:
        labs = ["shift-" + k for k in W.late_t0s_labels(c)] + (["bursts-" + k for k in W.late_t0s_labels(c)] if c.brb else []) + ["cut"]
        out += [(c.name, lab) for lab in labs]
    return out


LATE = _late_params()


@pytest.mark.parametrize("name,lab", LATE, ids=["%s-%s" % p for p in LATE])
def test_late_run_equals_oracle(name, lab):
    case = W.by_name()[name]
    specs, _keys = W.late_specs(case)[lab]
    plain, _logged, ev = both_builds_equal_oracle(case, (name, lab), specs, step_cap=W.STEP_LIMIT)
    if lab == "cut":
        assert plain["stats"]["stepcap"] > 0
    else:
        assert max(r["t_stop"] for r in plain["inst"]) > W.late_t0s(case)[lab.split("-", 1)[1]]
        assert all(e[0] >= min(a["t"] for a in sp["actions"]) for sp, per in zip(specs, ev) for k in per for e in per[k])


LATE_POL = [(n, pol) for n in W.LATE_INTERLEAVED for pol in ("look1", "at_now")]


@pytest.mark.parametrize("name,pol", LATE_POL, ids=["%s-%s" % p for p in LATE_POL])
def test_late_run_fed_in_pieces_equals_oneshot(name, pol):
    """The shifted run under lookahead(1) and under at_now (the actions of one early step stay on the host until the
    instance stands at that step, 59,900 steps in, and go in with t == t_now): both equal the one-shot run."""
    R, F = _runner()
    case = W.by_name()[name]
    specs, _keys = W.late_specs(case)["shift-59900"]
    whole, whole_ev = run_case(case, specs, LOG)
    marks = W.at_now_marks(case, W.T0)
    policy = R.lookahead(1) if pol == "look1" else R.at_now(marks)
    trace = {}
    if case.flagged:
        got, got_ev = F.run_flagged_interleaved(specs, policy, event_capacity=LOG, key_window=case.key_window, trace=trace)
    else:
        got, got_ev = R.run_batch_interleaved(specs, policy, event_capacity=LOG, key_window=case.key_window, trace=trace)
    assert trace["slices"] >= 4 and trace["unconsumed"] == 0, trace
    if pol == "at_now":
        assert sorted(trace["at_now"]) == sorted((i, t) for i, ts in marks.items() for t in ts) and marks, (trace["at_now"], marks)
    a = state_mismatches(whole, got, "one-shot vs " + pol)
    a += [("events", i) for i, (x, y) in enumerate(zip(whole_ev, got_ev)) if x != y]
    b = oracle_mismatches(case, (name, "shift-59900"), specs, got, got_ev, W.STEP_LIMIT)
    assert not a and not b, (name, pol, a[:8], b[:8])
