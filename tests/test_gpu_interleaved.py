"""Actions injected BETWEEN sliced brc_run calls, on every kernel family, against the same build's one-shot run
and the C oracle.  Every other parity test injects a batch's whole action list before the first brc_run; the path
network.Cluster.run takes -- an action that arrives after the engine has advanced -- runs through upload_injections'
consumed-prefix erase and re-sort, brc_inject's t == t_now acceptance (the kernels re-enter step t), the host's
re-opening of QUIESCENT instances, the extra-SEND table's pruning, and the kernels' record window seeing the list in
pieces.  tests/interleaved_workloads.py has one small batch per family; tests/test_interleaved_workloads.py proves
its preconditions on the oracle.  tests/engine_runner.drive_interleaved feeds each batch under lookahead(1),
lookahead(3), at_now and after_quiet, without an event log and with one (drained with events_since per slice).

Per case, policy and log setting, bit-exact: (a) every instances_result() field, replicas() record, stats() field,
round_histogram(66) and decisions() equals the one-shot run (everything injected, then run()) -- nothing excluded;
(b) every instance equals the oracle: status, t_stop, msgs_sent, arrivals, cell_steps, deliveries, decided, every
honest replica's decisions, the sorted DELIVER / DECIDE / SEND lists, round_histogram and decisions.
"""
import pytest

from tests import interleaved_workloads as W
from tests.test_gpu_step_noevent import state_mismatches

pytestmark = pytest.mark.gpu

CASES = W.cases()
LOG = 1 << 20
_ONESHOT = {}


def _runner():
    from tests import engine_runner
    return engine_runner


def _L():
    from byzantinerandomizedconsensus_amd import _lib
    return _lib


def oneshot(case, cap):
    """The same build with everything injected first, then run(): once per case and log setting."""
    if (case.name, cap) not in _ONESHOT:
        R = _runner()
        if cap:
            _ONESHOT[(case.name, cap)] = R.run_batch_noevents(case.specs, event_capacity=cap, with_events=True, **case.open_kw())
        else:
            _ONESHOT[(case.name, cap)] = (R.run_batch_noevents(case.specs, **case.open_kw()), None)
    return _ONESHOT[(case.name, cap)]


def oracle_mismatches(case, st, events=None):
    out = []
    hon = [d for d in range(case.specs[0]["n"]) if d not in case.byz]
    for i, (exp, dec, delivers) in W.oracle_results(case).items():
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
    if case.consensus:
        hist, counts, undecided, dis = W.expected_read_side(case)
        want = {lab: counts.get(v, 0) for v, lab in enumerate(case.specs[0]["values"][:4])}
        want["undecided"] = undecided
        if st["hist"] != hist:
            out.append(("oracle", "round_histogram", st["hist"], hist))
        if st["dec"] != (want, dis):
            out.append(("oracle", "decisions", st["dec"], (want, dis)))
    return out


PARAMS = [(c.name, pol, cap) for c in CASES for pol in c.policies() for cap in (0, LOG)]


@pytest.mark.parametrize("name,pol,cap", PARAMS, ids=["%s-%s-%s" % (n, p, "log" if c else "nolog") for n, p, c in PARAMS])
def test_interleaved_equals_oneshot_and_oracle(name, pol, cap):
    R = _runner()
    case = W.by_name()[name]
    whole, whole_ev = oneshot(case, cap)
    trace = {}
    got, got_ev = R.run_batch_interleaved(case.specs, case.policies()[pol], event_capacity=cap, trace=trace, **case.open_kw())
    print(name, pol, cap, case.inst, {k: trace[k] for k in ("slices", "pieces", "at_now", "reopened", "unconsumed")},
          {k: got["stats"][k] for k in ("done", "quiescent", "max_t", "cell_steps", "lane_loads")})
    assert got["stats"]["running"] == 0 and got["stats"]["events_dropped"] == 0 and trace["unconsumed"] == 0, (name, got["stats"])
    # the policy did what it is for
    times = max(len({a["t"] for a in sp["actions"]}) for sp in case.specs)
    assert trace["slices"] >= 2 and (trace["pieces"] >= 2 or pol == "look3" and times <= 4), (name, pol, trace)
    if pol == "at_now":
        assert sorted(trace["at_now"]) == sorted((i, t) for i, ts in case.marks.items() for t in ts), (trace["at_now"], case.marks)
    if pol == "after_quiet":
        assert sorted(i for i, _t in trace["reopened"]) == sorted(i for i, b in case.bounds.items() for _ in b), trace["reopened"]
    vs_whole = state_mismatches(whole, got, "one-shot vs " + pol)
    if cap:
        vs_whole += [("events", i) for i, (a, b) in enumerate(zip(whole_ev, got_ev)) if a != b]
    vs_oracle = oracle_mismatches(case, got, got_ev)
    # a difference places itself: the one-shot run alone matching the oracle is a defect of the interleaved path
    assert not vs_whole and not vs_oracle, (name, pol, vs_whole[:8], vs_oracle[:8], "one-shot vs oracle",
                                            oracle_mismatches(case, whole, whole_ev)[:6])


# ---- extra SENDs pruned while the run goes on ------------------------------------------------------------------
def _oracle_one(sp, st, events):
    exp, _dec, delivers = W.oracle_run(sp)
    r = st["inst"][0]
    out = [(k, r[k], exp[k]) for k in W.CKEYS if r[k] != exp[k]]
    if r["deliveries"] != delivers:
        out.append(("deliveries", r["deliveries"], delivers))
    return out + [(k + " events", len(events[0][k]), len(exp["events"][k])) for k in ("deliver", "decide", "send")
                  if events[0][k] != exp["events"][k]]


def test_pruned_extra_sends():
    """48 extra-SEND records over the run, never more than XSEND_MAX = 16 in flight: fed three action times ahead the
    table is pruned as the item advances and the run equals the oracle; the same list at once is refused
    (BRC_E_UNSUPPORTED) and changes nothing."""
    R, L = _runner(), _L()
    sp = W.pruning_spec()
    got, ev = R.run_batch_interleaved([sp], R.lookahead(3), event_capacity=LOG)
    diff = _oracle_one(sp, got, ev)
    assert not diff, diff
    with R.open_batch([dict(sp, actions=[])]) as eng:
        with pytest.raises(L.EngineError) as err:
            eng.inject(R._injections(sp, 0))
        assert err.value.code == L.E_UNSUPPORTED
        # nothing of the refused batch stayed: the interleaved run on this engine is the run above
        again, _ = R.drive_interleaved(eng, [sp], R.lookahead(3))
    free, _ = R.run_batch_interleaved([sp], R.lookahead(3))
    assert not state_mismatches(free, again, "fresh vs after the refused batch")
    assert not [k for k in W.CKEYS + ("deliveries",) if got["inst"][0][k] != free["inst"][0][k]]


# ---- refusals leave no trace --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["p16-ref-byz", "n64-ref-brb", "w128-ref-brb"])
def test_refused_batches_leave_no_trace(name):
    """Half-way through a run(3) sliced run: a batch with one record before the item's step (BRC_E_STATE), on the
    3-bit-id kernel a batch that overflows the extra-SEND table (BRC_E_UNSUPPORTED); at the end an injection into a
    DONE / STEPCAP instance where there is one.  Each batch carries valid records before the bad one.  The run
    equals the one-shot run, which saw none of them."""
    R, L = _runner(), _L()
    case = W.by_name()[name]
    whole, _ = oneshot(case, 0)
    n = case.specs[0]["n"]
    allm = (1 << n) - 1
    refused = []
    with R.open_batch(case.specs, **case.open_kw()) as eng:
        for _ in range(case.specs[0]["step_cap"]):
            left = eng.run(3)
            res = eng.instances_result()
            i = max(range(case.count), key=lambda j: res[j]["t_now"])
            now = res[i]["t_now"]
            if now >= 5 and res[i]["status"] == "running":
                good = dict(t=now + 1, kind=L.INJ_SEND, instance=i, node=6, kp=6, s=1, value=0, dst=allm)
                with pytest.raises(L.EngineError) as err:
                    eng.inject([good, dict(good, t=now - 1, s=2)])
                assert err.value.code == L.E_STATE
                refused.append("past")
                if case.inst[1] == 16:
                    # 18 first SENDs by other nodes of three keys SENT before (a node's repeat on used links is dropped)
                    many = [dict(t=now + 1 + j, kind=L.INJ_SEND, instance=i, node=o, kp=kp, s=0, value=0, dst=allm)
                            for j, (o, kp) in enumerate((o, kp) for kp in (0, 3, 5) for o in (1, 4, 6, 7, 8, 10))]
                    assert len(many) > W.XSEND_MAX
                    with pytest.raises(L.EngineError) as err:
                        eng.inject([good] + many)
                    assert err.value.code == L.E_UNSUPPORTED
                    refused.append("xsend")
            if left == 0:
                break
        assert "past" in refused and ("xsend" in refused or case.inst[1] != 16), refused
        got = R.read_state(eng, case.specs)
    assert not state_mismatches(whole, got, "one-shot vs sliced with refused batches")


def test_stopped_instances_refuse_injections():
    """DONE (consensus) and STEPCAP instances: BRC_E_STATE, and every output stays as it was."""
    R, L = _runner(), _L()
    case = W.by_name()["p4-ref-cons"]
    capped = [dict(sp, step_cap=12, actions=[a for a in sp["actions"] if a["t"] <= 12]) for sp in case.specs]
    for specs, want in ((case.specs, "done"), (capped, "stepcap")):
        with R.open_batch(specs, **case.open_kw()) as eng:
            eng.run()
            before = R.read_state(eng, specs)
            hit = [i for i, r in enumerate(before["inst"]) if r["status"] == want]
            assert hit, (want, [r["status"] for r in before["inst"]])
            for i in hit:
                with pytest.raises(L.EngineError) as err:
                    eng.inject([dict(t=before["inst"][i]["t_now"], kind=L.INJ_PROPOSE, instance=i, node=0, value=1)])
                assert err.value.code == L.E_STATE
            assert eng.run() == 0
            assert not state_mismatches(before, R.read_state(eng, specs), "before vs after refused injections")


# ---- reset ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["p16-ref-byz", "n64-ref-brb", "n64-xref-brb"])
def test_reset_between_interleaved_runs(name):
    """An interleaved run, reset(), the same run again: equal (send_count, send_dst, the extra-SEND records and the
    pending lists are cleared).  reset_at(offset + count) and the re-keyed specs fed the same way: a fresh engine
    at that offset."""
    R = _runner()
    case = W.by_name()[name]
    pol = case.policies()["at_now"]
    moved = [dict(sp, g=sp["g"] + case.count) for sp in case.specs]
    fresh_b, _ = R.run_batch_interleaved(moved, R.lookahead(1), **case.open_kw())
    with R.open_batch(R._unfed(case.specs), **case.open_kw()) as eng:
        first, _ = R.drive_interleaved(eng, case.specs, pol)
        eng.reset()
        second, _ = R.drive_interleaved(eng, case.specs, pol)
        eng.reset_at(W.OFFSET + case.count)
        third, _ = R.drive_interleaved(eng, moved, R.lookahead(1))
    assert not state_mismatches(oneshot(case, 0)[0], first, "one-shot vs first")
    assert not state_mismatches(first, second, "first vs after reset()")
    assert state_mismatches(first, third, "A vs B"), "the two id ranges give one result: nothing is shown"
    assert not state_mismatches(fresh_b, third, "fresh engine at the new offset vs reset_at")
