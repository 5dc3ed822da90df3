"""GPU: a second SEND of one key (include/brc.h, "Extra SENDs") on the wide step kernels (n > 64) of an engine
created with BRC_FLAG_WIDE_RECORDS, against the reference fixture tests/golden/wide_xsend/ and the C oracle.
tests/wide_xsend_workloads.py has one batch of three instances per shape; tests/test_wide_xsend_workloads.py proves
their preconditions on the oracle.  Before the feature brc_inject refused every second SEND of a key above 64 replicas
(BRC_E_UNSUPPORTED) and network.Cluster.brb_send raised EngineError for it."""
import pytest

from tests import golden_io
from tests import wide_xsend_workloads as W
from tests.golden import specs as S
from tests.test_gpu_interleaved import oracle_mismatches
from tests.test_gpu_step_noevent import state_mismatches
from tests.test_wide_xsend_workloads import FIX, wire_messages

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in W.cases()]
LOG = 1 << 20


def _runner():
    from tests import engine_runner, wide_records_runner
    return engine_runner, wide_records_runner


def _L():
    from byzantinerandomizedconsensus_amd import _lib
    return _lib


def _injections(case, specs=None):
    """The batch's injections; in the GARBAGE cases every SEND and ECHO / READY with random bits at and above n."""
    R, F = _runner()
    L = _L()
    specs = case.specs if specs is None else specs
    out = F.injections(specs)
    if case.name in W.GARBAGE:
        n = specs[0]["n"]
        out = [dict(x, dst=x["dst"] | W.garbage(n, j)) if x["kind"] in (L.INJ_SEND, L.INJ_MSG) else x for j, x in enumerate(out)]
        assert any(x.get("dst", 0) >> n for x in out)
    return out


def _run(case, cap, specs=None):
    R, F = _runner()
    specs = case.specs if specs is None else specs
    with F.open_flagged(specs, cap, inject=False, **case.open_kw()) as eng:
        eng.inject(_injections(case, specs))
        eng.run()
        assert eng.last_kernel() == "step"
        st = R.read_state(eng, specs)
        ev = None if not cap else [R.sort_result({"events": e})["events"] for e in R.instance_events(eng.events(), specs)]
    return st, ev


def test_fixture_runs_equal_the_reference():
    R, F = _runner()
    for c in FIX:
        sp = c["spec"]
        st, ev = F.run_flagged([sp], event_capacity=LOG)
        golden_io.assert_matches(c["result"], dict(st["inst"][0], events=ev[0]), sp["name"])
        assert st["inst"][0]["cell_steps"] == c["cell_steps"], sp["name"]


@pytest.mark.parametrize("cap", (0, LOG), ids=("nolog", "log"))
@pytest.mark.parametrize("name", NAMES)
def test_workload_equals_oracle(name, cap):
    case = W.by_name()[name]
    st, ev = _run(case, cap)
    print(name, cap, [{k: r[k] for k in W.CKEYS} for r in st["inst"]])
    assert st["stats"]["running"] == 0 and st["stats"]["events_dropped"] == 0
    diff = oracle_mismatches(case, st, ev)
    assert not diff, (name, diff[:8])


@pytest.mark.parametrize("pol", ("look1", "at_now"))
@pytest.mark.parametrize("name", W.INTERLEAVED)
def test_interleaved_equals_oneshot_and_oracle(name, pol):
    """The extra SEND of the marked instance goes in with t == t_now (at_now): the re-entered step lands nothing twice."""
    R, F = _runner()
    case = W.by_name()[name]
    whole, whole_ev = F.run_flagged(case.specs, event_capacity=LOG, **case.open_kw())
    trace = {}
    got, got_ev = F.run_flagged_interleaved(case.specs, case.policies()[pol], event_capacity=LOG, trace=trace, **case.open_kw())
    if pol == "at_now":
        assert sorted(trace["at_now"]) == sorted((i, t) for i, ts in case.marks.items() for t in ts), (trace["at_now"], case.marks)
        for i, ts in case.marks.items():
            assert any(a["t"] in ts for a in W.extra_sends(case.specs[i]))
    vs_whole = state_mismatches(whole, got, "one-shot vs " + pol)
    vs_whole += [("events", i) for i, (a, b) in enumerate(zip(whole_ev, got_ev)) if a != b]
    vs_oracle = oracle_mismatches(case, got, got_ev)
    assert not vs_whole and not vs_oracle, (name, pol, vs_whole[:8], vs_oracle[:8])


@pytest.mark.parametrize("name", ("xw-128-ref-unif", "xw-256-ref-brb"))
def test_reset_with_records_in_flight(name):
    """run(2) leaves records in flight (extra SENDs at steps 0 .. 3, arrivals up to D later): reset() and the same
    batch again equals a fresh engine; reset_at and the re-keyed batch equals a fresh engine at that offset."""
    R, F = _runner()
    case = W.by_name()[name]
    moved = [dict(sp, g=sp["g"] + W.COUNT) for sp in case.specs]
    fresh_a, _ = F.run_flagged(case.specs, **case.open_kw())
    fresh_b, _ = F.run_flagged(moved, **case.open_kw())
    with F.open_flagged(case.specs, **case.open_kw()) as eng:
        assert eng.run(2) > 0
        assert any(1 <= r["t_now"] <= 3 for r in eng.instances_result())
        eng.reset()
        eng.inject(F.injections(case.specs))
        eng.run()
        second = R.read_state(eng, case.specs)
        eng.reset()
        eng.inject(F.injections(case.specs))
        eng.run(2)
        eng.reset_at(W.OFFSET + W.COUNT)
        eng.inject(F.injections(moved))
        eng.run()
        third = R.read_state(eng, moved)
    assert not state_mismatches(fresh_a, second, "fresh vs after reset()")
    assert not state_mismatches(fresh_b, third, "fresh at the new offset vs after reset_at()")
    assert state_mismatches(second, third, "A vs B"), "the two id ranges give one result: nothing is shown"


def _valid_run_equals_oracle(eng, sp, local=0, count=1):
    R, F = _runner()
    eng.inject(R._injections(sp, local))
    eng.run()
    r = eng.instances_result()[local]
    exp, _dec, delivers = W.I.oracle_run(sp)
    diff = [(k, r[k], exp[k]) for k in W.CKEYS if r[k] != exp[k]]
    assert not diff and r["deliveries"] == delivers, (sp["name"], diff)


def _plain(n, f, seed, byz, g=W.OFFSET, **kw):
    return dict(S.brb_spec(n, f, seed, W.UNIF, 3, g, [(0, 0, 0)], byzantine=byz, **kw), step_cap=W.I.STEP_CAP)


@pytest.mark.parametrize("what", ("declared", "absent"))
def test_extra_send_of_a_key_not_sent_stops_that_instance_only(what):
    """brc_inject marks a SEND as extra by the SENDs it has seen, whatever their times: here the first SEND it saw is
    stamped later than the second, so the extra SEND finds the key declared but not SENT (or absent) at its step:
    BRC_BADINJ for that instance; its neighbour in the batch runs to the oracle's result."""
    R, F = _runner()
    L = _L()
    specs = [dict(_plain(70, 23, 0x2E5900E0, W.BYZ70, g=W.OFFSET + i), name="badinj-wide/%d" % i) for i in range(2)]
    late = dict(t=9, kind=L.INJ_SEND, instance=0, node=69, kp=69, s=0, value=0, dst=(1 << 70) - 1)
    early = dict(t=2, kind=L.INJ_SEND, instance=0, node=66, kp=69, s=0, value=0, dst=0b1011 | 1 << 65)
    key = [dict(t=1, kind=L.INJ_KEY, instance=0, node=69, kp=69, s=0, value=0)] if what == "declared" else []
    with F.open_flagged(specs, inject=False) as eng:
        eng.inject(R._injections(specs[0], 0) + key + [late, early])
        _valid_run_equals_oracle(eng, specs[1], local=1)
        res = eng.instances_result()
    assert res[0]["status"] == "bad_injection" and res[0]["t_now"] == 2, res[0]
    assert res[1]["status"] == "quiescent"


def test_table_overflow_is_refused_at_once():
    """A 17th record in flight in one instance: BRC_E_UNSUPPORTED, nothing changed (the valid records ahead of it in
    the batch are not kept) -- the 16 before it run and equal the oracle on the same engine."""
    R, F = _runner()
    L = _L()
    sp = W.overflow_spec()
    ok = dict(sp, actions=sp["actions"][:-1])
    with F.open_flagged([sp], inject=False) as eng:
        with pytest.raises(L.EngineError) as err:
            eng.inject(R._injections(sp, 0))
        assert err.value.code == L.E_UNSUPPORTED and "records in flight" in str(err.value), str(err.value)
        _valid_run_equals_oracle(eng, ok)


def test_flagless_wide_engine_refuses_as_before():
    R, F = _runner()
    L = _L()
    sp = dict(_plain(100, 33, 0x2E5900E3, [98, 99]), name="refused-flagless-xsend")
    bad = dict(t=1, kind=L.INJ_SEND, instance=0, node=70, kp=0, s=0, value=0, dst=(1 << 100) - 1)
    with F.open_flagged([sp], inject=False, wide_records=False) as eng:
        with pytest.raises(L.EngineError) as err:
            eng.inject(R._injections(sp, 0) + [bad])         # the valid SEND ahead of it is not kept either
        assert err.value.code == L.E_UNSUPPORTED and "a key can be SENT only once on this kernel" in str(err.value)
        _valid_run_equals_oracle(eng, sp)


def test_repeat_with_no_link_left_changes_nothing():
    """The origin SENDs its key to everyone again (sender peers: no link left): accepted, not staged -- every counter
    equals the run without it; a stopped instance still refuses it."""
    R, F = _runner()
    L = _L()
    sp = dict(_plain(70, 23, 0x2E5900E4, W.BYZ70), name="noop-repeat-wide")
    again = dict(t=1, kind=L.INJ_SEND, instance=0, node=0, kp=0, s=0, value=0, dst=(1 << 70) - 1)
    sub = dict(again, t=2, dst=0b1101 | 1 << 64)
    with F.open_flagged([sp], event_capacity=LOG, inject=False) as eng:
        eng.inject(R._injections(sp, 0) + [again, sub])
        eng.run()
        res = eng.instances_result()[0]
        evs = R.instance_events(eng.events(), [sp])[0]
    exp, _dec, delivers = W.I.oracle_run(sp)
    assert not [(k, res[k], exp[k]) for k in W.CKEYS if res[k] != exp[k]] and res["deliveries"] == delivers
    assert R.sort_result({"events": evs})["events"] == exp["events"]
    stopped = dict(sp, step_cap=1)
    with F.open_flagged([stopped], inject=False) as eng:
        eng.inject(R._injections(stopped, 0))
        eng.run()
        assert eng.instances_result()[0]["status"] == "stepcap"
        with pytest.raises(L.EngineError) as err:
            eng.inject([again])
        assert err.value.code == L.E_STATE


def test_class_api_runs_the_fixture():
    """The fixture's specs through the reference's class API: 70 sender-peer BRBroadcast nodes (replica 68, the
    Byzantine one, is a peer without a node; its SEND to a subset is handed to the cluster as the raw message it is).
    The deliver upcalls are the reference's, at its steps and in its order."""
    from byzantinerandomizedconsensus_amd import network
    from byzantinerandomizedconsensus_amd.base.broadcast import IBroadcastHandler
    from byzantinerandomizedconsensus_amd.core.brbroadcast import BRBroadcast
    L = _L()
    saved = network.settings()
    try:
        for case in FIX:
            sp = case["spec"]
            network.reset()
            network.configure(delay_model=sp["delay_model"], delay_max=sp["dmax"], seed=sp["seed"], instance_id=sp["g"],
                              peer_mode="sender", step_cap=sp["step_cap"])
            got = []

            class H(IBroadcastHandler):
                def __init__(self, i):
                    self.i = i

                def deliver(self, message):
                    got.append([cluster.t, self.i, message])

            peers = [("localhost", 7300 + i) for i in range(sp["n"])]
            nodes = {i: BRBroadcast(sp["n"], sp["f"], p, peers, H(i)) for i, p in enumerate(peers) if i not in sp["byzantine"]}
            cluster = nodes[0].cluster
            todo = sorted(sp["actions"], key=lambda a: a["t"])
            while todo:
                assert todo[0]["t"] >= cluster.t, (sp["name"], todo[0], cluster.t)
                while todo and todo[0]["t"] == cluster.t:
                    a = todo.pop(0)
                    if a["kind"] == "brb_send":
                        nodes[a["node"]].broadcast(BRBroadcast.SEND, a["payload"])
                    else:
                        assert a["kind"] == "byz" and a["type"] == S.SEND and a["src"] in sp["byzantine"]
                        cluster.actions.append(dict(t=cluster.t, kind=L.INJ_SEND, node=a["src"], kp=a["kp"], s=a["s"], value=0,
                                                    dst=a["dst"]))
                cluster.run(max_steps=1)
            assert cluster.engine.cfg.flags & L.FLAG_WIDE_RECORDS
            status = cluster.run()
            assert status == case["result"]["status"], sp["name"]
            exp = [[t, node, "TEST %d.%d" % (kp + 1, s)] for (t, node, kp, s) in case["result"]["raw_order"]["deliver"]]
            assert got == exp, sp["name"]
    finally:
        network.reset()
        network.configure(**saved)


def test_replayed_wire_capture_reproduces_the_fixture():
    """wire.Codec.to_injections over the captured SENDs: two and more INJ_SEND records of one key, one of them to a
    subset with destinations in both words, reproduce the fixture run."""
    from tests.test_wire import codec_for
    R, F = _runner()
    L = _L()
    for c in FIX:
        sp = c["spec"]
        replay = codec_for(sp).to_injections(wire_messages(c))
        sends = [x for x in replay if x["kind"] == L.INJ_SEND]
        assert len(sends) == 5 and len({(x["kp"], x["s"]) for x in sends}) == 2
        assert any(x["dst"] >> 64 and x["dst"] & ((1 << 64) - 1) and x["dst"] != (1 << sp["n"]) - 1 for x in sends)
        with F.open_flagged([sp], event_capacity=LOG, inject=False) as eng:
            eng.inject(replay)
            eng.run()
            res = eng.instances_result()[0]
            evs = R.instance_events(eng.events(), [sp])[0]
        golden_io.assert_matches(c["result"], dict(res, events=evs), sp["name"])
        assert res["cell_steps"] == c["cell_steps"]
