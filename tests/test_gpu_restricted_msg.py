"""GPU: a Byzantine replica's ECHO / READY to a subset of the peers (include/brc.h, "Restricted ECHO / READY") on
the non-lean narrow step kernels, against the reference fixture tests/golden/restricted_msg/ and the C oracle.
tests/restricted_msg_workloads.py has one small batch per kernel family and mode;
tests/test_restricted_msg_workloads.py proves their preconditions on the oracle.  Before the feature brc_inject
refused every such record with BRC_E_UNSUPPORTED."""
import pytest

from tests import golden_io
from tests import restricted_msg_workloads as W
from tests.golden import specs as S
from tests.test_gpu_interleaved import oracle_mismatches
from tests.test_gpu_step_noevent import state_mismatches
from tests.test_restricted_msg_workloads import FIX

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in W.cases()]
LOG = 1 << 20


def _runner():
    from tests import engine_runner
    return engine_runner


def _L():
    from byzantinerandomizedconsensus_amd import _lib
    return _lib


def test_fixture_runs_equal_the_reference():
    R = _runner()
    got = R.run_specs([c["spec"] for c in FIX])
    for c, r in zip(FIX, got):
        golden_io.assert_matches(c["result"], r, c["spec"]["name"])
        assert r["cell_steps"] == c["cell_steps"], c["spec"]["name"]


@pytest.mark.parametrize("cap", (0, LOG), ids=("nolog", "log"))
@pytest.mark.parametrize("name", NAMES)
def test_workload_equals_oracle(name, cap):
    R = _runner()
    case = W.by_name()[name]
    if cap:
        st, ev = R.run_batch_noevents(case.specs, event_capacity=cap, with_events=True, **case.open_kw())
    else:
        st, ev = R.run_batch_noevents(case.specs, **case.open_kw()), None
    assert st["stats"]["running"] == 0 and st["stats"]["events_dropped"] == 0
    diff = oracle_mismatches(case, st, ev)
    assert not diff, (name, diff[:8])


@pytest.mark.parametrize("pol", ("look1", "at_now"))
@pytest.mark.parametrize("name", W.INTERLEAVED)
def test_interleaved_equals_oneshot_and_oracle(name, pol):
    """The restricted records of the marked instances go in with t == t_now (at_now): the re-entered step lands
    nothing twice."""
    R = _runner()
    case = W.by_name()[name]
    whole, whole_ev = R.run_batch_noevents(case.specs, event_capacity=LOG, with_events=True, **case.open_kw())
    trace = {}
    got, got_ev = R.run_batch_interleaved(case.specs, case.policies()[pol], event_capacity=LOG, trace=trace, **case.open_kw())
    if pol == "at_now":
        assert sorted(trace["at_now"]) == sorted((i, t) for i, ts in case.marks.items() for t in ts), (trace["at_now"], case.marks)
        for i, ts in case.marks.items():
            assert any(W.is_restricted(case.specs[i], a) and a["t"] in ts for a in case.specs[i]["actions"])
    vs_whole = state_mismatches(whole, got, "one-shot vs " + pol)
    vs_whole += [("events", i) for i, (a, b) in enumerate(zip(whole_ev, got_ev)) if a != b]
    vs_oracle = oracle_mismatches(case, got, got_ev)
    assert not vs_whole and not vs_oracle, (name, pol, vs_whole[:8], vs_oracle[:8])


@pytest.mark.parametrize("name", ("rm-p16-ref-brb", "rm-n64-xref-brb"))
def test_reset_with_records_in_flight(name):
    """run(2) leaves records in flight (injected at steps 1 .. 3, arrivals up to D later): reset() and the same batch
    again equals a fresh engine; reset_at and the re-keyed batch equals a fresh engine at that offset."""
    R = _runner()
    case = W.by_name()[name]
    moved = [dict(sp, g=sp["g"] + case.count) for sp in case.specs]
    fresh_a = R.run_batch_noevents(case.specs, **case.open_kw())
    fresh_b = R.run_batch_noevents(moved, **case.open_kw())
    with R.open_batch(case.specs, **case.open_kw()) as eng:
        assert eng.run(2) > 0
        assert any(1 <= r["t_now"] <= 3 for r in eng.instances_result())
        eng.reset()
        for i, sp in enumerate(case.specs):
            eng.inject(R._injections(sp, i))
        eng.run()
        second = R.read_state(eng, case.specs)
        eng.reset()
        for i, sp in enumerate(case.specs):
            eng.inject(R._injections(sp, i))
        eng.run(2)
        eng.reset_at(W.OFFSET + case.count)
        for i, sp in enumerate(moved):
            eng.inject(R._injections(sp, i))
        eng.run()
        third = R.read_state(eng, moved)
    assert not state_mismatches(fresh_a, second, "fresh vs after reset()")
    assert not state_mismatches(fresh_b, third, "fresh at the new offset vs after reset_at()")
    assert state_mismatches(second, third, "A vs B"), "the two id ranges give one result: nothing is shown"


def _valid_run_equals_oracle(eng, sp):
    R = _runner()
    eng.inject(R._injections(sp, 0))
    eng.run()
    st = R.read_state(eng, [sp])
    exp, _dec, delivers = W.I.oracle_run(sp)
    r = st["inst"][0]
    diff = [(k, r[k], exp[k]) for k in W.CKEYS if r[k] != exp[k]]
    assert not diff and r["deliveries"] == delivers, (sp["name"], diff)


def _refused(eng, rec, word):
    L = _L()
    with pytest.raises(L.EngineError) as err:
        eng.inject([rec])
    assert err.value.code == L.E_UNSUPPORTED
    assert word in str(err.value), str(err.value)


REFUSALS = {
    # family word in the error text, spec of the valid run that follows, the refused record's node
    "honest": ("Byzantine sender", lambda: S.brb_spec(7, 2, 0x2E5700E0, W.UNIF, 3, W.OFFSET, [(0, 0, 0)], byzantine=[5, 6]), 2),
    "lean": ("lean", lambda: S.brb_spec(40, 13, 0x2E5700E1, W.UNIF, 3, W.OFFSET, [(0, 0, 0)], byzantine=[38, 39]), 39),
    "wide": ("wide", lambda: S.brb_spec(100, 33, 0x2E5700E2, W.UNIF, 3, W.OFFSET, [(0, 0, 0)], byzantine=[98, 99]), 99),
    "connection": ("connection", lambda: S.brb_spec(7, 2, 0x2E5700E3, W.UNIF, 3, W.OFFSET, [(0, 0, 0)], byzantine=[5, 6],
                                                  peer_mode="connection"), 6),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals_leave_no_trace(what):
    """A restricted ECHO from an honest sender, on the lean kernel (n = 40 without the flag), on the wide kernel
    (n = 100) and with connection peers: BRC_E_UNSUPPORTED, the kernel family named; the valid run that follows on
    the same engine equals the oracle."""
    R, L = _runner(), _L()
    word, make, node = REFUSALS[what]
    sp = dict(make(), name="refused-" + what, step_cap=W.I.STEP_CAP)
    valid = dict(t=0, kind=L.INJ_SEND, instance=0, node=1, kp=1, s=0, value=0, dst=(1 << sp["n"]) - 1)
    bad = dict(t=1, kind=L.INJ_MSG, type=L.ECHO, instance=0, node=node, kp=0, s=0, value=0, dst=0b101)
    with R.open_batch([dict(sp, actions=[])]) as eng:
        with pytest.raises(L.EngineError) as err:
            eng.inject([valid, bad])             # the valid record ahead of it is not kept either
        assert err.value.code == L.E_UNSUPPORTED and word in str(err.value), str(err.value)
        _valid_run_equals_oracle(eng, sp)


def test_table_overflow_is_refused_at_once():
    R, L = _runner(), _L()
    sp = W.overflow_spec()
    ok = dict(sp, actions=sp["actions"][:-1])
    with R.open_batch([dict(sp, actions=[])], key_window=sp["key_window"]) as eng:
        with pytest.raises(L.EngineError) as err:
            eng.inject(R._injections(sp, 0))
        assert err.value.code == L.E_UNSUPPORTED and "records in flight" in str(err.value), str(err.value)
        _valid_run_equals_oracle(eng, ok)


def test_replayed_wire_capture_reproduces_the_fixture():
    """wire.Codec.to_injections over the Byzantine replicas' captured messages: restricted INJ_MSG records that
    reproduce the fixture run."""
    from tests.test_wire import codec_for
    R, L = _runner(), _L()
    for c in FIX:
        sp = c["spec"]
        byz = set(sp["byzantine"])
        honest = [x for x in R._injections(sp, 0) if x["kind"] in (L.INJ_PROPOSE,) or x["node"] not in byz]
        replay = codec_for(sp).to_injections(c["wire_byz"])
        assert any(x["kind"] == L.INJ_MSG and x["dst"] != (1 << sp["n"]) - 1 for x in replay)
        with R.open_batch([dict(sp, actions=[])], event_capacity=LOG) as eng:
            eng.inject(honest + replay)
            eng.run()
            res = eng.instances_result()[0]
            evs = R.instance_events(eng.events(), [sp])[0]
        golden_io.assert_matches(c["result"], dict(res, events=evs), sp["name"])
        assert res["cell_steps"] == c["cell_steps"]
