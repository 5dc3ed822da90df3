"""GPU: a Byzantine replica's ECHO / READY to a subset of the peers (include/brc.h, "Restricted ECHO / READY") on the
wide step kernels (n > 64) of an engine created with BRC_FLAG_WIDE_RECORDS, against the reference fixture
tests/golden/restricted_msg_wide/ and the C oracle.  tests/restricted_msg_wide_workloads.py has one batch of three
instances per shape; tests/test_restricted_msg_wide_workloads.py proves their preconditions on the oracle.  Before the
feature brc_create refused the flag (BRC_E_INVALID), so every test here that opens a flagged engine failed there."""
import pytest

from tests import golden_io
from tests import restricted_msg_wide_workloads as W
from tests.golden import specs as S
from tests.test_gpu_interleaved import oracle_mismatches
from tests.test_gpu_step_noevent import state_mismatches
from tests.test_restricted_msg_wide_workloads import FIX

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in W.cases()]
LOG = 1 << 20


def _runner():
    from tests import engine_runner, wide_records_runner
    return engine_runner, wide_records_runner


def _L():
    from byzantinerandomizedconsensus_amd import _lib
    return _lib


def _garbage(case):
    n = case.specs[0]["n"]
    return (lambda i, j: W.garbage(n, 16 * i + j)) if case.name in W.GARBAGE else None


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
    R, F = _runner()
    case = W.by_name()[name]
    st, ev = F.run_flagged(case.specs, event_capacity=cap, garbage=_garbage(case), **case.open_kw())
    print(name, cap, [{k: r[k] for k in W.CKEYS} for r in st["inst"]])
    assert st["stats"]["running"] == 0 and st["stats"]["events_dropped"] == 0
    diff = oracle_mismatches(case, st, ev)
    assert not diff, (name, diff[:8])


@pytest.mark.parametrize("pol", ("look1", "at_now"))
@pytest.mark.parametrize("name", W.INTERLEAVED)
def test_interleaved_equals_oneshot_and_oracle(name, pol):
    """The restricted records of the marked instance go in with t == t_now (at_now): the re-entered step lands nothing
    twice."""
    R, F = _runner()
    case = W.by_name()[name]
    whole, whole_ev = F.run_flagged(case.specs, event_capacity=LOG, **case.open_kw())
    trace = {}
    got, got_ev = F.run_flagged_interleaved(case.specs, case.policies()[pol], event_capacity=LOG, trace=trace, **case.open_kw())
    if pol == "at_now":
        assert sorted(trace["at_now"]) == sorted((i, t) for i, ts in case.marks.items() for t in ts), (trace["at_now"], case.marks)
        for i, ts in case.marks.items():
            assert any(W.is_restricted(case.specs[i], a) and a["t"] in ts for a in case.specs[i]["actions"])
    vs_whole = state_mismatches(whole, got, "one-shot vs " + pol)
    vs_whole += [("events", i) for i, (a, b) in enumerate(zip(whole_ev, got_ev)) if a != b]
    vs_oracle = oracle_mismatches(case, got, got_ev)
    assert not vs_whole and not vs_oracle, (name, pol, vs_whole[:8], vs_oracle[:8])


@pytest.mark.parametrize("name", ("rw-128-ref-brb", "rw-256-ref-brb"))
def test_reset_with_records_in_flight(name):
    """run(2) leaves records in flight (injected at steps 1 .. 3, arrivals up to D later): reset() and the same batch
    again equals a fresh engine; reset_at and the re-keyed batch equals a fresh engine at that offset."""
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


def _valid_run_equals_oracle(eng, sp):
    R, F = _runner()
    eng.inject(R._injections(sp, 0))
    eng.run()
    st = R.read_state(eng, [sp])
    exp, _dec, delivers = W.I.oracle_run(sp)
    r = st["inst"][0]
    diff = [(k, r[k], exp[k]) for k in W.CKEYS if r[k] != exp[k]]
    assert not diff and r["deliveries"] == delivers, (sp["name"], diff)


def test_table_overflow_is_refused_at_once():
    """A 17th record in flight in one instance: BRC_E_UNSUPPORTED, nothing changed -- the 16 before it run and equal the
    oracle on the same engine."""
    R, F = _runner()
    L = _L()
    sp = W.overflow_spec()
    ok = dict(sp, actions=sp["actions"][:-1])
    with F.open_flagged([sp], inject=False) as eng:
        with pytest.raises(L.EngineError) as err:
            eng.inject(R._injections(sp, 0))
        assert err.value.code == L.E_UNSUPPORTED and "records in flight" in str(err.value), str(err.value)
        _valid_run_equals_oracle(eng, ok)


def _plain(n, f, seed, byz, **kw):
    return dict(S.brb_spec(n, f, seed, W.UNIF, 3, W.OFFSET, [(0, 0, 0)], byzantine=byz, **kw), step_cap=W.I.STEP_CAP)


def test_honest_sender_is_still_refused():
    R, F = _runner()
    L = _L()
    sp = dict(_plain(70, 23, 0x2E5800E0, W.BYZ70), name="refused-honest-wide")
    valid = dict(t=0, kind=L.INJ_SEND, instance=0, node=1, kp=1, s=0, value=0, dst=(1 << 70) - 1)
    bad = dict(t=1, kind=L.INJ_MSG, type=L.ECHO, instance=0, node=64, kp=0, s=0, value=0, dst=0b101 | 1 << 65)
    with F.open_flagged([sp], inject=False) as eng:
        with pytest.raises(L.EngineError) as err:
            eng.inject([valid, bad])             # the valid record ahead of it is not kept either
        assert err.value.code == L.E_UNSUPPORTED and "Byzantine sender" in str(err.value), str(err.value)
        _valid_run_equals_oracle(eng, sp)


@pytest.mark.parametrize("what", ("narrow", "connection"))
def test_create_refuses_the_flag(what):
    R, F = _runner()
    L = _L()
    sp = _plain(40, 13, 0x2E5800E1, [38, 39]) if what == "narrow" else _plain(70, 23, 0x2E5800E2, W.BYZ70, peer_mode="connection")
    with pytest.raises(L.EngineError) as err:
        F.open_flagged([sp], inject=False).close()
    assert err.value.code == L.E_INVALID
    assert ("n > 64" if what == "narrow" else "connection peers") in str(err.value), str(err.value)
    # the same configuration without the flag is created
    F.open_flagged([sp], inject=False, wide_records=False).close()


def test_flagless_wide_engine_refuses_as_before():
    R, F = _runner()
    L = _L()
    sp = dict(_plain(100, 33, 0x2E5800E3, [98, 99]), name="refused-flagless-wide")
    bad = dict(t=1, kind=L.INJ_MSG, type=L.ECHO, instance=0, node=99, kp=0, s=0, value=0, dst=0b101)
    with F.open_flagged([sp], inject=False, wide_records=False) as eng:
        with pytest.raises(L.EngineError) as err:
            eng.inject([bad])
        assert err.value.code == L.E_UNSUPPORTED
        assert "not on the wide kernels (n > 64), whose receivers ballot over the senders' cells" in str(err.value)
        _valid_run_equals_oracle(eng, sp)


def test_replayed_wire_capture_reproduces_the_fixture():
    """wire.Codec.to_injections over the Byzantine replica's captured messages: restricted INJ_MSG records with
    destinations in both words that reproduce the fixture run."""
    from tests.test_wire import codec_for
    R, F = _runner()
    L = _L()
    for c in FIX:
        sp = c["spec"]
        byz = set(sp["byzantine"])
        honest = [x for x in R._injections(sp, 0) if x["kind"] in (L.INJ_PROPOSE,) or x["node"] not in byz]
        replay = codec_for(sp).to_injections(c["wire_byz"])
        assert any(x["kind"] == L.INJ_MSG and x["dst"] >> 64 and x["dst"] & ((1 << 64) - 1) and x["dst"] != (1 << sp["n"]) - 1
                   for x in replay)
        with F.open_flagged([sp], event_capacity=LOG, inject=False) as eng:
            eng.inject(honest + replay)
            eng.run()
            res = eng.instances_result()[0]
            evs = R.instance_events(eng.events(), [sp])[0]
        golden_io.assert_matches(c["result"], dict(res, events=evs), sp["name"])
        assert res["cell_steps"] == c["cell_steps"]
