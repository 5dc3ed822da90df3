"""GPU: three-bit consensus value ids (seven proposal strings besides "-1") on the wide step kernels (n > 64) of an
engine created with BRC_FLAG_WIDE_VALUES, against the reference fixture tests/golden/wide_values/ and the C oracle.
tests/wide_values_workloads.py has one batch of three instances per shape; tests/test_wide_values_workloads.py proves
their preconditions on the oracle.  Before the feature brc_create refused the flag bit, brc_inject and
brc_load_proposals refused ids >= 4 above 64 replicas and network.Cluster raised EngineError for a fourth string."""
import ctypes

import numpy as np
import pytest

from tests import golden_io
from tests import wide_values_workloads as W
from tests.golden import specs as S
from tests.test_gpu_step_noevent import state_mismatches
from tests.test_wide_values_workloads import FIX

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in W.cases()]
LOG = 1 << 20


def _runner():
    from tests import engine_runner, wide_records_runner
    return engine_runner, wide_records_runner


def _L():
    from byzantinerandomizedconsensus_amd import _lib
    return _lib


def _open(specs, cap=0, wide_values=True, wide_records=False, loaded=True, key_window=8):
    """The engine of one batch: proposals loaded (or injected), every other action injected, not yet run."""
    from byzantinerandomizedconsensus_amd.engine import Engine
    R, F = _runner()
    L = _L()
    kw = F.engine_kw(specs, cap, key_window)
    eng = Engine(wide_values=wide_values, wide_records=wide_records,
                 proposals=L.PROPOSALS_LOADED if loaded else L.PROPOSALS_NONE, **kw)
    try:
        if loaded:
            eng.load_proposals(R._loaded_proposals(specs))
        inj = []
        for i, sp in enumerate(specs):
            inj += R._injections(dict(sp, actions=[a for a in sp["actions"] if not (loaded and a["kind"] == "propose")]), i)
        eng.inject(inj)
    except Exception:
        eng.close()
        raise
    return eng


def _read(eng, specs, cap):
    R, F = _runner()
    st = R.read_state(eng, specs)
    ev = None if not cap else [R.sort_result({"events": e})["events"] for e in R.instance_events(eng.events(), specs)]
    return st, ev


def _run(case, cap, max_steps=0, **kw):
    with _open(case.specs, cap, wide_records=case.both, **kw) as eng:
        if max_steps:
            while eng.run(max_steps):
                pass
        else:
            eng.run()
        assert eng.last_kernel() == "step"
        return _read(eng, case.specs, cap)


def oracle_mismatches(case, st, events=None):
    """Differences from the oracle: counters, cell_steps, deliveries, every honest replica's record, the ordered event
    lists, the round histogram and the eight-id decision histogram."""
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
        if bool(r["decided"]) != all(d in dec for d in hon):
            out.append(("oracle", i, "decided", r["decided"]))
        if events is not None:
            out += [("oracle", i, k + " events", len(events[i][k]), len(exp["events"][k]))
                    for k in ("deliver", "decide", "send") if events[i][k] != exp["events"][k]]
    hist, counts, undecided, dis = W.expected_read_side(case)
    want = {lab: counts.get(v, 0) for v, lab in enumerate(S.VALUES8)}
    want["undecided"] = undecided
    if st["hist"] != hist:
        out.append(("oracle", "round_histogram", st["hist"], hist))
    if st["dec"] != (want, dis):                     # brc_read_value_decisions (read_state: eight labels)
        out.append(("oracle", "decisions", st["dec"], (want, dis)))
    return out


def test_fixture_runs_equal_the_reference():
    for c in FIX:
        sp = c["spec"]
        with _open([sp], LOG, loaded=False) as eng:
            eng.run()
            st, ev = _read(eng, [sp], LOG)
        golden_io.assert_matches(c["result"], dict(st["inst"][0], events=ev[0]), sp["name"])
        assert st["inst"][0]["cell_steps"] == c["cell_steps"], sp["name"]


def test_class_api_runs_the_fixture():
    """The fixture's specs through the reference's class API: 70 sender-peer ByzantineRandomizedConsensus nodes.  The
    decide upcalls are the reference's, at its steps and in its order.  The fixture's f = 23 violates the
    constructor's N > 5f assert (the generator runs the reference under python -O for the same reason), so the nodes
    are built as the constructor builds them, minus that line."""
    import queue
    from byzantinerandomizedconsensus_amd.core.brbroadcast import BRBroadcast
    from byzantinerandomizedconsensus_amd import network
    from byzantinerandomizedconsensus_amd.base.consensus import IConsensusHandler
    from byzantinerandomizedconsensus_amd.core.byzantinerandomizedconsensus import ByzantineRandomizedConsensus
    L = _L()
    saved = network.settings()
    try:
        for case in FIX:
            sp = case["spec"]
            network.reset()
            network.configure(delay_model=sp["delay_model"], delay_max=sp["dmax"], delay_const=sp.get("dconst", 1),
                              seed=sp["seed"], instance_id=sp["g"], peer_mode="sender", step_cap=sp["step_cap"],
                              round_cap=sp["round_cap"])
            got = []

            class H(IConsensusHandler):
                def __init__(self, i):
                    self.i = i

                def decide(self, value):
                    got.append([cluster.t, self.i, value])

            peers = [("localhost", 7400 + i) for i in range(sp["n"])]
            nodes = []
            for i, p in enumerate(peers):
                nd = object.__new__(ByzantineRandomizedConsensus)
                nd.message_queue, nd.N, nd.f, nd.round, nd.phase = queue.Queue(20), sp["n"], sp["f"], 0, 0
                nd.brb = BRBroadcast(sp["n"], sp["f"], p, peers, nd)
                nd.consensus_user, nd.host_address = H(i), p
                nd.brb.cluster.add_consensus(nd, nd.brb.node_id)
                nd.brb.broadcast_listener()
                nodes.append(nd)
            cluster = nodes[0].brb.cluster
            for a in sp["actions"]:
                assert a["kind"] == "propose" and a["t"] == 0
                nodes[a["node"]].propose(sp["values"][a["value"]])
            status = cluster.run()
            assert cluster.engine.cfg.flags & L.FLAG_WIDE_VALUES and cluster.values.cap == 8
            assert status == case["result"]["status"], sp["name"]
            exp = [[t, node, v] for (t, node, _r, v) in case["result"]["raw_order"]["decide"]]
            assert got == exp, sp["name"]
    finally:
        network.reset()
        network.configure(**saved)


@pytest.mark.parametrize("cap", (0, LOG), ids=("nolog", "log"))
@pytest.mark.parametrize("name", NAMES)
def test_workload_equals_oracle(name, cap):
    L = _L()
    case = W.by_name()[name]
    with _open(case.specs, cap, wide_records=case.both) as eng:
        eng.run()
        assert eng.last_kernel() == "step"
        assert bool(eng.cfg.flags & L.FLAG_WIDE_RECORDS) == case.both and eng.cfg.flags & L.FLAG_WIDE_VALUES
        st, ev = _read(eng, case.specs, cap)
        print(name, cap, [{k: r[k] for k in W.CKEYS} for r in st["inst"]], st["dec"])
        # an id >= 4 was decided (tests/test_wide_values_workloads.py): the four-id read-out refuses
        assert any(st["dec"][0][lab] for lab in S.VALUES8[4:])
        arr, dis = np.zeros(5, dtype=np.uint64), ctypes.c_uint64(0)
        with pytest.raises(L.EngineError) as err:
            eng._chk(eng._lib.brc_read_decisions(eng._h, arr.ctypes.data_as(ctypes.c_void_p), ctypes.byref(dis)))
        assert err.value.code == L.E_STATE and "brc_read_value_decisions" in str(err.value)
    assert st["stats"]["running"] == 0 and st["stats"]["events_dropped"] == 0
    diff = oracle_mismatches(case, st, ev)
    assert not diff, (name, diff[:8])


@pytest.mark.parametrize("name", W.SLICED)
def test_sliced_run_equals_oneshot(name):
    """run(3) until nothing runs: the eight host-mask planes and the 3-bit `order` persist across launches."""
    case = W.by_name()[name]
    whole, whole_ev = _run(case, LOG)
    got, got_ev = _run(case, LOG, max_steps=3)
    diff = state_mismatches(whole, got, "one-shot vs slices of 3")
    diff += [("events", i) for i, (a, b) in enumerate(zip(whole_ev, got_ev)) if a != b]
    assert not diff, (name, diff[:8])
    assert not oracle_mismatches(case, got, got_ev)


def test_reset_at_equals_a_fresh_engine():
    """A run stopped in mid-consensus (values of ids >= 4 in the host masks), reset_at, the re-keyed batch: every
    read_state() field equals a fresh engine at that offset."""
    R, F = _runner()
    case = W.by_name()[W.RESET_AT]
    moved = [dict(sp, g=sp["g"] + W.COUNT) for sp in case.specs]
    with _open(moved) as eng:
        eng.run()
        fresh = R.read_state(eng, moved)
    with _open(case.specs) as eng:
        assert eng.run(7) > 0
        assert any(r["deliveries"] for r in eng.instances_result())
        eng.reset_at(W.OFFSET + W.COUNT)
        eng.load_proposals(R._loaded_proposals(moved))
        inj = []
        for i, sp in enumerate(moved):
            inj += R._injections(dict(sp, actions=[a for a in sp["actions"] if a["kind"] != "propose"]), i)
        eng.inject(inj)
        eng.run()
        again = R.read_state(eng, moved)
    assert not state_mismatches(fresh, again, "fresh at the new offset vs after reset_at()")
    assert any(fresh["dec"][0][lab] for lab in S.VALUES8[4:])


@pytest.mark.parametrize("n,model,dmax", ((70, W.SLOW, 8), (130, W.GEO, 16)), ids=("n70", "n130"))
def test_binary_proposals_equal_the_flagless_engine(n, model, dmax):
    """Philox-drawn binary proposals: the flagged engine equals the flagless one in every read_state() field and
    event, with and without an event log."""
    R, F = _runner()
    specs = [dict(S.cons_spec(n, 5, 0x3B17B000 + n, model, dmax, W.OFFSET + i, round_cap=1), name="wv-binary-%d/%d" % (n, i),
                  step_cap=W.I.STEP_CAP) for i in range(W.COUNT)]
    for cap in (0, LOG):
        out = []
        for flag in (False, True):
            with _open(specs, cap, wide_values=flag) as eng:
                eng.run()
                out.append(_read(eng, specs, cap))
        (a, aev), (b, bev) = out
        assert not state_mismatches(a, b, "flagless vs flagged")
        assert aev == bev
        assert a["stats"]["running"] == 0 and any(r["status"] == "done" for r in a["inst"])


def _cfg(n=70, **kw):
    L = _L()
    base = dict(n=n, f=5, instances=1, protocol="consensus", seed=1, delay_model=L.DELAY_SLOWSET, delay_max=4,
                round_cap=1, step_cap=400, key_window=8)
    base.update(kw)
    return base


def test_refusals():
    from byzantinerandomizedconsensus_amd.engine import Engine
    L = _L()
    for kw, word in ((dict(n=64), "n > 64"), (dict(peer_mode=L.PEER_CONNECTION), "sender peers"),
                     (dict(mode=L.MODE_SPEC, key_window=4), "BRC_MODE_SPEC")):
        with pytest.raises(L.EngineError) as err:
            Engine(wide_values=True, **_cfg(**kw))
        assert err.value.code == L.E_INVALID and "BRC_FLAG_WIDE_VALUES" in str(err.value) and word in str(err.value), str(err.value)
        Engine(**_cfg(**kw)).close()                       # the configuration itself is valid
    propose = lambda v: [dict(t=0, kind=L.INJ_PROPOSE, instance=0, node=0, value=v)]      # noqa: E731
    with Engine(wide_values=True, **_cfg()) as eng:
        with pytest.raises(L.EngineError) as err:
            eng.inject(propose(8))
        assert err.value.code == L.E_INVALID
        eng.inject(propose(7))
    with Engine(wide_values=True, proposals=L.PROPOSALS_LOADED, **_cfg()) as eng:
        with pytest.raises(L.EngineError) as err:
            eng.load_proposals([[8] * 70])
        assert err.value.code == L.E_INVALID
        eng.load_proposals([[7] * 70])
    # without the flag: as before
    with Engine(**_cfg()) as eng:
        with pytest.raises(L.EngineError) as err:
            eng.inject(propose(4))
        assert err.value.code == L.E_INVALID and "BRC_FLAG_WIDE_VALUES" in str(err.value)
        eng.inject(propose(3))
    with Engine(proposals=L.PROPOSALS_LOADED, **_cfg()) as eng:
        with pytest.raises(L.EngineError) as err:
            eng.load_proposals([[4] * 70])
        assert err.value.code == L.E_INVALID and "BRC_FLAG_WIDE_VALUES" in str(err.value)
        eng.load_proposals([[3] * 70])
