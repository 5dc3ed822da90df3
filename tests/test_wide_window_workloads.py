"""Preconditions of tests/test_gpu_wide_windows.py, on the C oracle alone (no GPU): every workload of
tests/wide_window_workloads.py ends `done`, its send log needs more than half the tested key window (so the window is in
use), and an oracle run stays short enough for the suite."""
import time

import pytest

from tests import wide_window_workloads as W
from tests.golden import specs as S

NAMES = [c.name for c in W.cases()]
# an oracle run's CPU time (of its thread: a loaded machine does not change it).  W.SLOW_ORACLE names the exception,
# the reference protocol at n = 130: round cap 4 is the lowest at which its window is in use, 9.4 to 10.8 s a run
ORACLE_SECONDS = 10.0


@pytest.mark.parametrize("name", NAMES)
def test_workload_preconditions(name):
    from oracle import oracle
    case = W.by_name()[name]
    specs = case.specs
    assert len(specs) == W.COUNT and 8 <= W.COUNT <= 32
    sp0 = specs[0]
    assert sp0["n"] > 64 and sp0["mode"] in ("consensus", "beb_consensus") and sp0.get("peer_mode", "sender") == "sender"
    assert case.q * case.nv in (16, 32) and sp0.get("nv", 1) == case.nv
    assert len(case.byz) >= 2 and len({b // 64 for b in case.byz}) >= 2, "silent Byzantine replicas in different words"
    assert W.accepted(sp0["n"], case.inst[3], case.q, case.nv, sp0["delay_model"], sp0["dmax"])
    assert not W.accepted(sp0["n"], case.inst[3], case.q, case.nv, sp0["delay_model"], sp0["dmax"], flag=False)
    if name in W.SAME_SPECS:
        strip = lambda sp: {k: v for k, v in sp.items() if k != "name"}                      # noqa: E731
        assert [strip(sp) for sp in specs] == [strip(sp) for sp in W.by_name()[W.SAME_SPECS[name]].specs]
    res = W.oracle_results(case)
    if name in W.SAME_SPECS:                               # timed with the batch whose oracle runs it shares
        first, took = res[0][0], 0.0
    else:
        t0 = time.thread_time()
        first = oracle.run(specs[0], kinds=("send",))
        took = time.thread_time() - t0
    assert took < ORACLE_SECONDS or name in W.SLOW_ORACLE, (name, took)
    assert all(exp["status"] == "done" for (exp, _dec, _n) in res.values()), [(i, r[0]["status"]) for i, r in res.items()]
    assert all(exp["t_stop"] < W.I.STEP_CAP for (exp, _dec, _n) in res.values())
    need = [W.needs(exp, sp0["dmax"]) for (exp, _dec, _n) in res.values()]
    print(name, "oracle %.1f s" % took, "window needed per instance", need, "keys", len({(e[3], e[4]) for e in first["events"]["send"]}))
    if case.half is not None:
        # some origin first SENDs phase s + Q / 2 or later while its phase-s key was still sending
        assert max(need) > case.half, (name, need)
    elif not case.rec:
        assert max(need) > 8, (name, need)                # beyond what an unflagged engine holds
    if case.v8:
        assert all(any(a["kind"] == "propose" and a["value"] >= 4 for a in sp["actions"]) for sp in specs)
        assert sp0["values"] == S.VALUES8
    if case.rec:
        from tests import wide_xsend_workloads as X
        for sp in specs:
            slots = [a["kp"] * case.q + a["s"] % case.q for a in sp["actions"] if a["kind"] == "byz"]
            assert min(slots) >= 2048, slots                      # beyond the 11 bits a slot index took so far
            assert len(X.extra_sends(sp)) == 1 and X.table_records(sp) == (2, 0)
            assert any(a["kind"] == "byz" and a["type"] == S.ECHO and a["dst"] != (1 << sp["n"]) - 1 for a in sp["actions"])


def test_parity_case_is_an_unflagged_shape():
    case = W.parity_case()
    sp0 = case.specs[0]
    assert W.accepted(sp0["n"], case.inst[3], case.q, case.nv, flag=False)
    assert all(exp["status"] == "done" for (exp, _dec, _n) in W.oracle_results(case).values())


def test_flagged_acceptance_table():
    """A self-check of this suite's model of brc_create (W.accepted, W.lds_bytes_wide: no engine is involved):
    everything required fits, and the one refused family is NPAD 256 with a key window of 32 under per-link delays
    above 8.  tests/test_gpu_wide_windows.py::test_create_equals_the_acceptance_model holds brc_create to the model
    over the same grid."""
    for n in W.GRID_N:
        for model, dmax in W.GRID_DELAYS:
            for q, nv in W.GRID_SLOTS:
                # (the deferred-SEND queue is sq[Q][NPAD] bytes: 16 x 2 and 8 x 4 fit, at 159,920 and 157,872 B)
                want = not (n == 130 and q == 32 and dmax > 8 and model in (W.UNIF, W.GEO))
                assert W.accepted(n, W.REF, q, nv, model, dmax) == want, (n, model, dmax, q, nv)
                assert not W.accepted(n, W.REF, q, nv, model, dmax, flag=False)
                assert not W.accepted(n, W.I.SPEC, q, nv, model, dmax) and not W.accepted(n, W.REF, q, nv, model, dmax, conn=True)
    assert not W.accepted(70, W.REF, 64, 1) and not W.accepted(70, W.REF, 32, 2)
    assert W.lds_bytes_wide(256, 32, 1, 5, 16) == 164016 and W.lds_bytes_wide(256, 32, 1, 2, 16) == 162480
    assert W.lds_bytes_wide(256, 32, 1, 4, 8) == 147120 and W.lds_bytes_wide(128, 32, 1, 5, 16) <= 96 * 1024


def test_wide_sender_consensus_cluster_sets_the_flag():
    """The class API: a consensus cluster above 64 nodes with sender peers creates its engine with
    BRC_FLAG_WIDE_WINDOWS and window 16 (the properties _create_engine passes on; the engine's own configuration is
    checked on the GPU, test_gpu_wide_windows.py); broadcast clusters, connection peers and smaller clusters do not."""
    from byzantinerandomizedconsensus_amd import _lib as L
    from byzantinerandomizedconsensus_amd import network
    assert L.FLAG_WIDE_WINDOWS == W.FLAG == 8 and L.ABI_VERSION >= 10
    network.reset()
    try:
        peers = tuple(("localhost", 9300 + i) for i in range(70))
        c = network.Cluster(peers, dict(network.settings(), peer_mode="sender"))
        assert not c.wide_windows                          # broadcast-only so far
        assert c.key_window == 8
        c.add_consensus(object(), 0)
        assert c.wide_windows and c.wide_values and c.key_window == 16
        k = network.Cluster(peers, dict(network.settings(), peer_mode="connection"))
        k.add_consensus(object(), 0)
        assert not k.wide_windows and k.key_window == 8
        small = network.Cluster(peers[:40], dict(network.settings(), peer_mode="sender"))
        small.add_consensus(object(), 0)
        assert not small.wide_windows and small.key_window == 8
    finally:
        network.reset()
