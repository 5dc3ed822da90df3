"""Preconditions of tests/test_gpu_life_windows.py, checked on the C oracle alone (no GPU): every
workload of tests/life_window_workloads.py ends DONE on its sampled ids, the late-step workloads stop
after step 256 (the slow-set one: 128), and every honest replica decides at least round_cap times where
the GPU test claims it -- so a GPU run is not spent finding a workload that stops early.  The oracle's
results are the ones the GPU tests compare with (one cache, tests/life_window_workloads.oracle_sample)."""
import pytest

from tests import life_window_workloads as T

W = T.workloads()


def test_table_covers_every_part():
    for p, least in (("a", 9), ("b", 12), ("c", 6), ("d", 2)):
        assert len(T.part(p)) >= least, p
    L = T._L()
    cells = {(W[k]["kw"]["key_window"], W[k]["kw"].get("mode", L.MODE_REFERENCE), W[k]["kw"].get("peer_mode", L.PEER_SENDER))
             for k in T.part("a")}
    assert cells == {(q, m, pm) for q in (32, 64, 128)
                     for m, pm in ((L.MODE_REFERENCE, L.PEER_SENDER), (L.MODE_BEB, L.PEER_SENDER),
                                   (L.MODE_REFERENCE, L.PEER_CONNECTION))}
    for name in T.part("a"):
        cap, half_overflows = T.PROBED[name]
        assert cap == W[name]["kw"]["round_cap"] > 0 and half_overflows > 0, name


@pytest.mark.parametrize("name", sorted(W))
def test_workload_preconditions(name):
    w = W[name]
    kw = w["kw"]
    ids = T.sample_ids(name, w)
    assert ids[0] == 0 and ids[1] == w["count"] - 1 and len(set(ids)) == len(ids) >= 3
    if kw["n"] == 64 and kw["round_cap"] >= 32:
        assert len(ids) == 3                       # the oracle takes seconds there: the boundary ids plus one
    else:
        assert len(ids) >= 4
    honest = [d for d in range(kw["n"]) if d not in kw.get("byzantine", ())]
    for i, (exp, first, last, count) in T.oracle_sample(name, w).items():
        assert exp["status"] == "done", (name, i, exp["status"])
        assert exp["t_stop"] > w["t_floor"], (name, i, exp["t_stop"])
        assert all(d in first for d in honest), (name, i)
        assert not any(d in first for d in kw.get("byzantine", ())), (name, i)
        if w["decides"]:
            assert min(count[d] for d in honest) >= kw["round_cap"], (name, i)
