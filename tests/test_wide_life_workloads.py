"""Preconditions of tests/test_gpu_wide_life.py, on the C oracle alone (no GPU): every batch of
tests/wide_life_workloads.py is non-vacuous, the window-16 batch needs its window, the slow-set batches have both
receiver classes, and the oracle is fast enough to use.  Plus the binding's side of the interface: the flag bit and
the ABI version."""
import time

import pytest

from tests import wide_life_workloads as WL
from tests import wide_window_workloads as W

NAMES = [b.name for b in WL.batches()]
ORACLE_SECONDS = 60.0                        # every oracle run of the module together, wall clock
_TOOK = []


def _results(batch):
    """oracle_results; the first call makes every batch's runs (WL.oracle_all) and keeps the time they took."""
    if not _TOOK:
        _TOOK.append(WL.oracle_all())
    return WL.oracle_results(batch)


@pytest.mark.parametrize("name", NAMES)
def test_batch_preconditions(name):
    b = WL.by_name()[name]
    specs = b.specs
    sp0 = specs[0]
    assert len(specs) == b.count and b.count in (2, WL.COUNT)
    assert 64 < sp0["n"] <= 256 and sp0.get("peer_mode", "sender") == "sender" and sp0.get("nv", 1) == 1
    assert sp0["delay_model"] in (WL.CONST, WL.SLOW) and sp0["dmax"] <= 8
    assert sorted(sp0["byzantine"]) == sorted(b.byz)
    assert all(a["kind"] == "propose" and a["t"] == 0 for sp in specs for a in sp["actions"]), "no injections"
    npad = 128 if sp0["n"] <= 128 else 256
    assert WL.lds_bytes_life_wide(npad, b.q, 1, sp0["mode"] == "spec") <= 160 * 1024
    res = _results(b)
    hon = [d for d in range(sp0["n"]) if d not in b.byz]
    status = [exp["status"] for (exp, _dec, _n) in res.values()]
    print(name, status, [exp["t_stop"] for (exp, _dec, _n) in res.values()])
    if b.stepcap:
        assert sp0["round_cap"] == 0 and sp0["step_cap"] == WL.STEPCAP_AT
        assert all(s == "stepcap" for s in status), status
        assert all(exp["t_stop"] <= WL.STEPCAP_AT and exp["cell_steps"] > 0 for (exp, _dec, _n) in res.values())
    else:
        # non-vacuous: an instance ends `done` with every honest replica decided
        assert any(exp["status"] == "done" and all(d in dec for d in hon) for (exp, dec, _n) in res.values()), status
        assert all(exp["t_stop"] < sp0["step_cap"] for (exp, _dec, _n) in res.values())
    if sp0["delay_model"] == WL.SLOW and sp0["dmax"] > 1:
        sizes = [WL.class_sizes(sp) for sp in specs]
        assert any(nf > 0 and ns > 0 for (nf, ns) in sizes), sizes
    else:
        assert all(WL.class_sizes(sp)[0] == 0 for sp in specs)
    if b.proposals == "loaded":
        assert {a["value"] for sp in specs for a in sp["actions"]} == {1, 2, 3}
    if name == WL.Q16:
        need = [W.needs(exp, sp0["dmax"]) for (exp, _dec, _n) in res.values()]
        assert b.q == 16 and b.wide_windows and max(need) > 8, need      # window 8 would overflow


def test_shapes_cover_the_issue_list():
    by = WL.by_name()
    ns = {b.specs[0]["n"] for b in WL.batches()}
    assert {70, 90, 100, 130, 256} <= ns
    assert any(x >= 64 for x in by["wl-256-ref-byz"].byz) and any(x < 64 for x in by["wl-256-ref-byz"].byz)
    assert {b.specs[0]["mode"] for b in WL.batches()} == {"consensus", "spec", "beb_consensus"}
    assert any(b.specs[0]["delay_model"] == WL.CONST and b.specs[0]["dconst"] == 2 for b in WL.batches())
    assert any(b.specs[0]["dmax"] == 1 for b in WL.batches())


def test_oracle_time_budget():
    """The whole module's oracle runs stay under a minute (shrink n = 256's batch, not the check).  Runs that another
    test module made earlier in the same process are not made again, and count nothing."""
    _results(WL.batches()[0])
    print("oracle runs of the module: %.1f s" % _TOOK[0])
    assert _TOOK[0] < ORACLE_SECONDS, _TOOK[0]


def test_flag_and_abi():
    from byzantinerandomizedconsensus_amd import _lib as L
    assert L.FLAG_WIDE_LIFE == WL.FLAG == 16 and L.ABI_VERSION >= 11
    import inspect

    from byzantinerandomizedconsensus_amd.engine import Engine
    assert inspect.signature(Engine.__init__).parameters["wide_life"].default is False


def test_class_api_does_not_set_the_flag():
    """network.Cluster creates its engines without BRC_FLAG_WIDE_LIFE: it injects and logs events."""
    import inspect

    from byzantinerandomizedconsensus_amd import network
    assert "wide_life" not in inspect.getsource(network)
