"""Preconditions of tests/test_gpu_wide_values.py, on the oracle alone (no GPU): the oracle reproduces the reference
fixture of more than three proposal strings at n = 70, every workload case depends on the third bit of its value ids,
the eight-way case fills a replica's value table, the small-f case decides among two ids above the bound, and a
70-node sender-peer cluster keeps eight value ids."""
import json
import os

import pytest

from oracle import oracle
from tests import golden_io
from tests import wide_values_workloads as W
from tests.golden import specs as S

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "wide_values", "wide_values.json")


def fixture_cases():
    with open(FIXTURE) as fh:
        return json.load(fh)["cases"]


FIX = fixture_cases()
NAMES = [c.name for c in W.cases()]


@pytest.mark.parametrize("idx", range(len(FIX)), ids=[c["spec"]["name"] for c in FIX])
def test_oracle_reproduces_reference_fixture(idx):
    """(d)"""
    case = FIX[idx]
    got = oracle.run(case["spec"])
    golden_io.assert_matches(case["result"], got, case["spec"]["name"])
    assert got["cell_steps"] == case["cell_steps"]
    # the DECIDE upcalls: the same set as the reference issued (its order is what the class API replays)
    assert sorted(map(list, got["events"]["decide"])) == sorted(case["result"]["raw_order"]["decide"])


def test_fixture_holds_the_cases_it_should():
    assert os.path.getsize(FIXTURE) <= 32 * 1024          # its siblings: 15 to 30 KB
    specs = [c["spec"] for c in FIX]
    assert [(sp["n"], sp["f"], sp["mode"], sp["delay_model"], sp["dmax"], sp["byzantine"], sp["peer_mode"], sp["round_cap"])
            for sp in specs] == [(70, 23, "consensus", m, d, [], "sender", 2) for m, d in ((W.UNIF, 4), (W.SLOW, 8), (0, 1))]
    assert all(sp["values"] == S.VALUES8 for sp in specs)
    props = [[a["value"] for a in sp["actions"] if a["kind"] == "propose"] for sp in specs]
    assert all(len(p) == 70 for p in props)
    assert props[0].count(4) == 52 and set(props[0]) == {1, 2, 3, 4, 5}              # a majority of id 4
    assert all(props[1].count(v) == 14 for v in (1, 2, 3, 4, 5))                     # a five-way split
    assert props[2].count(5) == 51 and set(props[2]) == {1, 2, 3, 4, 5}              # a majority of id 5 with a tail
    # the slow-set and constant-delay runs decide (the five-way split ends in "-1"); uniform delays stall the
    # reference's broadcast at this size, as in the cons_uniform_n70 fixture
    assert [c["result"]["status"] for c in FIX] == ["quiescent", "done", "done"]
    assert {e[3] for e in FIX[1]["result"]["events"]["decide"]} == {"-1"}


def test_table_covers_the_shapes():
    cases = W.cases()
    for c in cases:
        assert len(c.specs) == W.COUNT and [s["g"] for s in c.specs] == [777 + i for i in range(W.COUNT)]
        assert all(sp["values"] == S.VALUES8 and sp["round_cap"] == 1 for sp in c.specs)
        assert max(a["value"] for sp in c.specs for a in sp["actions"] if "value" in a) >= 4
    assert max(a["value"] for c in cases for sp in c.specs for a in sp["actions"] if a["kind"] == "propose") == 7
    got = {(c.specs[0]["n"], c.specs[0]["mode"], c.inst[1], c.inst[2]) for c in cases}
    assert got == {(70, "consensus", 128, 8), (128, "consensus", 128, 4), (70, "consensus", 128, 16),
                   (130, "beb_consensus", 256, 4), (130, "consensus", 256, 16), (128, "beb_consensus", 128, 8)}
    for c in cases:
        sp = c.specs[0]
        assert (4 if sp["dmax"] <= 4 else 8 if sp["dmax"] <= 8 else 16) == c.inst[2]
    by = W.by_name()
    assert any(a["kind"] == "deliver" and a["value"] >= 4 for a in by["wv-256-deliver"].specs[0]["actions"])
    assert {a["value"] for sp in by["wv-256-deliver"].specs for a in sp["actions"] if a["kind"] == "deliver"} == {4, 5, 6, 7}
    keys = [a for a in by["wv-256-byzkey"].specs[1]["actions"] if a["kind"] == "byz_key"]
    assert keys and all(a["value"] == 6 for a in keys)
    assert any(a["kind"] == "byz" and a["type"] == S.SEND for a in by["wv-256-byzkey"].specs[1]["actions"])
    both = by["wv-128-both"]
    assert both.both and [c.name for c in cases if c.both] == ["wv-128-both"]
    for sp in both.specs:
        rec = [a for a in sp["actions"] if a["kind"] == "byz" and a["type"] == S.ECHO]
        assert len(rec) == 1 and rec[0]["src"] in sp["byzantine"] and rec[0]["dst"] != (1 << 70) - 1 and rec[0]["dst"] >> 64
    assert set(W.SLICED) | {W.RESET_AT} <= set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_the_third_bit_matters(name):
    """(a): run with every value id folded to two bits, the oracle's result changes for at least half the instances."""
    case = W.by_name()[name]
    changed = 0
    for i, (exp, _dec, _n) in W.oracle_results(case).items():
        assert exp["status"] in ("done", "quiescent"), (name, i, exp["status"])
        low = oracle.run(W.fold(case.specs[i]))
        low["events"] = golden_io.canonical_events(low["events"])
        changed += any(low[k] != exp[k] for k in W.CKEYS) or low["events"] != exp["events"]
    assert 2 * changed >= W.COUNT, (name, changed)
    # ... and an id >= 4 is decided somewhere in the case
    assert any(v >= 4 for _i, (_e, dec, _n) in W.oracle_results(case).items() for ds in dec.values() for (_r, _t, v) in ds), name


def _replays(name):
    case = W.by_name()[name]
    out = []
    for i, sp in enumerate(case.specs):
        exp = oracle.run(sp)
        decides, widest, above = W.replay(sp, exp)
        want = sorted([t, d, r, S.VALUES8.index(v)] for t, d, r, v in exp["events"]["decide"])
        assert sorted(decides) == want, (name, i)          # the replay is the oracle's consensus
        out.append((decides, widest, above))
    return out


def test_eight_way_case_fills_a_value_table():
    """(b): some honest replica inserts eight ids in one window, id 0 among them."""
    reps = _replays("wv-128full-eight")
    assert all(widest == 8 for _d, widest, _a in reps), [w for _d, w, _a in reps]
    for sp in W.by_name()["wv-128full-eight"].specs:
        assert {a["value"] for a in sp["actions"] if a["kind"] == "propose"} == set(range(8))


def test_small_f_case_decides_among_two_ids_above_the_bound():
    """(c): in every instance some decisions find two ids with 2 |hosts| > 4 f; the one inserted first decides -- id
    6, against id 0 and its larger host set -- while the replicas that were handed nothing decide id 0."""
    reps = _replays("wv-128-smallf")
    assert W.by_name()["wv-128-smallf"].specs[0]["f"] == 5
    for decides, _w, above in reps:
        two = [(d, a) for d, a in zip(decides, above) if len(a) >= 2]
        assert len(two) >= 10 and all(a == [6, 0] and d[3] == 6 for d, a in two), two[:4]
        assert all(d[3] == (a[0] if a else 0) for d, a in zip(decides, above))
        assert {d[3] for d in decides} == {0, 6}


def test_wide_sender_cluster_keeps_eight_value_ids():
    """(e): a 70-node cluster with sender peers gets three-bit value ids; its engine is created with
    BRC_FLAG_WIDE_VALUES once consensus nodes are registered.  Connection peers above 64 keep two bits."""
    from byzantinerandomizedconsensus_amd import _lib as L
    from byzantinerandomizedconsensus_amd import network
    assert L.FLAG_WIDE_VALUES == 4 and L.ABI_VERSION >= 9
    network.reset()
    try:
        peers = tuple(("localhost", 9100 + i) for i in range(70))
        c = network.Cluster(peers, dict(network.settings(), peer_mode="sender"))
        assert c.values.cap == 8
        assert [c.values.id_of(s) for s in S.VALUES8] == list(range(8))
        assert not c.wide_values                           # broadcast-only so far
        c.add_consensus(object(), 0)
        assert c.wide_values and not c.wide_records
        k = network.Cluster(peers, dict(network.settings(), peer_mode="connection"))
        k.add_consensus(object(), 0)
        assert k.values.cap == 4 and not k.wide_values
        small = network.Cluster(peers[:40], dict(network.settings(), peer_mode="sender"))
        small.add_consensus(object(), 0)
        assert small.values.cap == 8 and not small.wide_values
    finally:
        network.reset()
