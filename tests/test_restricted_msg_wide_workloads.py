"""Preconditions of tests/test_gpu_restricted_msg_wide.py, on the oracle alone (no GPU): the oracle reproduces the
reference fixture of restricted ECHO / READY messages at n = 70, the restriction matters in every workload case, the
cases hold what the wide kernels can get wrong, and no instance overflows its record table."""
import json
import os

import pytest

from oracle import oracle
from tests import golden_io
from tests import restricted_msg_wide_workloads as W
from tests.golden import specs as S

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "restricted_msg_wide", "restricted_msg_wide.json")


def fixture_cases():
    with open(FIXTURE) as fh:
        return json.load(fh)["cases"]


FIX = fixture_cases()
NAMES = [c.name for c in W.cases()]


@pytest.mark.parametrize("idx", range(len(FIX)), ids=[c["spec"]["name"] for c in FIX])
def test_oracle_reproduces_reference_fixture(idx):
    case = FIX[idx]
    got = oracle.run(case["spec"])
    golden_io.assert_matches(case["result"], got, case["spec"]["name"])
    assert got["cell_steps"] == case["cell_steps"]


def test_fixture_holds_the_cases_it_should():
    specs = [c["spec"] for c in FIX]
    assert {(sp["n"], sp["f"], sp["mode"], sp["delay_model"], sp["dmax"]) for sp in specs} == {(70, 23, "brb", W.UNIF, 4)}
    for c in FIX:
        sp = c["spec"]
        assert len(sp["byzantine"]) == 1 and sp["byzantine"][0] >= 64
        rest = [a for a in sp["actions"] if W.is_restricted(sp, a)]
        # an ECHO to a subset with members on both sides of replica 64
        assert any(a["type"] == S.ECHO and a["dst"] & ((1 << 64) - 1) and a["dst"] >> 64 for a in rest)
        assert all(a["src"] == sp["byzantine"][0] for a in rest)
        # every captured Byzantine wire message is there, on the links of its destination set only
        links = sum(bin(a["dst"]).count("1") for a in rest)
        assert 0 < links <= len(c["wire_byz"]) < 2 * sp["n"] + links
    # the second run sends the same ECHO to everyone afterwards: the links it used are suppressed
    again = [a for a in specs[1]["actions"] if a["kind"] == "byz" and a["type"] == S.ECHO and a["dst"] == (1 << 70) - 1]
    first = [a for a in specs[1]["actions"] if W.is_restricted(specs[1], a) and a["type"] == S.ECHO]
    assert len(again) == 1 and again[0]["t"] > first[0]["t"]
    assert not [a for a in specs[0]["actions"] if a["kind"] == "byz" and a["dst"] == (1 << 70) - 1]
    echo_links = [w for w in FIX[1]["wire_byz"] if json.loads(w[3])["type"] == S.ECHO]
    assert len(echo_links) == 70 and len({w[2] for w in echo_links}) == 70


def test_table_covers_the_shapes():
    cases = W.cases()
    for c in cases:
        assert len(c.specs) == 3 and [s["g"] for s in c.specs] == [777, 778, 779]
    got = {(c.specs[0]["n"], c.specs[0]["mode"], c.specs[0]["delay_model"], c.specs[0]["dmax"]) for c in cases}
    assert got == {(70, "brb", W.UNIF, 4), (70, "consensus", W.SLOW, 8), (70, "spec_brb", W.UNIF, 4), (70, "beb", W.UNIF, 4),
                   (130, "brb", W.GEO, 16), (130, "spec", W.SLOW, 5)}
    sc = W.by_name()["rw-256-spec-cons"].specs[0]
    assert sc["round_cap"] == 1
    # consensus cases: records on honest proposals' keys
    for name in ("rw-128-ref-cons", "rw-256-spec-cons"):
        for sp in W.by_name()[name].specs:
            assert all(a["kp"] not in sp["byzantine"] for a in sp["actions"] if W.is_restricted(sp, a))
            assert any(a["kind"] == "propose" and a["node"] == r["kp"] and a["t"] == 0 for r in sp["actions"] if W.is_restricted(sp, r)
                       for a in sp["actions"])
    assert all(W.by_name()[n]._late for n in W.INTERLEAVED)
    assert {W.by_name()[n].specs[0]["n"] for n in W.GARBAGE} == {70, 130}
    for n in (70, 130):
        assert W.garbage(n, 1) and not W.garbage(n, 1) & ((1 << n) - 1) and W.garbage(n, 1) < 1 << 256


def test_contents_across_the_cases():
    rest = [(sp, a) for c in W.cases() for sp in c.specs for a in sp["actions"] if W.is_restricted(sp, a)]
    assert any(a["src"] >= 64 for _sp, a in rest) and any(a["src"] >= 128 for _sp, a in rest)
    # destinations only in the highest word
    assert any(a["dst"] >> 64 and not a["dst"] & ((1 << 64) - 1) for sp, a in rest if sp["n"] == 70)
    assert any(a["dst"] >> 128 and not a["dst"] & ((1 << 128) - 1) for sp, a in rest if sp["n"] == 130)
    # destinations that are all Byzantine
    assert any(a["dst"] == sum(1 << b for b in sp["byzantine"]) for sp, a in rest)
    for c in W.cases():
        per = [W.table_records(sp) for sp in c.specs]
        assert any(e for _r, e in per), c.name                   # the empty remainder after a full broadcast
        sp = c.specs[0]
        full = [a for a in sp["actions"] if a["kind"] == "byz" and a["type"] != S.SEND and a["dst"] == (1 << sp["n"]) - 1]
        # a broadcast after a restricted record of the same (node, type, key)
        assert any(W.is_restricted(sp, b) and b["t"] < a["t"] and (b["src"], b["type"], b["kp"], b["s"]) ==
                   (a["src"], a["type"], a["kp"], a["s"]) for a in full for b in sp["actions"]), c.name
        # an ECHO and a READY record of one key at one step
        r0 = [a for a in sp["actions"] if W.is_restricted(sp, a)]
        assert any(a["type"] == S.ECHO and b["type"] == S.READY and (a["t"], a["kp"], a["s"]) == (b["t"], b["kp"], b["s"])
                   for a in r0 for b in r0), c.name
        # each instance with destination sets of its own
        sets = [tuple(sorted(a["dst"] for a in s["actions"] if W.is_restricted(s, a))) for s in c.specs]
        assert len(set(sets)) == len(sets), c.name


@pytest.mark.parametrize("name", NAMES)
def test_restriction_matters_and_table_holds(name):
    case = W.by_name()[name]
    specs = case.specs
    exp = W.oracle_results(case)
    for sp in specs:
        assert all(a["src"] in sp["byzantine"] for a in sp["actions"] if W.is_restricted(sp, a))
    # the restriction matters: widened to every peer, at least half of the instances give another result
    differ = 0
    for i, sp in enumerate(specs):
        wide = oracle.run(W.widened(sp))
        wide["events"] = golden_io.canonical_events(wide["events"])
        base = exp[i][0]
        differ += any(base[k] != wide[k] for k in W.CKEYS) or base["events"] != wide["events"]
        assert base["status"] in ("quiescent", "done"), (name, i, base["status"])
    assert 2 * differ >= len(specs), (name, differ, len(specs))
    # the record table: at most XSEND_MAX records per instance when its actions are injected at once
    recs = [W.table_records(sp)[0] for sp in specs]
    assert 0 < max(recs) <= W.XSEND_MAX and all(recs), (name, recs)


def test_overflow_spec_overflows_and_its_prefix_does_not():
    sp = W.overflow_spec()
    assert W.table_records(sp) == (W.XSEND_MAX + 1, 0)
    ok = dict(sp, actions=sp["actions"][:-1])
    assert W.table_records(ok) == (W.XSEND_MAX, 0)
    assert oracle.run(ok, light=True)["status"] == "quiescent"
