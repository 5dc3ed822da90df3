"""Preconditions of tests/test_gpu_restricted_msg.py, on the oracle alone (no GPU): the oracle reproduces the
reference fixture of restricted ECHO / READY messages, the restriction matters in every workload case, and no case
overflows the record table."""
import json
import os

import pytest

from oracle import oracle
from tests import golden_io
from tests import restricted_msg_workloads as W
from tests.golden import specs as S

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "restricted_msg", "restricted_msg.json")


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
    restricted = [[a for a in sp["actions"] if W.is_restricted(sp, a)] for sp in specs]
    assert all(restricted)
    assert {(sp["n"], sp["f"], sp["delay_model"], sp["dmax"]) for sp in specs if sp["mode"] == "brb"} == {(7, 2, 1, 4), (16, 5, 2, 8)}
    # an ECHO to one half and a READY to the other, at different steps
    assert any({a["type"] for a in r} == {S.ECHO, S.READY} and len({a["t"] for a in r}) > 1 and
               not (r[0]["dst"] & r[1]["dst"]) for r in restricted)
    # the same replica ECHOes the same key to all later: suppression of the links it used
    assert any(a["kind"] == "byz" and a["type"] == S.ECHO and a["dst"] == (1 << sp["n"]) - 1 and
               any(b["t"] < a["t"] and (b["src"], b["type"], b["kp"], b["s"]) == (a["src"], a["type"], a["kp"], a["s"]) for b in r)
               for sp, r in zip(specs, restricted) for a in sp["actions"])
    cons = [sp for sp in specs if sp["mode"] == "consensus"]
    assert cons and all(sp["n"] == 7 and sp["round_cap"] == 1 for sp in cons)
    # ... with ECHOes of honest proposals' keys
    assert any(a["kp"] not in sp["byzantine"] for sp in cons for a in sp["actions"] if W.is_restricted(sp, a))
    # every captured Byzantine wire message is there, restricted ones on their links only
    for c in FIX:
        sp = c["spec"]
        links = sum(bin(a["dst"]).count("1") for a in sp["actions"] if W.is_restricted(sp, a))
        assert 0 < links < len(c["wire_byz"])


def test_table_covers_every_family():
    cases = W.cases()
    fam = {}
    for c in cases:
        sp = c.specs[0]
        fam.setdefault((c.family, sp["mode"]), []).append(c)
        assert sp["delay_model"] == W.UNIF and sp["dmax"] >= 3
        assert sp["g"] == W.OFFSET and len(c.specs) <= 3 * W.ipw_of(sp["n"]) + 1
        assert [s["g"] for s in c.specs] == list(range(W.OFFSET, W.OFFSET + len(c.specs)))
    want = {("packed4", "brb"), ("packed4", "consensus"), ("packed8", "brb"), ("packed8", "consensus"),
            ("packed16", "brb"), ("packed16", "consensus"), ("packed32", "brb"), ("packed32", "consensus"),
            ("packed16", "spec_brb"), ("packed8", "beb"), ("general64", "brb")}
    assert want <= set(fam)
    assert {c.specs[0]["n"] for c in cases} == {4, 7, 16, 25, 40}
    g64 = W.by_name()["rm-n64-xref-brb"].specs[0]
    assert (g64["n"], g64["f"], g64.get("general_keys")) == (40, 13, True)
    assert all(W.by_name()[n]._late for n in W.INTERLEAVED)


@pytest.mark.parametrize("name", NAMES)
def test_restriction_matters_and_table_holds(name):
    case = W.by_name()[name]
    specs = case.specs
    n = specs[0]["n"]
    exp = W.oracle_results(case)
    # destination sets differ between the instances of a packed item
    dsts = [tuple(sorted((a["t"], a["type"], a["dst"]) for a in sp["actions"] if W.is_restricted(sp, a))) for sp in specs]
    ipw = W.ipw_of(n)
    if ipw > 1:
        item0 = [d for d in dsts[:ipw] if d]
        # (n = 4 has 14 proper subsets: two of eight drawn ones may coincide)
        assert len(set(item0)) >= min(len(item0), 4) > 1
    # every restricted record comes from a Byzantine replica and names a key that exists by then
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
    # the record table: at most XSEND_MAX records per wave item when the batch is injected at once
    items, _empty = W.table_records(specs)
    assert max(items.values()) <= W.XSEND_MAX, (name, items)
    assert sum(items.values()) > 0


def test_empty_remainder_and_mixed_records_are_present():
    empties = {c.name: W.table_records(c.specs)[1] for c in W.cases()}
    assert sum(bool(v) for v in empties.values()) >= 4, empties
    mix = W.by_name()["rm-p8-mix-brb"]
    for sp in mix.specs:
        acts = [a for a in sp["actions"] if a["t"] == 2 and (a["kp"], a["s"]) == (0, 0)]
        assert any(a["kind"] == "brb_send" for a in acts) and any(W.is_restricted(sp, a) for a in acts)


def test_overflow_spec_overflows_and_its_prefix_does_not():
    sp = W.overflow_spec()
    items, _ = W.table_records([sp])
    assert items[0] == W.XSEND_MAX + 1
    ok = dict(sp, actions=sp["actions"][:-1])
    assert W.table_records([ok])[0][0] == W.XSEND_MAX
    assert oracle.run(ok, light=True)["status"] == "quiescent"
