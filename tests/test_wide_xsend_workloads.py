"""Preconditions of tests/test_gpu_wide_xsend.py, on the oracle alone (no GPU): the oracle reproduces the reference
fixture of second SENDs of one key at n = 70, the extra SENDs matter in every workload case, the cases hold what the
wide kernels can get wrong, and no instance overflows its record table."""
import json
import os

import pytest

from oracle import oracle
from oracle.schedule import Schedule
from tests import golden_io
from tests import wide_xsend_workloads as W
from tests.golden import specs as S

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "wide_xsend", "wide_xsend.json")
SIBLING = os.path.join(HERE, "golden", "restricted_msg_wide", "restricted_msg_wide.json")


def fixture_cases():
    with open(FIXTURE) as fh:
        return json.load(fh)["cases"]


def wire_messages(case):
    """The fixture's SEND wire messages [t, src, dst, envelope], one per link (stored grouped over destinations)."""
    return sorted([t, src, d, env] for t, src, mask, env in case["wire_send"] for d in range(case["spec"]["n"])
                  if (int(mask, 16) >> d) & 1)


FIX = fixture_cases()
NAMES = [c.name for c in W.cases()]


@pytest.mark.parametrize("idx", range(len(FIX)), ids=[c["spec"]["name"] for c in FIX])
def test_oracle_reproduces_reference_fixture(idx):
    case = FIX[idx]
    got = oracle.run(case["spec"])
    golden_io.assert_matches(case["result"], got, case["spec"]["name"])
    assert got["cell_steps"] == case["cell_steps"]
    # the DELIVER upcalls: the same set as the reference issued (its order is what the class API replays)
    assert sorted(map(list, got["events"]["deliver"])) == sorted(case["result"]["raw_order"]["deliver"])


def test_fixture_holds_the_cases_it_should():
    assert os.path.getsize(FIXTURE) <= os.path.getsize(SIBLING)
    specs = [c["spec"] for c in FIX]
    assert [(sp["n"], sp["f"], sp["mode"], sp["delay_model"], sp["dmax"], sp["byzantine"], sp["peer_mode"]) for sp in specs] == \
        [(70, 23, "brb", m, d, [68], "sender") for m, d in ((W.UNIF, 4), (W.SLOW, 8), (W.UNIF, 4), (W.SLOW, 8))]
    for j, c in enumerate(FIX):
        sp = c["spec"]
        ex = W.extra_sends(sp)
        who = [(a["t"], a.get("node", a.get("src")), a["kp"]) for a in ex]
        # origin 0's payload from node 65 and again from node 0, origin 66's from node 3, key 0 from Byzantine 68
        assert sorted(n for _t, n, _k in who) == [0, 3, 65, 68] and (2, 3, 66) in who
        own = next(t for t, n, k in who if n == 0)
        others = [t for t, n, k in who if k == 0 and n != 0]
        assert (own < min(others)) == (j >= 2) and (min(others) < own) == (j < 2)
        b = next(a for a in ex if a.get("src") == 68)
        assert b["dst"] == sum(1 << d for d in (1, 5, 63, 64, 69))
        # the extra SENDs move the result
        base, wo = oracle.run(sp, light=True), oracle.run(W.without_extras(sp), light=True)
        assert base["msgs_sent"] > wo["msgs_sent"] and base["arrivals"] > wo["arrivals"]
        # the wire: every SEND on the links it travelled; node 0's repeat on none (sender peers)
        wire = wire_messages(c)
        assert len(wire) == 4 * 70 + 5 and {(w[1], json.loads(w[3])["type"]) for w in wire} == {(x, S.SEND) for x in (0, 3, 65, 66, 68)}
        assert not [w for w in wire if w[1] == 0 and w[0] > 0]


def test_table_covers_the_shapes():
    cases = W.cases()
    for c in cases:
        assert len(c.specs) == W.COUNT <= 4 and [s["g"] for s in c.specs] == [777 + i for i in range(W.COUNT)]
    got = {(c.specs[0]["n"], c.specs[0]["mode"], c.specs[0]["delay_model"], c.specs[0]["dmax"], c.inst[1], c.inst[2]) for c in cases}
    assert got == {(70, "brb", W.SLOW, 8, 128, 8), (70, "brb", W.UNIF, 4, 128, 4), (70, "spec_brb", W.UNIF, 4, 128, 4),
                   (70, "beb", W.UNIF, 4, 128, 4), (70, "consensus", W.SLOW, 8, 128, 8), (128, "brb", W.SLOW, 8, 128, 8),
                   (130, "brb", W.GEO, 16, 256, 16), (130, "spec_brb", W.UNIF, 4, 256, 4)}
    assert len(W.INTERLEAVED) == 3 and all(W.by_name()[n]._late for n in W.INTERLEAVED)
    assert {W.by_name()[n].specs[0]["n"] for n in W.GARBAGE} == {70, 128, 130}
    for n in (70, 128, 130):
        assert W.garbage(n, 1) and not W.garbage(n, 1) & ((1 << n) - 1) and W.garbage(n, 1) < 1 << 256


def _senders(sp):
    return [a.get("node", a.get("src")) for a in W.extra_sends(sp)]


def test_contents_across_the_cases():
    B = W.by_name()
    for c in W.cases():
        # each instance with senders and destination sets of its own
        sets = [tuple((a.get("node", a.get("src")), a.get("dst")) for a in W.extra_sends(sp)) for sp in c.specs]
        assert all(sets) and len(set(sets)) == len(sets), c.name
    # n = 70: extra SENDs from both sides of replica 64, to destinations on both sides
    s70 = [x for sp in B["xw-128-ref-brb"].specs + B["xw-128-ref-unif"].specs for x in _senders(sp)]
    assert any(x < 64 for x in s70) and any(x >= 64 for x in s70)
    d70 = [a["dst"] for sp in B["xw-128-ref-unif"].specs for a in W.extra_sends(sp) if "dst" in a]
    assert any(m & ((1 << 64) - 1) and m >> 64 for m in d70)
    # n = 128: sender 127;  n = 130: senders in words 1 and 2, a destination set in word 2 only among the remainders
    assert 127 in [x for sp in B["xw-128full-ref-brb"].specs for x in _senders(sp)]
    s130 = [x for sp in B["xw-256-ref-brb"].specs for x in _senders(sp)]
    assert any(64 <= x < 128 for x in s130) and any(x >= 128 for x in s130)
    assert any(a["dst"] >> 128 for sp in B["xw-256-ref-brb"].specs for a in W.extra_sends(sp) if "dst" in a)
    for name in ("xw-128-ref-unif", "xw-128-spec-brb", "xw-256-spec-brb", "xw-128full-ref-brb", "xw-256-ref-brb"):
        specs = B[name].specs
        # "split": a restricted first SEND to A, an extra SEND of another node to B overlapping A, the origin's own to C
        sp = specs[0]
        sends = [a for a in sp["actions"] if a["kind"] == "byz" and a["type"] == S.SEND]
        first, second, third = sends
        assert first["src"] == third["src"] != second["src"] and first["t"] < second["t"] < third["t"]
        assert first["dst"] & second["dst"] and second["dst"] & ~first["dst"] and third["dst"] & ~first["dst"]
        assert first["dst"] != (1 << sp["n"]) - 1
        # "with-records": an extra SEND, a restricted ECHO and a restricted READY of one key at one step
        sp = specs[2]
        rec = [a for a in sp["actions"] if a["kind"] == "byz"]
        assert {a["type"] for a in rec} == {S.SEND, S.ECHO, S.READY} and len({(a["t"], a["kp"], a["s"], a["src"]) for a in rec}) == 1
        assert all(a["dst"] != (1 << sp["n"]) - 1 for a in rec) and rec[0] in W.extra_sends(sp)
    # "same-step": under every delay model some honest receiver's links from the two senders have one delay, so the
    # first SEND and the extra one land on one cell in one step (both are sent at step 0)
    for name in ("xw-128-ref-unif", "xw-128-beb-brb", "xw-256-spec-brb", "xw-128full-ref-brb"):
        sp = B[name].specs[1]
        a, b, again = [x for x in sp["actions"] if x["kind"] == "brb_send"]
        assert a["t"] == b["t"] == 0 and a["node"] != b["node"] and again["node"] == a["node"] and again["t"] == 1
        sch = Schedule(sp["n"], sp["f"], sp["seed"], sp["delay_model"], sp["dmax"], sp.get("dconst", 1))
        hon = [d for d in range(sp["n"]) if d not in sp["byzantine"]]
        assert any(sch.delay(sp["g"], a["node"], d) == sch.delay(sp["g"], b["node"], d) for d in hon), name
    # best-effort broadcast: the extra SENDs deliver where the restricted first SEND did not reach ("split")
    for sp in B["xw-128-beb-brb"].specs[::2]:
        assert oracle.run(sp, light=True)["counts"]["deliver"] > oracle.run(W.without_extras(sp), light=True)["counts"]["deliver"]
    # consensus: a Byzantine origin's declared phase-0 key, one half of the peers from each of two Byzantine senders
    for sp in B["xw-128-ref-cons"].specs:
        key = [a for a in sp["actions"] if a["kind"] == "byz_key"]
        sends = [a for a in sp["actions"] if a["kind"] == "byz" and a["type"] == S.SEND]
        assert len(key) == 1 and key[0]["kp"] in sp["byzantine"] and key[0]["s"] == 0 and len(sends) == 2
        assert sends[0]["src"] != sends[1]["src"] and {sends[0]["src"], sends[1]["src"]} <= set(sp["byzantine"])
        assert sends[0]["dst"] & sends[1]["dst"] == 0 and sends[0]["dst"] | sends[1]["dst"] == (1 << 70) - 1
    # slot reuse: sequence numbers 0 and 4 share a slot of the window of 4, both get an extra SEND, and the second
    # generation starts after the first's extra SEND has gone quiet (the run does not overflow)
    wc = B["xw-128-ref-wrap"]
    assert wc.key_window == 4
    for sp in wc.specs:
        assert sorted({a["s"] for a in W.extra_sends(sp)}) == [0, 4]


@pytest.mark.parametrize("name", NAMES)
def test_extra_sends_matter_and_table_holds(name):
    case = W.by_name()[name]
    specs = case.specs
    exp = W.oracle_results(case)
    differ = 0
    for i, sp in enumerate(specs):
        base = exp[i][0]
        assert base["status"] in ("quiescent", "done"), (name, i, base["status"])
        # real work: messages arrive and honest replicas answer them
        assert base["arrivals"] > sp["n"] and base["cell_steps"] > sp["n"] and base["counts"]["deliver"] + base["counts"]["send"] > 2
        wo = oracle.run(W.without_extras(sp))
        wo["events"] = golden_io.canonical_events(wo["events"])
        differ += any(base[k] != wo[k] for k in W.CKEYS) or base["events"] != wo["events"]
    assert 2 * differ >= len(specs), (name, differ, len(specs))
    # the record table: at most XSEND_MAX records per instance when its actions are injected at once
    recs = [W.table_records(sp)[0] for sp in specs]
    assert 0 < max(recs) <= W.XSEND_MAX and all(recs), (name, recs)


def test_a_repeat_with_no_link_left_is_in_the_table():
    assert any(W.table_records(sp)[1] for c in W.cases() for sp in c.specs)


def test_overflow_spec_overflows_and_its_prefix_does_not():
    sp = W.overflow_spec()
    assert W.table_records(sp) == (W.XSEND_MAX + 1, 0)
    ok = dict(sp, actions=sp["actions"][:-1])
    assert W.table_records(ok) == (W.XSEND_MAX, 0)
    assert oracle.run(ok, light=True)["status"] == "quiescent"
