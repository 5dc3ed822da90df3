"""Preconditions of tests/test_gpu_fault_bounds.py, checked without a GPU: the oracle reproduces the reference fixture
tests/golden/fault_bounds/fault_bounds.json (results, raw upcall order, cell steps); the table of
tests/fault_bound_workloads.py holds the grid it names, every case does real work on the oracle, f MATTERS (at least
half of a case's instances give another oracle result under f = (n - 1) // 3), and the regimes the table claims are
real: nothing delivered where 2 f + 1 exceeds the honest replicas, a phase end on the second delivery, no phase end
under the reference's consensus at f = 0, no slow replica at f = 0, one fast replica at f = n - 1, and windows that hold
every case but the three meant to overflow."""
import json
import os

import pytest

from oracle import oracle
from oracle.schedule import Schedule
from tests import fault_bound_workloads as F
from tests import golden_io
from tests import wide_window_workloads as W
from tests.golden import specs as S

CASES = F.cases()
NAMES = [c.name for c in CASES]
with open(os.path.join(golden_io.GOLDEN, "fault_bounds", "fault_bounds.json")) as _fh:
    FIXTURE = json.load(_fh)["cases"]


# ---- the reference fixture ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(FIXTURE)))
def test_oracle_reproduces_the_fixture(idx):
    case = FIXTURE[idx]
    got = oracle.run(case["spec"])
    golden_io.assert_matches(case["result"], got, "fault_bounds[%d]" % idx)
    assert got["cell_steps"] == case["cell_steps"]
    for k in ("deliver", "decide"):
        assert [list(r) for r in got["events"][k]] == case["result"]["raw_order"][k], (idx, k)


def test_fixture_holds_the_regimes():
    shapes = {(c["spec"]["n"], c["spec"]["f"]) for c in FIXTURE}
    assert {n for n, _ in shapes} == {1, 2, 3, 4, 7, 10} and 12 <= len(FIXTURE) <= 16
    for c in FIXTURE:
        n, f = c["spec"]["n"], c["spec"]["f"]
        assert f in {0, (n - 1) // 3 + 1, (n + 1) // 2, n - 1} and f < n
        assert f != (n - 1) // 3 or n <= 3, (n, f)
    assert {c["spec"]["mode"] for c in FIXTURE} == {"brb", "consensus"}
    assert {c["spec"]["delay_model"] for c in FIXTURE} == {F.UNIF, F.SLOW}
    assert {c["spec"]["round_cap"] for c in FIXTURE if c["spec"]["mode"] == "consensus"} == {1, 2}
    assert {(c["spec"]["n"] + c["spec"]["f"]) % 2 for c in FIXTURE} == {0, 1}
    # 2 f + 1 above the honest replicas: nothing is delivered -- and everywhere else something is
    for c in FIXTURE:
        sp = c["spec"]
        unreachable = 2 * sp["f"] + 1 > sp["n"] - len(sp["byzantine"])
        assert (c["result"]["counts"]["deliver"] == 0) == unreachable, sp["name"]
    assert sum(2 * c["spec"]["f"] + 1 > c["spec"]["n"] - len(c["spec"]["byzantine"]) for c in FIXTURE) >= 4
    assert any(c["spec"]["byzantine"] and 2 * c["spec"]["f"] + 1 <= c["spec"]["n"] for c in FIXTURE)
    # n - f <= 2: the reference's phase ends on delivery n - f + 1
    small = [c for c in FIXTURE if c["spec"]["mode"] == "consensus" and c["spec"]["n"] - c["spec"]["f"] <= 2
             and c["result"]["counts"]["deliver"]]
    assert {(c["spec"]["n"], c["spec"]["f"]) for c in small} == {(1, 0), (2, 0), (3, 1)}
    for c in small:
        sp, ev = c["spec"], c["result"]["events"]
        first = {}
        for t, node, kp, s in c["result"]["raw_order"]["deliver"]:
            first.setdefault(node, []).append(t)
        ends = sorted(e for e in ev["send"] if e[2] == S.SEND and e[4] == 1)
        if (sp["n"], sp["f"]) == (3, 1):
            # every replica SENDs its phase-2 key at the step of its third delivery, none at its second
            assert len(ends) == 3
            for t, node, _typ, _kp, _s in ends:
                assert first[node][2] == t and first[node][1] <= t, (node, t, first[node])
        else:
            assert not ends and c["result"]["counts"]["decide"] == 0 and c["result"]["status"] == "quiescent"


# ---- the table --------------------------------------------------------------------------------------------------------
GRID = {
    "packed4": {(1, 0), (2, 0), (2, 1), (3, 0), (3, 2), (4, 3)},
    "packed": {(7, 0), (7, 3), (7, 6), (16, 8), (16, 15), (29, 0), (29, 14)},
    "lean": {(40, 0), (40, 14), (40, 20), (64, 32), (64, 63)},
    "general64": {(40, 0), (40, 20)},
    "life": {(40, 0), (40, 39), (64, 32)},
    "life-pl": {(50, 0), (50, 25)},
    "wide": {(70, 0), (70, 24), (70, 35), (130, 65), (130, 129)},
    "wide-life": {(70, 0), (70, 35), (70, 69), (130, 65)},
    "pattern": {(70, 24), (70, 35)},
}
MODES = {
    "packed4": {F.REF, F.SPEC, F.BEB}, "packed": {F.REF, F.SPEC, F.CONN}, "lean": {F.REF, F.SPEC, F.BEB},
    "general64": {F.XREF, F.CONN}, "life": {F.REF, F.SPEC, F.BEB, F.CONN}, "life-pl": {F.SPEC, F.CONN},
    "wide": {F.REF, F.SPEC, F.BEB}, "wide-life": {F.REF, F.SPEC, F.BEB}, "pattern": {F.REF},
}


def test_table_holds_the_grid():
    for fam, shapes in GRID.items():
        mine = [c for c in CASES if c.family == fam]
        assert {(c.n, c.f) for c in mine} >= shapes, (fam, shapes - {(c.n, c.f) for c in mine})
        assert {c.mode for c in mine} == MODES[fam], fam
    assert any(not c.consensus for c in CASES if c.family == "packed4")
    assert [c.kind for c in CASES if c.family == "wide"].count("records") == 1
    assert all(c.masks for c in CASES if c.family in ("life", "pattern") or (c.family == "packed" and not c.overflow))
    assert sorted(c.family for c in CASES if c.overflow) == ["lean", "packed", "wide"]
    assert all(c.specs[0]["delay_model"] == F.UNIF and c.dmax == 12 for c in CASES if c.family == "life-pl" and c.mode == F.SPEC)
    # (connection peers under uniform delays up to 12 stall before any quorum, whatever f: geometric delays there)
    assert all(c.dmax == 12 and c.specs[0]["delay_model"] in (F.UNIF, F.GEO) for c in CASES if c.family == "life-pl")
    assert all(c.dmax <= 8 for c in CASES if c.family != "life-pl")
    assert all(1 <= c.round_cap <= 3 and 16 <= c.count <= 64 and c.specs[0]["step_cap"] <= 400 for c in CASES)
    assert all([sp["g"] for sp in c.specs] == list(range(777, 777 + c.count)) for c in CASES)
    assert F.SLICED["packed"] in NAMES and F.by_name()[F.SLICED["wide"]].n > 64


@pytest.mark.parametrize("name", NAMES)
def test_case_lands_on_its_family_and_its_masks_differ(name):
    c = F.by_name()[name]
    npad = F.T.pick_npad(c.n)
    fam = {"packed4": npad == 4 and c.inst[0] == "step", "packed": 8 <= npad <= 32 and c.inst[0] == "step",
           "lean": npad == 64 and c.inst[:2] == ("step", 64) and c.inst[3] in (F.REF, F.SPEC, F.BEB),
           "general64": npad == 64 and c.inst[0] == "step" and c.inst[3] in (F.XREF, F.CONN),
           "life": c.inst[0] == "life" and npad == 64 and c.model in (F.CONST, F.SLOW) and c.dmax <= 8,
           "life-pl": c.inst[0] == "life" and npad == 64 and c.model in (F.UNIF, F.GEO),
           "wide": c.inst[0] == "wide", "wide-life": c.inst[0] == "wide_life" and c.n > 64 and c.model in (F.CONST, F.SLOW),
           "pattern": c.inst[0] == "pattern" and c.n > 64 and c.nv == 2}
    assert fam[c.family], (name, c.inst)
    assert all(F.T.instantiation(sp, c.q) == F.T.instantiation(c.specs[0], c.q) for sp in c.specs)
    if c.masks:
        ipw = max(1, 64 // npad)
        assert [sp["byzantine"] for sp in c.specs] == c.masks and c.cfg_byz and c.cfg_byz not in c.masks
        for a in range(0, c.count, ipw):
            item = [tuple(m) for m in c.masks[a:a + ipw]]
            assert len(item) < 2 or len(set(item)) >= 2, (name, a)
        assert len({tuple(m) for m in c.masks}) >= 4
    else:
        assert all(sp["byzantine"] == [] for sp in c.specs)


@pytest.mark.parametrize("name", NAMES)
def test_slow_set_sizes(name):
    """f = 0: no slow replica; f = n - 1: exactly one fast replica, in every instance -- and where the masks say so,
    that replica is the Byzantine one."""
    c = F.by_name()[name]
    sp0 = c.specs[0]
    sch = Schedule(c.n, c.f, sp0["seed"], sp0["delay_model"], sp0["dmax"], sp0.get("dconst", 1))
    hit = 0
    for sp in c.specs:
        slow = [x for x in range(c.n) if sch.is_slow(sp["g"], x)]
        assert len(slow) == c.f
        if c.f == c.n - 1:
            fast = [x for x in range(c.n) if x not in slow]
            assert len(fast) == 1 and fast[0] == F.fast_replica(c.n, sp0["seed"], c.model, c.dmax, sp["g"])
            hit += sp["byzantine"] == fast
    if c.f == c.n - 1 and c.masks and c.n > 1:
        assert hit >= c.count // 3, (name, hit)


def _phase_ends(exp, byz):
    """SENDs of keys with a phase index above 0 by honest replicas: each is one phase end."""
    return [e for e in exp["events"]["send"] if e[2] == S.SEND and e[4] >= 1 and e[1] not in byz]


@pytest.mark.parametrize("name", NAMES)
def test_case_does_real_work_and_its_regime_is_real(name):
    c = F.by_name()[name]
    res = F.oracle_results(c)
    assert sorted(res) == c.oracle_ids() and (c.n > 64 or len(res) == c.count)
    ends = 0
    for i, (exp, dec, delivers) in res.items():
        assert exp["arrivals"] > 0 and exp["cell_steps"] > 0, (name, i)
        assert exp["status"] in ("done", "quiescent", "stepcap"), (name, i, exp["status"])
        assert not any(d in dec for d in c.byz(i)), (name, i)
        if c.unreachable(i):
            assert delivers == 0 and not dec and exp["status"] == "quiescent", (name, i, delivers)
        elif c.kind != "pattern":
            assert delivers > 0, (name, i)
        ends += bool(_phase_ends(exp, c.byz(i)))
        if c.stalls():
            assert not _phase_ends(exp, c.byz(i)) and not dec and exp["status"] == "quiescent", (name, i)
    if c.consensus and not c.stalls() and not all(c.unreachable(i) for i in res):
        assert ends > 0, (name, "no compared instance ends a phase")
    if c.second():
        # every honest replica that ends its first phase does so at the step of its second delivery
        seen = 0
        for i, (exp, _dec, _d) in res.items():
            per = {}
            for t, node, _kp, _s in exp["events"]["deliver"]:
                per.setdefault(node, []).append(t)
            for t, node, _typ, _kp, s in _phase_ends(exp, c.byz(i)):
                if s == 1:
                    assert sorted(per[node])[1] == t, (name, i, node, t, sorted(per[node])[:3])
                    seen += 1
        assert seen > 0, name
    # the key window: what the oracle's send log needs (the engine's BRC_OVERFLOW is not the oracle's under REF / BEB)
    need = max(W.needs(exp, c.dmax) for (exp, _dec, _d) in res.values())
    if c.overflow:
        assert need > c.q and c.mode == F.REF and c.inst[0] in ("step", "wide"), (name, need)
    else:
        assert need <= c.q, (name, need, c.q)
    if c.mode == F.SPEC:
        assert not any(exp["status"] == "overflow" for (exp, _dec, _d) in res.values())


def test_the_regimes_occur():
    assert sum(all(c.unreachable(i) for i in range(c.count)) for c in CASES) >= 10
    assert {c.mode for c in CASES if c.second()} == {F.SPEC, F.BEB}
    assert {c.family for c in CASES if c.stalls()} >= {"packed4", "packed", "lean", "general64", "life"}
    assert {c.family for c in CASES if c.f == 0} == set(GRID) - {"pattern"}
    assert {c.family for c in CASES if c.f == c.n - 1 and c.n > 1} >= {"packed4", "packed", "lean", "life", "wide", "wide-life"}


@pytest.mark.parametrize("name", [c.name for c in CASES if c.f != F.standard(c.n)])
def test_f_matters(name):
    """Under f = (n - 1) // 3 at least half of the instances give another result (any counter, the delivery count,
    any decide event): a kernel that clamps f to the standard bound, or reads it from a narrower field that holds the
    standard bound, cannot pass the bit-exact comparison."""
    c = F.by_name()[name]
    mine, std = F.all_summaries(c), F.all_summaries(c, std=True)
    changed = sum(a != b for a, b in zip(mine, std))
    assert 2 * changed >= c.count, (name, changed, c.count)


def test_standard_bound_committees_of_one_and_two_by_hand():
    """n <= 2 at f = 0 IS the standard bound: the exact result, by hand, as the reference fixture has it.  n = 1:
    SEND, ECHO and READY to itself, one delivery per key, and the consensus count (1) never exceeds n - f = 1.
    n = 2: per key 2 SENDs, 4 ECHOs, 4 READYs; both replicas deliver both keys, and the count (2) never exceeds 2."""
    by = F.by_name()
    fx = {(c["spec"]["n"], c["spec"]["mode"]): c["result"] for c in FIXTURE if c["spec"]["n"] <= 2 and c["spec"]["f"] == 0}
    for name, key, msgs, delivers in (("p4-n1f0-ref", (1, "consensus"), 3, 1), ("p4-n2f0-ref", (2, "consensus"), 20, 4)):
        c = by[name]
        assert c.f == F.standard(c.n) == 0
        want = fx[key]
        assert (want["msgs_sent"], want["arrivals"], want["counts"]["deliver"], want["counts"]["decide"]) == (msgs, msgs, delivers, 0)
        for i, (exp, dec, n_del) in F.oracle_results(c).items():
            assert (exp["status"], exp["msgs_sent"], exp["arrivals"], n_del, dec) == ("quiescent", msgs, msgs, delivers, {}), (name, i)
            assert [e[2:] for e in exp["events"]["deliver"]] == [[kp, 0] for _node in range(c.n) for kp in range(c.n)]
    c = by["p4-n1f0-brb"]
    assert fx[(1, "brb")]["msgs_sent"] == 3 and fx[(1, "brb")]["counts"]["deliver"] == 1
    for i, (exp, _dec, n_del) in F.oracle_results(c).items():
        sends = [a for a in c.specs[i]["actions"] if a["kind"] == "brb_send"]
        assert len(sends) == 1 and (exp["msgs_sent"], exp["arrivals"], n_del) == (3, 3, 1), (i, exp["msgs_sent"])
        # SEND, ECHO, READY one link delay apart: the delivery three delays after the SEND
        d = Schedule(1, 0, c.specs[i]["seed"], c.model, c.dmax).delay(c.specs[i]["g"], 0, 0)
        assert exp["events"]["deliver"] == [[sends[0]["t"] + 3 * d, 0, 0, 0]], (i, exp["events"]["deliver"])
