"""Preconditions of tests/key_layout_workloads.py, on the oracle alone: every case is a configuration brc_create
accepts (the restated rules), the table reaches every (family, NV, Q extreme) cell of the grid, no compared instance
overflows or runs into the step cap, the variant slots v >= 1 carry arrivals, the two splits differ, one case per
family that takes injections has a Byzantine origin's key delivered by every honest replica, and the oracle equals
the independent Python model (tests/spec_model.py) on the SPEC and BEB-broadcast cases."""
import pytest

from oracle import oracle
from tests import golden_io, spec_model
from tests import key_layout_workloads as K
from tests.golden import specs as S

CASES = K.cases()
REF, SPEC, BEB, CONN, XREF = K.REF, K.SPEC, K.BEB, K.CONN, K.XREF


def _kernel_env(case):
    return case.kernel if 33 <= case.specs[0]["n"] <= 64 else "auto"


def test_even_split_of_two_variants_is_the_equivocation_pattern():
    for n, byz in ((16, list(range(11, 16))), (7, [6]), (70, [1, 64, 69]), (130, [0, 129])):
        assert S.variant_actions(n, byz, 2, "even") == S.equivocation_actions(n, byz)
    acts = S.variant_actions(16, [3, 15], 4, "skewed")
    for b in (3, 15):
        dst = [a["dst"] for a in acts if a["kind"] == "byz" and a["type"] == S.SEND and a["src"] == b]
        assert len(dst) == 4 and sum(dst) == (1 << 16) - 1 and all(x & y == 0 for i, x in enumerate(dst) for y in dst[:i])
        assert [bin(d).count("1") for d in dst] == [13, 1, 1, 1] and not any(d >> b & 1 for b in (3, 15) for d in dst[1:])
    assert sorted({a["value"] for a in acts if a["kind"] == "byz_key"}) == [0, 1, 2, 3]


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_case_is_accepted_and_named_right(name):
    case = K.by_name()[name]
    sp = case.specs[0]
    kw = dict(kernel=_kernel_env(case), proposals=case.run["proposals"], byz_pattern=case.run.get("byz_pattern", False))
    assert K.accepted(sp, case.q, events=False, **kw) == case.kernel, name
    if case.kernel == "step":
        assert K.accepted(sp, case.q, events=True, **kw) == "step", name       # the event-log twin
        assert case.inst == K.T.instantiation(sp, case.q)[:4] + (case.inst[4],)
    assert sp.get("nv", 1) == case.nv and case.key_window == case.q
    assert all(s["g"] == K.OFFSET + i for i, s in enumerate(case.specs)) and K.OFFSET > 0
    npad = K.T.pick_npad(sp["n"])
    fam = {"packed": npad <= 16, "lean": npad == 64 and case.inst[3] in (REF, SPEC, BEB) and case.inst[0] == "step",
           "general64": npad == 64 and case.inst[3] in (XREF, CONN), "wide": case.inst[0] == "wide",
           "life": case.inst[0] == "life", "pattern": case.run.get("byz_pattern", False)}
    assert fam[case.family], (name, case.inst)
    assert case.count == (3 * (64 // npad) + 1 if npad < 64 else 5 if npad == 64 else case.count) and 2 <= case.count <= 25
    if "twoclass" in case.tags and case.family == "lean":
        assert case.inst[4] == 2
    if "perlink" in case.tags and case.family == "lean":
        assert case.inst[4] == 0


def test_refusals_restated():
    """The rules of brc_create the issue names (tests/test_gpu_key_layout.py holds the engine to them)."""
    spec16 = dict(n=16, mode="spec", delay_model=K.SLOW, dmax=4)
    assert K.accepted(dict(spec16, nv=4), 4) is None and K.accepted(dict(spec16, nv=4), 2) == "step"
    assert K.accepted(dict(spec16, n=70, nv=2), 2) is None and K.accepted(dict(spec16, n=70, nv=1), 2) == "step"
    ref70 = dict(n=70, mode="consensus", delay_model=K.SLOW, dmax=4)
    assert K.accepted(dict(ref70, nv=4), 4) is None and K.accepted(dict(ref70, nv=2), 8) is None
    assert K.accepted(dict(ref70, nv=4), 2) == "step"


def test_table_reaches_the_grid():
    have = {(c.family, c.inst[3] if c.family != "life" else c.mode, t) for c in CASES for t in c.tags}
    shapes = {(c.family, c.specs[0]["n"]) for c in CASES}
    want = []
    for mode in (REF, SPEC, BEB, CONN):
        want += [("packed", mode, t) for t in ("nv4-q2", "nv4-qmax", "nv2-qmax", "nv1-q2")]
    for mode in (REF, SPEC, BEB):
        want += [("lean", mode, t) for t in ("nv4-q2", "q4v2", "q2v2", "twoclass", "perlink")]
    want += [("lean", m, t) for m in (REF, BEB) for t in ("nv4-qmax", "nv2-qmax")]
    want += [("general64", m, t) for m in (XREF, CONN) for t in ("nv4-q2", "nv4-qmax")]
    want += [("wide", m, t) for m in (REF, BEB, CONN) for t in ("nv4-q2", "q2v2", "q4v2")]
    want += [("wide", SPEC, "spec-q2v1"), ("wide", REF, "records")]
    want += [("life", m, "nv4-q%d" % q) for m in (REF, CONN) for q in (2, 16, 32)]
    want += [("life", m, t) for m in (REF, CONN, SPEC) for t in ("twoclass", "perlink")] + [("life", SPEC, "nv4-q2")]
    missing = [w for w in want if w not in have and w not in K.UNREACHABLE]
    assert not missing, missing
    assert not [u for u in K.UNREACHABLE if u in have], "a cell listed as unreachable is reached"
    assert shapes >= {("packed", 7), ("packed", 16), ("lean", 40), ("lean", 64), ("wide", 70), ("wide", 130),
                      ("pattern", 16), ("pattern", 40), ("pattern", 70)}
    # the Q extremes are brc_create's: the next window up is refused, per family and NV
    for c in CASES:
        if {"nv4-qmax", "nv2-qmax"} & c.tags:
            kw = dict(kernel="step", events=True, proposals=c.run["proposals"])
            assert K.accepted(c.specs[0], c.q, **kw) == "step" and K.accepted(c.specs[0], 2 * c.q, **kw) is None, c.name
    # Q * NV = 128 on the lifetime kernel: the HBM slot metadata, and no whole origin in a 64-slot word
    big = [c for c in CASES if c.family == "life" and c.q * c.nv == 128]
    assert {c.mode for c in big} == {REF, CONN} and all(c.specs[0]["delay_model"] in (K.CONST, K.SLOW) for c in big)
    assert any(c.specs[0].get("wide_records") for c in CASES)


def _light(sp):
    return oracle.run(sp, light=True)


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_oracle_runs_the_case_and_the_variants_work(name):
    case = K.by_name()[name]
    ids = case.oracle_ids()
    K.oracle_events(case)
    res = K.T.oracle_results(case)
    spec_mode = case.specs[0]["mode"] == "spec"
    for i in ids:
        exp = res[i][0]
        assert exp["status"] in ("done", "quiescent"), (name, i, exp["status"])
        assert not spec_mode or exp["status"] == "done", (name, i, exp["status"])
        assert exp["t_stop"] < case.specs[i]["step_cap"]
    if not case.split:
        return
    sp = case.specs[0]
    nv = case.nv
    # the variants v >= 1 carry arrivals: without their actions the run has fewer
    without = dict(sp, actions=[a for a in sp["actions"] if a["kind"] not in ("byz", "byz_key") or a["kp"] % nv == 0])
    assert _light(without)["arrivals"] < res[0][0]["arrivals"], name
    if case.split == "pattern":
        return
    other = case.other_split().specs[0]
    a, b = oracle.run(other), res[0][0]
    a["events"] = golden_io.canonical_events(a["events"])
    same = [k for k in ("arrivals", "msgs_sent", "cell_steps") if a[k] == b[k]] + \
        [k for k in ("deliver", "decide", "send") if a["events"][k] == K.oracle_events(case)[0][k]]
    print(name, "equal between the splits:", same)
    assert len(same) < 6, name


def _fully_delivered(case):
    """Instances (of the compared ids) in which some Byzantine origin's key is delivered by every honest replica."""
    sp = case.specs[0]
    byz = set(sp["byzantine"])
    honest = sp["n"] - len(byz)
    out = []
    for i, ev in K.oracle_events(case).items():
        per = {}
        for (_t, node, kp, s) in ev["deliver"]:
            if kp // case.nv in byz and node not in byz:
                per[(kp, s)] = per.get((kp, s), 0) + 1
        if any(v == honest for v in per.values()):
            out.append(i)
    return out


@pytest.mark.parametrize("family", ["packed", "lean", "general64", "wide"])
def test_a_byzantine_key_is_delivered_by_every_honest_replica(family):
    found = [c.name for c in CASES if c.family == family and c.split == "skewed" and _fully_delivered(c)]
    print(family, found)
    assert found, family


SPEC_OR_BEB = [c.name for c in CASES if c.specs[0]["mode"] in ("spec", "spec_brb", "beb")]


@pytest.mark.parametrize("name", SPEC_OR_BEB)
def test_oracle_equals_the_python_model(name):
    case = K.by_name()[name]
    i = case.oracle_ids()[-1]
    sp = case.specs[i]
    exp = spec_model.run(sp)
    K.oracle_events(case)
    got = K.T.oracle_results(case)[i][0]
    for k in ("status", "t_stop", "msgs_sent", "arrivals"):
        assert got[k] == exp[k], (name, k, got[k], exp[k])
    a, b = golden_io.canonical_events(got["events"]), golden_io.canonical_events(exp["events"])
    for k in ("deliver", "decide", "send"):
        assert a[k] == b[k], (name, k)
