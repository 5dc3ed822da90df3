"""CPU only, the oracle alone: the preconditions of tests/time_axis_workloads.py -- what keeps a case of
tests/test_gpu_time_axis.py from testing nothing."""
import pytest

from tests import time_axis_workloads as W

CASES = W.cases()
NAMES = [c.name for c in CASES]
STEP = [c.name for c in W.step_cases()]


def _statuses(specs):
    return [W._light(sp) for sp in specs]


def test_table_covers_every_family():
    fams = {c.family for c in CASES}
    assert fams == {"packed4", "packed8", "packed16", "packed32", "lean64r-ref", "lean64r-spec", "lean64-ref", "lean64-spec",
                    "general64", "conn8", "conn64", "wide128", "wide256", "wide128-records", "wide128-values", "life"}
    from tests import step_noevent_workloads as T
    by = W.by_name()
    # the step-kernel instantiation brc_create picks (step_noevent_workloads.instantiation restates its rules)
    want = {"p4-ref-cons": ("step", 4), "p8-spec-brb": ("step", 8), "p16-ref-byz": ("step", 16), "p32-beb-cons": ("step", 32),
            "n40r-ref-cons": ("step", 64, T.REF, 2), "n40r-spec-cons": ("step", 64, T.SPEC, 2), "n64-ref-brb": ("step", 64, T.REF, 0),
            "n64-spec-brb": ("step", 64, T.SPEC, 0), "n40-xref-brb": ("step", 64, T.XREF, 0), "n6-conn-cons": ("step", 8, T.CONN, 0),
            "n40-conn-brb": ("step", 64, T.CONN, 0), "w128-ref-cons": ("wide", 128, T.REF), "w128-spec-cons": ("wide", 128, T.SPEC),
            "w256-ref-brb": ("wide", 256, T.REF), "w128-rec-brb": ("wide", 128, T.REF), "w128-val-cons": ("wide", 128, T.REF)}
    for name, w in want.items():
        inst = T.instantiation(by[name].specs[0], by[name].key_window)
        got = (inst[0], inst[1]) + ((inst[3],) if len(w) > 2 else ()) + ((inst[4],) if len(w) > 3 else ())
        assert got == w, (name, inst)
    for c in CASES:
        assert c.count <= (3 if c.specs[0]["n"] > 64 else 8)
        assert [sp["g"] for sp in c.specs] == list(range(W.OFFSET, W.OFFSET + c.count))
        assert sorted(c.byz) == sorted(c.specs[0]["byzantine"])
        assert all(a["t"] == 0 and a["kind"] == "propose" for sp in c.specs for a in sp["actions"]) or not c.life
    assert set(W.SLICED) | set(W.LATE_EXTRA) | set(W.LATE_INTERLEAVED) <= set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_caps_stop_some_instance_below_t_last(name):
    case = W.by_name()[name]
    caps, ref, t_last = W.caps(case)
    assert set(caps) == {"zero", "one", "mid", "last-1", "last"} | ({"gap"} if case.gap else set()), (name, caps)
    uncapped = _statuses(case.specs)
    for lab, c in caps.items():
        runs = _statuses(W.capped_specs(case, c))
        if lab == "last":
            assert [(r["status"], r["t_stop"]) for r in runs] == [(r["status"], r["t_stop"]) for r in uncapped], (name, lab)
            assert all(r == u for r, u in zip(runs, uncapped)), (name, lab)
            continue
        assert c < t_last and runs[ref]["status"] == "stepcap", (name, lab, c, runs[ref])
        # truncated counters: a capped run never counts more than the whole one, and the ref run counts less
        assert all(r["msgs_sent"] <= u["msgs_sent"] and r["arrivals"] <= u["arrivals"] and r["t_stop"] <= c for r, u in zip(runs, uncapped))
        assert runs[ref]["arrivals"] < uncapped[ref]["arrivals"], (name, lab)
        if lab == "gap":
            assert 0 < runs[ref]["t_stop"] < c, (name, c, runs[ref])
        if lab == "mid":
            assert runs[ref]["t_stop"] == c and c not in {a["t"] for a in case.specs[ref]["actions"]}, (name, c, runs[ref])
    assert caps["last-1"] == t_last - 1 and caps["last"] == t_last and caps["zero"] == 0 and caps["one"] == 1


def test_per_link_lifetime_case_has_no_gap_step():
    """gap = False is a fact of the schedule, not a choice: no cap below t_last leaves t_stop < cap in any instance."""
    case = W.by_name()["life-perlink"]
    _caps, _ref, t_last = W.caps(case)
    for c in range(1, t_last):
        assert all(r["t_stop"] == c for r in _statuses(W.capped_specs(case, c)) if r["status"] == "stepcap"), c


def test_capped_runs_leave_partially_decided_instances():
    """Some consensus case, at some cap, stops an instance in which some honest replica has decided and another has
    not: round_histogram must put it in hist[0]."""
    hit = []
    for case in CASES:
        if not case.consensus:
            continue
        caps = W.caps(case)[0]
        hon = case.specs[0]["n"] - len(case.byz)
        for lab in ("mid", "last-1"):
            for (exp, dec, _d) in W.oracle_results((case.name, lab), W.capped_specs(case, caps[lab])):
                if exp["status"] == "stepcap" and 0 < len(dec) < hon:
                    hit.append((case.name, lab))
    assert hit, "no capped instance is partially decided"
    print(sorted(set(hit)))


@pytest.mark.parametrize("m", W.mixed(), ids=lambda m: m.name)
def test_mixed_items_end_differently_within_one_item(m):
    n = m.specs[0]["n"]
    npad = 4
    while npad < n:
        npad *= 2
    assert n <= 32 and m.count <= 64 // npad, "one wave item"
    runs = _statuses(m.specs)
    assert {i: r["status"] for i, r in enumerate(runs)} == m.want, runs
    sts = set(m.want.values())
    assert "stepcap" in sts and sts & {"quiescent", "done"}
    if m.name == "p8-ends":
        assert runs[1]["t_stop"] == 0 and runs[1]["msgs_sent"] == 0
        assert runs[0]["t_stop"] < m.cap - 1
        # the action at t == cap is performed and counted; its messages never arrive
        for i in (3, 4):
            before = W._light(dict(m.specs[i], actions=[a for a in m.specs[i]["actions"] if a["t"] < m.cap]))
            assert runs[i]["t_stop"] == m.cap and runs[i]["msgs_sent"] == before["msgs_sent"] + n
            assert runs[i]["arrivals"] == before["arrivals"] and before["status"] == "quiescent"
        assert 10 <= runs[2]["t_stop"] <= m.cap and runs[2]["arrivals"] < W._light(dict(m.specs[2], step_cap=W.RUN_CAP))["arrivals"]
    else:
        assert {i: r["t_stop"] for i, r in enumerate(runs)} == m.t_stop
        a, b = runs
        # A ends before B's action, B's action falls before a bound over all of A's sender's links (10 + 8) and
        # lands past the cap
        assert a["t_stop"] < min(x["t"] for x in m.specs[1]["actions"]) < 10 + 8 and b["arrivals"] == 0 and b["msgs_sent"] == 1
        assert W._light(dict(m.specs[1], step_cap=19))["t_stop"] == 12 and W._light(dict(m.specs[1], step_cap=20))["t_stop"] == 20 > m.cap
        assert W._light(dict(m.specs[0], step_cap=W.RUN_CAP)) == a


def _plus(exp, t0):
    out = dict(exp, t_stop=exp["t_stop"] + t0)
    out["events"] = {k: [[e[0] + t0] + list(e[1:]) for e in v] for k, v in exp["events"].items()}
    return out


@pytest.mark.parametrize("name", STEP)
def test_late_runs_are_translations(name):
    """oracle(shift(sp, T0)) == oracle(sp) with T0 added to t_stop and every event time; the cut run stops by
    STEP_LIMIT; the second burst's reused-slot key is delivered at every honest replica."""
    case = W.by_name()[name]
    t_last = W.caps(case)[2]
    base = W.oracle_results((name, "base"), case.specs)
    late = W.late_specs(case)
    assert ("bursts-59900" in late) == case.brb
    assert set(W.late_t0s(case)) == ({"59900", "x32768", "x128"} if name in W.LATE_EXTRA else {"59900"})
    hon = [d for d in range(case.specs[0]["n"]) if d not in case.byz]
    for lab, (specs, keys) in late.items():
        res = W.oracle_results((name, lab), specs)
        t0 = min(a["t"] for a in specs[0]["actions"]) if keys is None else None
        if lab.startswith("shift"):
            t0 = W.late_t0s(case)[lab[6:]]
            for (exp, _dec, _d), (b, _bd, _b) in zip(res, base):
                assert exp == _plus(b, t0), (name, lab)
            if lab != "shift-59900":
                # the run crosses the power of two
                p = 32768 if lab == "shift-x32768" else 128
                assert t0 < p <= t0 + t_last, (name, lab, t0, t_last)
            else:
                assert t0 + t_last > 59900 and all(sp["step_cap"] == W.STEP_LIMIT for sp in specs)
        elif lab == "cut":
            t0, mid = W.cut_t0(case), W.caps(case)[0]["mid"]
            ref = W.caps(case)[1]
            assert res[ref][0]["status"] == "stepcap" and res[ref][0]["t_stop"] <= W.STEP_LIMIT
            for (exp, _dec, _d), sp in zip(res, case.specs):
                want = W.oracle_run(W.capped(sp, mid))[0]
                assert exp == _plus(want, t0), (name, lab)
        else:
            t0 = W.late_t0s(case)[lab[7:]]
            for i, ((exp, _dec, _d), (o, s)) in enumerate(zip(res, keys)):
                got = sorted(e[1] for e in exp["events"]["deliver"] if e[2:] == [o, s])
                assert got == hon and all(e[0] > t0 for e in exp["events"]["deliver"] if e[2:] == [o, s]), (name, lab, i, got)
                assert exp["status"] == "quiescent" and exp["t_stop"] > t0
                # the same slot as a first-burst key; the first burst is long over
                q = specs[i].get("window") or case.key_window
                assert (o, s - q) in W.first_keys(case.specs[i]) and base[i][0]["t_stop"] < t0
                if case.byz:
                    late_echo = [e for e in exp["events"]["send"] if e[0] == t0 and e[1] == case.byz[0]]
                    assert late_echo or any(a["t"] == t0 and a["kind"] == "byz" for a in specs[i]["actions"])


@pytest.mark.parametrize("name", W.LATE_INTERLEAVED)
def test_at_now_marks_are_steps_with_arrivals(name):
    case = W.by_name()[name]
    marks = W.at_now_marks(case, W.T0)
    assert marks and all(ts == {W.T0 + W.AT_NOW_STEP[name]} for ts in marks.values()), marks
    assert tuple(W.late_t0s(case)) == W.late_t0s_labels(case)
    if case.wide_records:
        n = case.specs[0]["n"]
        assert all(any(a["t"] == W.AT_NOW_STEP[name] and a["kind"] == "byz" and a["dst"] != (1 << n) - 1 for a in case.specs[i]["actions"])
                   for i in marks)
