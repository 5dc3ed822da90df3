"""Preconditions of tests/test_gpu_interleaved.py, checked without a GPU on the C oracle alone: the table of
tests/interleaved_workloads.py names every kernel family and lands on the instantiation it claims; its action
lists hold what the GPU test relies on; every at_now time is a step at which the instance has arrivals; every
after_quiet boundary falls after the oracle's run of the groups before it went quiet (and that run is a prefix of
the full one), with a sibling of the wave item still active in packed cases; no instance stops with actions still
to come; and the pruning workload never has more than XSEND_MAX extra SENDs within delay_max steps of each other."""
import pytest

from tests import engine_runner as R
from tests import interleaved_workloads as W
from tests import step_noevent_workloads as T

CASES = W.cases()


def test_table_names_every_family():
    assert [c.family for c in CASES] == list(W.FAMILIES)
    want = {"packed4": ("step", 4), "packed8": ("step", 8), "packed16": ("step", 16), "packed32": ("step", 32),
            "wide128": ("wide", 128), "wide256": ("wide", 256)}
    for c in CASES:
        sp = c.specs[0]
        assert T.instantiation(sp, c.key_window) == c.inst, c.name
        assert 2 <= c.count <= 8 and [s["g"] for s in c.specs] == list(range(W.OFFSET, W.OFFSET + c.count)), c.name
        assert all(R._cfg_key(s) == R._cfg_key(sp) for s in c.specs), c.name
        assert all(s["step_cap"] == W.STEP_CAP for s in c.specs) and list(sp["byzantine"]) == c.byz, c.name
        assert c.consensus == (sp["mode"] in ("consensus", "spec", "beb_consensus")), c.name
        assert c.packed == (c.inst[1] < 64), c.name
        if c.family in want:
            assert c.inst[:2] == want[c.family], c.name
    fam = {c.family: c for c in CASES}
    for mode, name in ((W.REF, "ref"), (W.SPEC, "spec"), (W.BEB, "beb")):
        assert fam["lean64r-" + name].inst == ("step", 64, 8, mode, 2)           # the register-mask build
        assert fam["lean64-" + name].inst[:2] + fam["lean64-" + name].inst[3:] == ("step", 64, mode, 0)
        assert not fam["lean64-" + name].specs[0].get("general_keys")
    assert fam["general64"].inst[3] == W.XREF and fam["conn64"].inst[3] == W.CONN and fam["conn64"].inst[1] == 64
    # every policy runs on every kind of kernel: packed, lean, tagged NPAD 64, wide
    for pol in ("at_now", "after_quiet"):
        have = {c.family for c in CASES if pol in c.policies()}
        assert have & {"packed4", "packed8", "packed16", "packed32"} and have & {"wide128", "wide256"}, pol
        assert have & {"lean64r-ref", "lean64r-spec", "lean64r-beb"} or pol == "after_quiet"
        assert have & {"lean64-ref", "lean64-spec", "lean64-beb"} and have & {"general64", "conn64"}, pol
    assert all("at_now" in c.policies() for c in CASES if c.family.startswith("lean64"))


def test_packed_items_carry_different_action_lists():
    for c in CASES:
        if not c.packed:
            continue
        ipw = 64 // c.inst[1]
        first = [R._injections(sp, 0) for sp in c.specs[:ipw]]
        assert len(first) >= 2 and any(a != first[0] for a in first[1:]), c.name


def _content(c):
    """The CONTENT labels the case's expanded action lists hold."""
    have = set()
    n, q = c.specs[0]["n"], c.key_window
    three_bit = (n <= 32 or c.inst[3] in (W.CONN, W.XREF)) and c.inst[3] != W.SPEC
    for i, sp in enumerate(c.specs):
        recs = R._injections(sp, i)
        kinds = {}
        for r in recs:
            kinds.setdefault(r["kind"], []).append(r)
        if len({r["t"] for r in kinds.get(R.L.INJ_PROPOSE, [])}) >= 3:
            have.add("staggered-propose")
        if any(r["s"] >= q for r in kinds.get(R.L.INJ_SEND, [])):
            have.add("wrapping-stream")
        if kinds.get(R.L.INJ_KEY) and kinds.get(R.L.INJ_MSG):
            have.add("byz-key-msg")
        if kinds.get(R.L.INJ_DELIVER):
            assert c.inst[3] in (W.REF, W.BEB), c.name
            have.add("deliver")
        allm = (1 << n) - 1
        for r in kinds.get(R.L.INJ_SEND, []):
            if r["dst"] != allm:
                have.add("restricted-send")
                if n > 64 and (r["dst"] >> 64) not in (0, allm >> 64):
                    have.add("restricted-hi")
        keys = [(r["kp"], r["s"]) for r in kinds.get(R.L.INJ_SEND, [])]
        if len(keys) != len(set(keys)):
            assert three_bit, (c.name, "an extra SEND on a kernel that keeps one SEND per key")
            have.add("extra-send")
        times = [r["t"] for r in recs]
        if max(times.count(t) for t in set(times)) > W.INJ_CACHE and c.inst[1] < 64:
            have.add("over-inj-cache")
    return have


def test_action_lists_hold_the_content():
    have = set()
    for c in CASES:
        have |= _content(c)
    assert have == set(W.CONTENT), sorted(set(W.CONTENT) - have)
    # a piece that lands while earlier records of the same item are uploaded and unconsumed: an at_now time with
    # a later unmarked action of the same instance (lookahead(1) has uploaded it before the instance gets there)
    for c in CASES:
        for i, ts in c.marks.items():
            (t,) = ts
            later = [a for a in c.specs[i]["actions"] if a["t"] > t]
            if later:
                break
        else:
            continue
        break
    else:
        raise AssertionError("no at_now action lands before an uploaded, unconsumed record")


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_case_preconditions(name):
    from oracle import oracle
    c = W.by_name()[name]
    res = W.oracle_results(c)
    dmax = c.specs[0]["dmax"]
    for i, (exp, _dec, delivers) in res.items():
        assert exp["status"] in ("done", "quiescent"), (name, i, exp["status"])       # no RUNNING, OVERFLOW, STEPCAP
        assert exp["cell_steps"] > 0, (name, i)
        last = max(a["t"] for a in c.specs[i]["actions"])
        assert last <= exp["t_stop"], (name, i, "stops at", exp["t_stop"], "with an action at", last)
    assert sum(r[2] > 0 for r in res.values()) * 2 >= c.count, (name, "most instances deliver something")
    print(name, c.inst, "t_stop", [r[0]["t_stop"] for r in res.values()], "marks", c.marks, "bounds", c.bounds)
    # at_now: the step of an honest ECHO / READY / deliver event of that instance
    for i, ts in c.marks.items():
        exp = res[i][0]
        for t in ts:
            steps = {e[0] for e in exp["events"]["send"] if e[2] in (2, 3) and e[1] not in c.byz} | \
                    {e[0] for e in exp["events"]["deliver"] if e[1] not in c.byz}
            assert t in steps and t >= c.late_lo > 0, (name, i, t)
            assert any(a["t"] == t for a in c.specs[i]["actions"]), (name, i, t)
    # after_quiet: the prefix goes quiet before the next group, and the full run continues it
    ipw = 64 // c.inst[1] if c.packed else 1
    for i, bs in c.bounds.items():
        full = res[i][0]
        for j, g in enumerate(bs):
            pre = oracle.run(c.prefix_spec(i, j))
            assert pre["status"] == "quiescent" and pre["t_stop"] + dmax < g, (name, i, j, pre["status"], pre["t_stop"], g)
            for k in ("deliver", "decide", "send"):
                got = sorted(map(list, pre["events"][k]), key=str)
                want = sorted([list(e) for e in full["events"][k] if e[0] < g], key=str)
                assert got == want, (name, i, j, k, len(got), len(want))
            assert any(a["t"] >= g for a in c.specs[i]["actions"]) and full["t_stop"] >= g, (name, i, j)
            if c.packed:
                sib = [s for s in range(i - i % ipw, min(i - i % ipw + ipw, c.count)) if s != i]
                assert any(res[s][0]["t_stop"] > pre["t_stop"] + 2 * dmax for s in sib), (name, i, j, "no sibling is active then")
    assert max(r[0]["t_stop"] for r in res.values()) <= 400, name          # run(1) loops are launch-bound


def test_pruning_workload():
    from oracle import oracle
    sp = W.pruning_spec()
    recs = R._injections(sp, 0)
    seen, extra = set(), []
    for r in recs:
        assert r["kind"] == R.L.INJ_SEND
        if (r["kp"], r["s"]) in seen:
            extra.append(r["t"])
        seen.add((r["kp"], r["s"]))
    assert len(extra) > W.XSEND_MAX
    assert max(sum(abs(a - b) <= sp["dmax"] for b in extra) for a in extra) <= W.XSEND_MAX // 2
    exp = oracle.run(sp)
    assert exp["status"] == "quiescent" and exp["counts"]["deliver"] > 0 and exp["t_stop"] >= extra[-1]
