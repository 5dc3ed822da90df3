"""Preconditions of tests/test_gpu_step_noevent.py, checked without a GPU: the table of
tests/step_noevent_workloads.py names every compiled EV = false step-kernel instantiation or lists it as
unreachable, and on the C oracle alone every compared id of every case ends done or quiescent with work
done, every consensus case has an instance whose honest replicas all decide, and every non-constant case
sees at least two distinct link delays -- so no GPU run is spent on a workload that does nothing.  The
oracle's results are the ones the GPU test compares with (one cache, step_noevent_workloads.oracle_results)."""
import pytest

from tests import step_noevent_workloads as T

CASES = T.cases()


def test_table_names_every_instantiation():
    full = T.full_set()
    assert len(full) == 108
    named = {c.inst for c in CASES}
    assert not named & set(T.UNREACHABLE)
    assert named | set(T.UNREACHABLE) == full
    by_family = {}
    for inst in full:
        by_family.setdefault((inst[0], inst[3] == T.XREF, inst[4]), set()).add(inst)
    assert {k: len(v) for k, v in by_family.items()} == {
        ("step", False, 0): 60, ("step", True, 0): 3, ("step", False, 2): 9, ("wide", False, 0): 24, ("wide", False, 4): 12}


def test_every_case_lands_on_the_instantiation_it_names():
    for c in CASES:
        sp = c.specs[0]
        assert T.instantiation(sp, c.key_window) == c.inst, c.name
        assert [s["g"] for s in c.specs] == list(range(T.OFFSET, T.OFFSET + c.count)), c.name
        npad = c.inst[1]
        assert c.count == (3 * (64 // npad) + 1 if npad < 64 else 5 if npad == 64 else 3), c.name
        assert npad // 2 < sp["n"] <= npad or sp["n"] == 3, c.name
        assert {4: sp["dmax"] <= 4, 8: 5 <= sp["dmax"] <= 8, 16: 9 <= sp["dmax"]}[c.inst[2]], c.name


def test_unreachable_instantiations_follow_from_the_wv4_rule():
    """brc_create's wide_wv4 wants an LDS carve of at most 40 KB: at NPAD = 256 REFERENCE and BEB (the same
    carve) never get there, SPEC does (cfg5's constant-delay leg)."""
    assert T.min_lds_wide_256(spec=False) == 44784 > 40 * 1024
    assert T.min_lds_wide_256(spec=True) <= 40 * 1024
    assert set(T.UNREACHABLE) == {("wide", 256, dm, m, 4) for dm in (4, 8) for m in (T.REF, T.BEB)}


def test_table_has_the_content_the_gpu_test_relies_on():
    names = [c.name for c in CASES]
    for kernel, packed in (("step", True), ("step", False), ("wide", False)):
        fam = [c for c in CASES if c.inst[0] == kernel and (c.inst[1] < 64) == packed]
        assert any(c.specs[0]["byzantine"] for c in fam), (kernel, packed)
        assert any(c.run["proposals"] == "loaded" for c in fam), (kernel, packed)
        assert any(c.specs[0]["n"] == c.inst[1] for c in fam) and any(c.specs[0]["n"] < c.inst[1] for c in fam)
    assert "n16-dm4-ref-equivocate" in names and "n16-dm4-spec-equivocate" in names
    brb = [c for c in CASES if not c.consensus]
    assert {(c.inst[1], c.inst[3]) for c in brb} == {(p, m) for p in (128, 256) for m in (T.REF, T.SPEC, T.BEB, T.CONN)}
    assert all(c.specs[0]["n"] == c.inst[1] for c in brb)
    assert all(c.specs[0]["n"] == 40 and c.specs[0]["values"] == T.S.VALUES8 for c in CASES if c.inst[3] == T.XREF)


def test_traced_kernel_names_are_the_tables():
    """profiles/r8/step_noevent_kernels.txt: the distinct step-kernel names of one rocprofv3 --kernel-trace run
    of tests/test_gpu_step_noevent.py.  Its EV = false names are exactly the instantiations the table claims to
    launch, every one with an EV = true twin also ran it (the WV = 4 kernels have none), and the key-lifetime
    kernel ran nothing (the BRC_KERNEL=step cases stayed on the step kernel)."""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "r8", "step_noevent_kernels.txt")
    with open(path) as fh:
        lines = [ln.strip() for ln in fh if ln.strip()]
    assert lines == sorted(set(lines)) and not any("life" in ln for ln in lines)
    seen = {False: set(), True: set()}
    for ln in lines:
        m = re.fullmatch(r"brc::brc_step(_wide)?<(\d+), (\d+), (true|false), (\d), (\d)>", ln)
        assert m, ln
        seen[m.group(4) == "true"].add(("wide" if m.group(1) else "step", int(m.group(2)), int(m.group(3)),
                                        int(m.group(5)), int(m.group(6))))
    named = {c.inst for c in CASES}
    assert seen[False] == named, (sorted(seen[False] - named), sorted(named - seen[False]))
    assert seen[True] == {i for i in named if i[4] != 4}


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_case_preconditions(name):
    c = T.by_name()[name]
    byz = set(c.specs[0]["byzantine"])
    honest = [d for d in range(c.specs[0]["n"]) if d not in byz]
    res = T.oracle_results(c)
    assert len(res) == (c.count if c.specs[0]["n"] <= 32 else 3)
    all_decided = delivered = 0
    for i, (exp, dec, delivers) in res.items():
        want = ("overflow",) if name.endswith("-ovf") else ("done", "quiescent")
        assert exp["status"] in want, (name, i, exp["status"])
        assert exp["cell_steps"] > 0, (name, i)
        delivered += delivers > 0
        assert not any(d in dec for d in byz), (name, i)
        all_decided += all(d in dec for d in honest)
    assert delivered > 0, (name, "no compared instance delivers anything")
    if c.consensus:
        assert all_decided > 0, (name, "no compared instance decides at every honest replica")
    if not c.constant:
        assert len(T.link_delays(c)) >= 2, name
