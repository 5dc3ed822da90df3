"""Preconditions of tests/test_gpu_byz_masks.py, checked without a GPU: the table of tests/byz_mask_workloads.py
meets its mask rules, every case lands on the instantiation it is meant for, does real work on the oracle (some
instance decides; exactly the instances with f silent replicas stall where the protocol makes them), and the
masks matter: for at least half of the instances of every case the oracle's (status, t_stop, msgs_sent, arrivals,
cell_steps) changes when the instance runs under its neighbour's mask -- so a kernel that reads another
instance's mask cannot pass the bit-exact comparison.  Every instance runs on the oracle; the results are the ones
the GPU test compares with."""
import numpy as np
import pytest

from tests import byz_mask_workloads as B
from tests import step_noevent_workloads as T

CASES = B.cases()
NAMES = [c.name for c in CASES]


def test_table_has_the_shapes():
    by = B.by_name()

    def insts(pred):
        return {c.inst for c in CASES if pred(c)}
    plain = lambda c: c.consensus and not c.equivocate and c.kernel == "step" and c.garbage is None  # noqa: E731
    # packed: consensus in REFERENCE and SPEC at every pad, n = 13 and n = 16 at NPAD 16
    assert {(c.mode, c.n, c.f) for c in CASES if plain(c) and c.n <= 32 and c.mode in (B.REF, B.SPEC)} == {
        (m, n, f) for m in (B.REF, B.SPEC) for n, f in ((4, 1), (7, 2), (13, 4), (16, 5), (31, 10))}
    assert {(c.inst[1], c.mode) for c in CASES if plain(c) and c.n <= 32 and c.mode in (B.CONN, B.BEB)} == {
        (16, B.CONN), (16, B.BEB)}
    assert [c.inst[:2] for c in CASES if not c.consensus] == [("step", 8)]
    models = {c.specs[0]["delay_model"] for c in CASES if c.n <= 32}
    assert B.SLOW in models and models & {B.UNIF, B.GEO}
    assert all(c.count == 2 * B.ipw(c.n) + 1 for c in CASES if c.n <= 32 and not c.equivocate)
    # NPAD = 64, step kernel
    n64 = lambda c: plain(c) and 32 < c.n <= 64  # noqa: E731
    assert insts(n64) >= {("step", 64, 8, B.REF, 2), ("step", 64, 8, B.SPEC, 2), ("step", 64, 4, B.REF, 0),
                          ("step", 64, 4, B.XREF, 0), ("step", 64, 8, B.CONN, 0)}
    assert by["n64-lean-ref-n50-unif3"].specs[0]["delay_model"] == B.UNIF and by["n64-lean-ref-n50-unif3"].specs[0]["dmax"] >= 3
    assert by["n64-xref-n40-slow4"].n == 40 and by["n64-conn-n40-slow6"].n == 40
    assert [c.name for c in CASES if c.n == 64 and c.kernel == "step"] == ["n64-lean-ref-slow8"]
    assert all(c.count == 5 for c in CASES if 32 < c.n <= 64)
    # key-lifetime kernel
    life = [c for c in CASES if c.kernel == "life"]
    assert sorted((c.life, c.mode) for c in life) == sorted([
        ("two-class", B.REF), ("two-class", B.SPEC), ("two-class", B.CONN), ("per-link", B.CONN), ("two-class-hbm", B.REF)])
    # wide kernels
    wide = [c for c in CASES if c.n > 64 and not c.equivocate and c.garbage is None]
    assert {c.n for c in wide if c.inst[1] == 128} == {70, 96} and {c.n for c in wide if c.inst[1] == 256} == {140}
    assert any(c.inst[4] == 4 and c.specs[0]["delay_model"] == B.SLOW for c in wide)
    assert any(c.specs[0]["delay_model"] == B.UNIF and c.inst[4] == 0 for c in wide)
    assert {c.mode for c in wide} == {B.REF, B.SPEC}
    assert all(c.count == 3 and c.specs[0]["round_cap"] == 1 for c in CASES if c.n > 64)
    assert (140 + 63) // 64 == 3 and T.pick_npad(140) // 64 == 4          # the caller's stride against the engine's
    # equivocation pattern and garbage bits
    eq = [c for c in CASES if c.equivocate]
    assert sorted((c.n, c.mode, c.count, c.specs[0]["nv"]) for c in eq) == [(16, B.REF, 13, 2), (16, B.SPEC, 13, 2), (70, B.REF, 3, 2)]
    assert all(c.run.get("byz_pattern") for c in eq)
    assert sorted(c.n for c in CASES if c.garbage is not None) == [13, 140]


@pytest.mark.parametrize("name", NAMES)
def test_mask_rules(name):
    c = B.by_name()[name]
    sets = [tuple(m) for m in c.masks]
    assert len(sets) == c.count and all(list(m) == sorted(set(m)) and all(0 <= d < c.n for d in m) for m in sets)
    assert [sp["g"] for sp in c.specs] == list(range(777, 777 + c.count))
    assert [sp["byzantine"] for sp in c.specs] == [list(m) for m in sets]
    cfg = tuple(sorted(c.cfg_byz))
    assert cfg and cfg not in sets, "the configuration mask must differ from every loaded one"
    assert c.kmax == (c.f if c.mode == B.SPEC or not c.consensus else c.f - 1)
    for it in B.items(c.n, c.count):
        if len(it) >= 2:
            assert len({sets[i] for i in it}) >= 2, (name, it)
    sizes = [len(m) for m in sets]
    if c.n <= 64:
        assert () in sets and (0,) in sets and (c.n - 1,) in sets and c.kmax in sizes
    else:
        words = (c.n + 63) // 64
        assert len(set(sets)) == 3 and c.kmax in sizes
        for m in sets:
            assert {d // 64 for d in m} == set(range(words)) and 0 in m and c.n - 1 in m, (name, m)
    stalled = c.stalled()
    if not c.stall:
        assert not stalled and max(sizes) == c.kmax
    elif c.f >= 2:
        assert len(stalled) == 1 and sorted(sizes)[-2:] == [c.f - 1, c.f]
    else:
        # f = 1: {0} and {n - 1} are sets of f replicas themselves (module docstring)
        assert stalled == [i for i, m in enumerate(sets) if m] and max(sizes) == 1
    if c.equivocate:
        assert len(set(sets)) >= min(c.count, 8) and len(set(sizes)) >= min(3, c.kmax + 1)
        for sp, m in zip(c.specs, sets):
            assert [a for a in sp["actions"] if a["kind"] != "propose"] == T.S.equivocation_actions(c.n, list(m))


def test_garbage_twins_are_the_same_batch():
    by = B.by_name()
    for c in CASES:
        if c.garbage is None:
            continue
        base = by[c.name[:-len("-garbage")]]
        assert [dict(sp, name="") for sp in c.specs] == [dict(sp, name="") for sp in base.specs]
        from tests.engine_runner import mask_words
        clean, dirty = mask_words(base.specs), mask_words(c.specs, c.garbage)
        words = (c.n + 63) // 64
        keep = np.array([(((1 << c.n) - 1) >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(words)], dtype=np.uint64)
        assert clean.shape == dirty.shape == (c.count, words)
        assert (dirty & keep == clean).all() and ((dirty & ~keep) != 0).any(axis=1).all()


@pytest.mark.parametrize("name", NAMES)
def test_case_lands_where_it_is_meant_to(name):
    c = B.by_name()[name]
    for sp in c.specs:
        assert T.instantiation(sp, c.key_window) == c.inst, name
    kernel, npad = c.inst[:2]
    assert npad == T.pick_npad(c.n) and (kernel == "wide") == (c.n > 64)
    if c.kernel == "life":
        # brc_create's eligibility (csrc/brc_engine.hip): NPAD = 64 consensus, Philox / loaded proposals, no
        # pattern, two-class delays up to 8 or per-link delays up to 16 with at most 32 key slots per origin
        sp = c.specs[0]
        per_link = sp["delay_model"] in (B.UNIF, B.GEO)
        assert npad == 64 and c.consensus and not c.equivocate and c.run["proposals"] != "inject"
        assert sp["dmax"] <= (16 if per_link else 8) and not (per_link and c.key_window > 32)
        assert c.life == ("per-link" if per_link else "two-class-hbm" if c.key_window >= 32 else "two-class")
    else:
        assert c.life is None


@pytest.mark.parametrize("name", NAMES)
def test_case_does_real_work_and_its_masks_matter(name):
    c = B.by_name()[name]
    res = B.oracle_results(c)
    assert sorted(res) == list(range(c.count)), "every instance runs on the oracle"
    decided = []
    for i, (exp, dec, delivers) in res.items():
        assert exp["status"] in ("done", "quiescent"), (name, i, exp["status"])
        assert exp["cell_steps"] > 0, (name, i)
        assert not any(d in dec for d in c.masks[i]), (name, i)
        decided.append(all(d in dec for d in B.honest(c, i)))
    assert 2 * sum(res[i][2] > 0 for i in res) >= c.count, (name, "most instances deliver nothing")
    two_class = c.specs[0]["delay_model"] in (B.CONST, B.SLOW)
    if c.consensus:
        assert any(decided), (name, "no instance decides at every honest replica")
        for i in c.stalled():
            assert res[i][0]["status"] == "quiescent" and not decided[i], (name, i)
            if c.f >= 2:
                assert not res[i][1], (name, i, "a replica decided with f silent ones")
        if c.mode == B.SPEC or two_class:
            # per-link delays stall the reference protocol whatever the masks (step_noevent_workloads.TUNED)
            assert all(decided[i] for i in range(c.count) if i not in c.stalled()), (name, decided)
        elif c.kmax > 0:
            assert any(decided[i] for i, m in enumerate(c.masks) if m), (name, "only the empty mask decides")
    nb = B.neighbour_results(c)
    changed = [tuple(res[i][0][k] for k in B.CKEYS) != nb[i] for i in range(c.count)]
    assert 2 * sum(changed) >= c.count, (name, changed)
