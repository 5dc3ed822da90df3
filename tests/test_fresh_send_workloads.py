"""Preconditions of tests/test_gpu_fresh_send.py, on the oracle and the schedule alone (no GPU): every workload of
tests/fresh_send_workloads.py contains the situation it is named for.  A slot is "unwritten" from the step its key is
SENT (or declared) until the first step at which that SEND reaches an honest receiver; whatever else touches the key
in between is a fallback that has to write the row first."""
import pytest

from tests import fresh_send_workloads as W
from tests import step_noevent_workloads as T
from tests.golden import specs as S


def _hon(sp):
    return [d for d in range(sp["n"]) if d not in sp["byzantine"]]


def _landings(sp, origin, t_send, dst=None):
    """The steps at which origin's SEND of step t_send reaches honest receivers."""
    sch = W.schedule(sp)
    return sorted({t_send + sch.delay(sp["g"], origin, d) for d in _hon(sp) if dst is None or (dst >> d) & 1})


def test_every_case_runs_to_its_end_on_the_oracle():
    for case in W.cases():
        res = T.oracle_results(case)
        assert sorted(res) == list(range(case.count)), case.name
        want = {"stepcap"} if case.name.endswith("-cut") else {"done", "quiescent"}
        assert {r[0]["status"] for r in res.values()} <= want, case.name
        assert all(r[0]["cell_steps"] > 0 for r in res.values()), case.name


@pytest.mark.parametrize("name", ["fresh-ref-cfg4-cap1", "fresh-ref-const3", "fresh-ref-unif4-cap3", "fresh-ref-n33"])
def test_first_landings_and_later_ones(name):
    """Two delay classes: a fast origin's SEND lands twice (the first landing is the fresh key-step, the second an
    ordinary one), a slow origin's once.  One class: once.  Per link: some origin's SEND lands at three steps or more."""
    case = W.by_name()[name]
    per = []
    for sp in case.specs:
        per.append([len(_landings(sp, o, 0)) for o in _hon(sp)])
    flat = [x for v in per for x in v]
    if "const3" in name:
        assert set(flat) == {1}
    elif "unif4" in name:
        assert max(flat) >= 3
    else:
        assert all(set(v) == {1, 2} for v in per), per


def test_early_messages_reach_keys_still_in_flight():
    for mode in ("ref", "spec"):
        case = W.by_name()["fresh-%s-early" % mode]
        for sp in case.specs:
            first = {o: _landings(sp, o, 0)[0] for o in W.ORIGINS}
            msgs = [a for a in sp["actions"] if a["kind"] == "byz" and a["type"] in (S.ECHO, S.READY)]
            assert {a["type"] for a in msgs} == {S.ECHO, S.READY}
            # stamped before the key's SEND lands anywhere (slow origins), and after its first landing (fast ones)
            assert any(a["t"] < first[a["kp"]] for a in msgs) and any(a["t"] >= first[a["kp"]] for a in msgs), sp["name"]


def test_restricted_sends_land_on_unwritten_rows():
    case = W.by_name()["fresh-ref-restricted"]
    for sp in case.specs:
        sends = [a for a in sp["actions"] if a["kind"] == "byz" and a["type"] == S.SEND]
        assert len(sends) == 2 and all(a["dst"] != W.ALL64 for a in sends)
        # each reaches an honest destination, and nothing touches its key before that
        for a in sends:
            assert _landings(sp, a["src"], a["t"], a["dst"]), sp["name"]
            assert not [b for b in sp["actions"] if b is not a and b["kind"] == "byz" and b["kp"] == a["kp"]]


def test_declared_key_stays_unwritten_across_the_epoch_move():
    c32_rebase = 100                                 # csrc/brc_internal.h C32_REBASE, restated
    case = W.by_name()["fresh-ref-declared"]
    for sp in case.specs:
        key = next(a for a in sp["actions"] if a["kind"] == "byz_key")
        send = next(a for a in sp["actions"] if a["kind"] == "byz" and a["kp"] == key["kp"])
        assert key["t"] == 0 and send["type"] == S.SEND and send["t"] > c32_rebase
        # the first burst is over long before: the step of the SEND is the next one the kernel visits
        assert max(_landings(sp, o, 0)[-1] for o in W.ORIGINS) + 16 < send["t"]


def test_reuse_allocates_one_slot_twice():
    case = W.by_name()["fresh-ref-reuse"]
    q = W.REUSE_Q
    for sp, (exp, _dec, delivers) in zip(case.specs, T.oracle_results(case).values()):
        sends = [(a["t"], a["kp"], a["s"]) for a in sp["actions"] if a["kind"] == "brb_send"]
        slots = {}
        for t, o, s in sends:
            slots.setdefault((o, s % q), []).append((t, s))
        assert all(len(v) == 2 and v[0][1] != v[1][1] for v in slots.values()), slots
        # both keys of every slot deliver at every honest replica: the second allocation is not an overflow
        assert exp["status"] == "quiescent" and delivers == 2 * len(slots) * len(_hon(sp))


def test_cut_run_stops_with_sends_in_flight():
    for mode in ("ref", "spec"):
        case = W.by_name()["fresh-%s-cut" % mode]
        for sp in case.specs:
            assert sp["step_cap"] == W.CUT_CAP
            last = [_landings(sp, o, 0)[-1] for o in _hon(sp)]
            first = [_landings(sp, o, 0)[0] for o in _hon(sp)]
            assert any(t > W.CUT_CAP for t in first) and all(t > W.CUT_CAP for t in last), sp["name"]


def test_direct_delivers_name_keys_still_in_flight():
    case = W.by_name()["fresh-ref-deliver"]
    for sp in case.specs:
        acts = [a for a in sp["actions"] if a["kind"] == "deliver"]
        assert len(acts) == 6 and all(a["t"] == 2 for a in acts)
        # the hosts' own phase-0 keys are still travelling to the slow receivers at step 2
        assert all(_landings(sp, a["kp"], 0)[-1] > 2 for a in acts)


def test_one_step_slices_cut_between_allocation_and_landing():
    """Every step is a launch boundary in the sliced runs, and a SEND lands a step after it was made at the earliest:
    every key has a boundary between its allocation and its first landing; in the two-class cases some keys have
    several (slow origins: 8 steps)."""
    for name in W.SLICED:
        case = W.by_name()[name]
        first = [_landings(sp, o, 0)[0] for sp in case.specs for o in _hon(sp)]
        assert min(first) >= 1, name
        assert "unif4" in name or max(first) == 8, name


def test_instantiations_cover_both_mask_forms():
    """The recorded instantiations (step_noevent_workloads.instantiation: what brc_create picks) are lean n = 64
    kernels with register delay masks (NLR = 2) and with LDS masks (NLR = 0), under REFERENCE and under SPEC -- in the
    main table and among the per-instance mask cases."""
    insts = {c.inst for c in W.cases()}
    assert all(i[:2] == ("step", 64) for i in insts), insts
    assert {(i[3], i[4]) for i in insts} == {(T.REF, 2), (T.REF, 0), (T.SPEC, 2), (T.SPEC, 0)}, insts
    for c in W.cases():
        assert c.inst == T.instantiation(c.specs[0], c.key_window), c.name
        two = c.specs[0]["delay_model"] in (T.SLOW, T.CONST)
        assert c.inst[4] == (2 if two else 0), c.name
    minst = {(c.inst[3], c.inst[4]) for c in W.mask_cases()}
    assert {(T.REF, 2), (T.SPEC, 2), (T.SPEC, 0)} <= minst, minst


def test_mask_cases_carry_different_masks():
    for c in W.mask_cases():
        masks = [tuple(sp["byzantine"]) for sp in c.specs]
        assert masks == [tuple(m) for m in c.masks] and len(set(masks)) >= 5, (c.name, masks)
        assert tuple(c.cfg_byz) not in masks and c.cfg_byz, c.name
        assert () in masks and (0,) in masks and (c.n - 1,) in masks, c.name
        # a neighbour's mask gives another result: the masks matter
        from tests import byz_mask_workloads as B
        own = [tuple(r[0][k] for k in B.CKEYS) for r in B.oracle_results(c).values()]
        other = B.neighbour_results(c)
        assert sum(a != b for a, b in zip(own, other)) * 2 >= c.count, c.name


def test_late_declared_case_rebases_with_an_unwritten_slot():
    """Shifted by LATE_T0, the declared case stays below STEP_LIMIT and its declared key waits 120 steps (more than
    C32_REBASE = 100) for its SEND, with nothing else going on between."""
    from tests import time_axis_workloads as TA
    case = W.by_name()["fresh-ref-declared"]
    t_last = max(r[0]["t_stop"] for r in T.oracle_results(case).values())
    assert W.LATE_T0 + t_last < TA.STEP_LIMIT and "fresh-ref-declared" in W.LATE
    for sp in case.specs:
        late = TA.shift(sp, W.LATE_T0)
        key = next(a for a in late["actions"] if a["kind"] == "byz_key")
        send = next(a for a in late["actions"] if a["kind"] == "byz" and a["kp"] == key["kp"])
        assert key["t"] == W.LATE_T0 and send["t"] - key["t"] > 100
