"""CPU: the oracle's fourth list (oracle.run(..., kinds=(..., "broadcasts")): one row per call that put a message on a
link, with the key's value id, whether it was the first of its (src, type, key) and its link count) held to bytes the
unmodified reference put on its connections (tests/golden/wire.json), and the preconditions of
tests/event_log_workloads.py, the table tests/test_gpu_event_log.py runs -- on the oracle alone."""
from collections import Counter

import pytest

from oracle import oracle
from tests import event_log_workloads as W
from tests import step_noevent_workloads as T
from tests.golden import specs as S
from tests.test_wire import CASES, codec_for, dst_masks

EV_SEND, EV_COPY = 3, 4                  # include/brc.h BRC_EV_SEND, BRC_EV_COPY


# ---- the new list against the reference's own bytes ---------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c["spec"]["name"] for c in CASES])
def test_broadcast_rows_export_the_reference_bytes(idx):
    case = CASES[idx]
    spec = case["spec"]
    exp = oracle.run(spec, kinds=W.KINDS)
    rows = exp["events"]["broadcasts"]
    assert exp["counts"]["broadcasts"] == len(rows) > 0
    events = [(0, t, EV_SEND if first else EV_COPY, src, typ, kp, s, value)
              for t, src, typ, kp, s, value, first, _links in rows]
    got = codec_for(spec).export(events, dst_masks=dst_masks(spec))
    assert got == case["wire"]
    assert sum(r[7] for r in rows) == exp["msgs_sent"] == case["result"]["msgs_sent"]
    assert [r[:5] for r in rows if r[6]] == exp["events"]["send"]
    assert all(r[6] in (0, 1) and 1 <= r[7] <= spec["n"] for r in rows)


def test_the_other_lists_do_not_depend_on_the_new_one():
    spec = CASES[0]["spec"]
    a, b = oracle.run(spec), oracle.run(spec, kinds=W.KINDS)
    assert "broadcasts" not in a["events"] and "broadcasts" not in a["counts"]
    assert all(a["events"][k] == b["events"][k] for k in a["events"])
    assert oracle.run(spec, kinds=("broadcasts",))["events"]["broadcasts"] == b["events"]["broadcasts"]
    light = oracle.run(spec, light=True)
    assert light["counts"] == a["counts"] and light["msgs_sent"] == a["msgs_sent"]


def test_oracle_run_leaves_the_new_members_alone():
    # a caller built before the fourth list passes a result that ends at cell_steps: oracle_run neither reads nor
    # writes what follows it (here: a buffer of sentinels, a capacity and a count it must not reset)
    import ctypes
    spec = CASES[0]["spec"]
    sp, _actions = oracle.c_spec(spec)
    rows = (ctypes.c_uint32 * (8 * 64))(*[0xA5A5A5A5] * (8 * 64))
    res = oracle._Result(bcasts=rows, bcast_cap=64, n_bcast=12345)
    assert oracle.lib().oracle_run(ctypes.byref(sp), ctypes.byref(res)) == 0
    assert res.n_bcast == 12345 and res.bcast_cap == 64 and set(rows) == {0xA5A5A5A5}
    assert res.n_send == CASES[0]["result"]["counts"]["send"] and res.msgs_sent == CASES[0]["result"]["msgs_sent"]
    assert oracle.lib().oracle_run_broadcasts(ctypes.byref(sp), ctypes.byref(res)) == 0
    assert 0 < res.n_bcast != 12345 and set(rows) != {0xA5A5A5A5}


def test_retry_grows_the_new_list(monkeypatch):
    # more rows than a list's first buffer holds: the run is repeated with bigger ones, all four lists exact
    spec = CASES[-1]["spec"]
    whole = oracle.run(spec, kinds=W.KINDS)
    assert min(whole["counts"].values()) > 0 or spec["mode"] == "brb"
    monkeypatch.setattr(oracle, "FIRST_CAP", 3)
    assert whole["counts"]["broadcasts"] > 2 * 3
    assert oracle.run(spec, kinds=W.KINDS) == whole
    assert oracle.run(spec, kinds=("broadcasts",))["events"]["broadcasts"] == whole["events"]["broadcasts"]


# ---- the workload table --------------------------------------------------------------------------------------------
NAMES = W.names()


def _rows(sp):
    return W.oracle_run(sp)["events"]["broadcasts"]


@pytest.mark.parametrize("name", NAMES)
def test_case_is_final_small_and_within_the_send_count(name):
    case = W.by_name()[name]
    total = 0
    for sp in case.specs:
        exp = W.oracle_run(sp)
        assert exp["status"] in ("quiescent", "done"), (sp["name"], exp["status"])
        rows = exp["events"]["broadcasts"]
        assert sum(r[7] for r in rows) == exp["msgs_sent"]
        assert [r[:5] for r in rows if r[6]] == exp["events"]["send"]
        # the engine's one-byte count of a cell's sends of one type in one step: the 256th copy is its documented limit
        per = Counter((r[1], r[0], r[2]) for r in rows)
        assert max(per.values()) < W.RING_MAX, (sp["name"], per.most_common(1))
        # a delivered key has a row: its value id is known
        keys = {(r[3], r[4]) for r in rows}
        assert all((kp, s) in keys for _t, _node, kp, s in exp["events"]["deliver"])
        total += W.event_count(sp, exp)
    assert 0 < total < W.LIMIT, (name, total)
    assert len({sp["name"] for sp in case.specs}) == len(case.specs)


@pytest.mark.parametrize("name", [c.name for c in W.cases() if c.kind == "storm" and c.connection])
def test_storm_refires(name):
    case = W.by_name()[name]
    (batch,) = case.batches
    n = batch[0]["n"]
    ipw = 1 if n > 32 else 64 // T.pick_npad(n)
    assert len(batch) == (3 * ipw + 1 if n <= 32 else 5 if n <= 64 else 3)
    assert n < T.pick_npad(n)
    for sp in batch:
        rows = _rows(sp)
        byz = set(sp["byzantine"])
        assert sum(r[7] for r in rows) > n * sum(r[6] for r in rows), sp["name"]
        assert any(not r[6] and r[2] == S.READY and r[1] not in byz for r in rows), sp["name"]     # a :119 re-fire
        assert any(not r[6] and r[1] in byz for r in rows), sp["name"]                             # a repeated injection
        assert {r[5] for r in rows} == {sp["g"] % 4}
    assert {sp["g"] % 4 for sp in batch} == {0, 1, 2, 3} or len(batch) < 4


@pytest.mark.parametrize("name", [c.name for c in W.cases() if c.twin_of])
def test_sender_twin_has_no_copy(name):
    case, conn = W.by_name()[name], W.by_name()[W.by_name()[name].twin_of]
    for sp, cp in zip(case.specs, conn.specs):
        assert S.clone(sp, peer_mode="connection", name=cp["name"]) == cp
        rows = _rows(sp)
        assert all(r[6] for r in rows) and sum(r[7] for r in rows) == sp["n"] * len(rows)
        assert len(_rows(cp)) > len(rows)


def test_every_instantiation_has_a_case():
    inst = {c.inst: c for c in W.cases() if hasattr(c, "inst")}
    assert set(inst) == {(k, npad, mode, x) for (k, npad, _dm, mode, x) in T.full_set() - set(T.UNREACHABLE)}
    for key, c in inst.items():
        for sp in c.specs:
            k, npad, _dm, mode, x = T.instantiation(sp, c.open_kw()["key_window"])
            assert (k, npad, mode, x) == key, (c.name, sp["name"])
    table = W.instantiation_cases()
    assert all(c.name == "inst-" + table[key].name for key, c in inst.items() if key != W.W256_SPEC_WV4)
    # the packed kernels keep the table's 3 IPW + 1 instances
    assert all(len(c.specs) == 3 * (64 // key[1]) + 1 for key, c in inst.items() if key[1] <= 32)
    assert len(W.saturation_names()) == len(set(W.saturation_names())) == 4


def test_value_ids():
    cases = W.cases()
    three = [c for c in cases if c.three_bit]
    assert len(three) >= 5
    for c in three:
        for b in c.batches:
            rows = [r for sp in b for r in _rows(sp)]
            high = {(r[3], r[4]) for r in rows if r[5] >= 4}
            assert high, c.name
            assert any((kp, s) in high for sp in b for _t, _n, kp, s in W.oracle_run(sp)["events"]["deliver"]), c.name
    assert max(r[5] for sp in W.by_name()["wv-128-maj"].specs for r in _rows(sp)) == 7
    assert any(r[5] == 0 for c in cases for sp in c.specs for r in _rows(sp))
    # key variants: 2 and 4 per origin
    assert {sp["nv"] for sp in W.by_name()["cons_equivocate_n16"].specs} == {2}
    assert {sp["nv"] for sp in W.by_name()["cons_equivocate4_n16"].specs} == {4}
    assert any(a["kind"] == "deliver" for sp in W.by_name()["cons_deliver_n6"].specs for a in sp["actions"])


def test_spec_case_tosses_the_coin():
    (batch,) = W.by_name()["spec-coin-n70"].batches
    coins = set()
    for sp in batch:
        rows = _rows(sp)
        sends = [r for r in rows if r[2] == S.SEND]
        # every phase-2 key of round 1 carries "-1": no replica counts a value, so none decides or adopts (f = 23 >= 0)
        assert {r[5] for r in sends if r[4] == 1} == {0}
        coin = oracle.lib().oracle_coin_id(sp["coin_seed"], sp["g"], 1)
        assert {r[5] for r in sends if r[4] == 2} == {coin}
        assert {r[5] for r in sends if r[4] == 0} == {1, 2}
        coins.add(coin)
        assert all(rnd == 2 for _t, _node, rnd, _v in W.oracle_run(sp)["events"]["decide"])
    assert coins == {1, 2}


def test_record_cases_log_sends_from_records():
    from tests import restricted_msg_wide_workloads as RW
    from tests import wide_xsend_workloads as XW
    for sp in W.by_name()["xw-128-ref-unif"].specs:
        assert XW.table_records(sp)[0] > 0
    for sp in W.by_name()["rw-128-ref-cons"].specs:
        assert RW.table_records(sp)[0] > 0
