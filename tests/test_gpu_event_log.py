"""GPU: the whole event log against the oracle -- every brc_event field of every record, the value id of DELIVER / SEND /
COPY events and the BRC_EV_COPY records of connection-identity peers included (tests/engine_runner.instance_events,
which every other parity module compares, drops the value id and the COPY kind) -- and a log that fills up: capacities
1, total / 2, total - 1, total and total + 1 of a batch that logs `total` events.  tests/event_log_workloads.py is the
table; tests/test_event_log_workloads.py proves its preconditions on the oracle and holds the oracle's broadcast rows
to the reference's own bytes."""
import ctypes
from collections import Counter

import pytest

from tests import event_log_workloads as W
from tests.state_compare import state_mismatches

pytestmark = pytest.mark.gpu

LOG = W.LIMIT                            # a roomy log: every case logs fewer events (test_event_log_workloads)
SENTINEL = 0xA5


def _mods():
    from byzantinerandomizedconsensus_amd import _lib as L
    from tests import engine_runner as R, wide_records_runner as F
    return L, R, F


def _open(case, specs, cap):
    """The engine of one batch of the case, inputs in place, not yet run."""
    L, R, F = _mods()
    kw = case.open_kw()
    if case.opener == "batch":
        return R.open_batch(specs, cap, **kw)
    if case.opener == "flagged":
        return F.open_flagged(specs, cap, **kw)
    assert case.opener == "values"
    from byzantinerandomizedconsensus_amd.engine import Engine
    eng = Engine(wide_values=True, wide_records=kw["wide_records"], proposals=L.PROPOSALS_LOADED,
                 **F.engine_kw(specs, cap, kw["key_window"]))
    try:
        _feed_values(eng, specs)
    except Exception:
        eng.close()
        raise
    return eng


def _feed_values(eng, specs):
    _L, R, _F = _mods()
    eng.load_proposals(R._loaded_proposals(specs))
    inj = []
    for i, sp in enumerate(specs):
        inj += R._injections(dict(sp, actions=[a for a in sp["actions"] if a["kind"] != "propose"]), i)
    eng.inject(inj)


# ---- full records ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", W.names())
def test_full_records_equal_the_oracle(name):
    L, R, _F = _mods()
    case = W.by_name()[name]
    for specs in case.batches:
        with _open(case, specs, LOG) as eng:
            eng.run()
            assert eng.last_kernel() == "step"
            inst, stats, evs = eng.instances_result(), eng.stats(), eng.events()
        assert stats["events_dropped"] == 0 and stats["running"] == 0
        per = R.instance_event_tuples(evs, len(specs))
        assert sum(map(len, per)) == len(evs)
        for i, sp in enumerate(specs):
            exp = W.oracle_run(sp)
            got, want = Counter(per[i]), Counter(R.oracle_event_tuples(sp, exp))
            diff = sorted((got - want).items())[:6], sorted((want - got).items())[:6]
            assert got == want, (sp["name"], "engine only / oracle only", diff)
            assert sorted(per[i]) == sorted(want.elements())
            kinds = Counter(ev[1] for ev in per[i])
            rows = exp["events"]["broadcasts"]
            for k in ("status", "t_stop", "msgs_sent", "arrivals", "cell_steps"):
                assert inst[i][k] == exp[k], (sp["name"], k, inst[i][k], exp[k])
            if sp.get("peer_mode") == "connection":
                assert inst[i]["msgs_sent"] == sum(r[7] for r in rows)
                assert kinds[L.EV_SEND] + kinds[L.EV_COPY] == len(rows)
            else:
                assert kinds[L.EV_COPY] == 0
                assert kinds[L.EV_SEND] == sum(r[6] for r in rows)
        if case.kind == "storm" and case.connection:
            assert any(ev[2] == L.EV_COPY for ev in evs)


# ---- a log that fills up -------------------------------------------------------------------------------------------
SAT = W.saturation_names()
CAPS = ("one", "half", "total-1", "total", "total+1")
_TWIN = {}


def _batch(name):
    case = W.by_name()[name]
    (specs,) = case.batches
    return case, specs


def _twin(name):
    """(read_state(), events(), total) of the case with a roomy log."""
    if name not in _TWIN:
        _L, R, _F = _mods()
        case, specs = _batch(name)
        with _open(case, specs, LOG) as eng:
            eng.run()
            st, evs = R.read_state(eng, specs), eng.events()
        assert st["stats"]["events_dropped"] == 0 and len(evs) == sum(W.event_count(sp, W.oracle_run(sp)) for sp in specs)
        assert len(evs) >= 4
        _TWIN[name] = (st, evs, len(evs))
    return _TWIN[name]


def _capacity(which, total):
    return {"one": 1, "half": total // 2, "total-1": total - 1, "total": total, "total+1": total + 1}[which]


def _with_dropped(st, dropped):
    return dict(st, stats=dict(st["stats"], events_dropped=dropped))


def _raw(eng, L, first, cap, ranged=True):
    """brc_read_events_range(first) / brc_read_events into a sentinel-filled buffer of cap records: (records the call
    wrote, as tuples; the count it reports).  A record is written if any of its bytes changed."""
    arr = (L.Event * cap)()
    ctypes.memset(arr, SENTINEL, ctypes.sizeof(arr))
    cnt = ctypes.c_size_t(0)
    if ranged:
        eng._chk(eng._lib.brc_read_events_range(eng._h, first, arr, cap, ctypes.byref(cnt)))
    else:
        eng._chk(eng._lib.brc_read_events(eng._h, arr, cap, ctypes.byref(cnt)))
    size = ctypes.sizeof(L.Event)
    raw = bytes(arr)
    blank = bytes([SENTINEL]) * size
    written = [j for j in range(cap) if raw[j * size:(j + 1) * size] != blank]
    assert written == list(range(len(written))), written           # a prefix of the buffer
    return [(e.instance, e.t, e.kind, e.node, e.type, e.a, e.b, e.value) for e in arr[:len(written)]], cnt.value


def _check_saturated(eng, L, st, name, C):
    """Every read-out of an engine that ran the case `name` with event capacity C."""
    st0, ev0, total = _twin(name)
    stored = min(C, total)
    diff = state_mismatches(_with_dropped(st0, max(0, total - C)), st, "roomy log vs capacity %d" % C)
    assert not diff, (name, C, diff[:8])
    assert st["stats"]["events_dropped"] == max(0, total - C)
    got, cnt = _raw(eng, L, 0, stored + 8, ranged=False)
    got_r, cnt_r = _raw(eng, L, 0, stored + 8)
    assert cnt == cnt_r == total
    assert len(got) == len(got_r) == stored and Counter(got) == Counter(got_r)
    over = Counter(got) - Counter(ev0)                    # an unwritten, doubly written or torn slot is no twin event
    assert not over, (name, C, sorted(over.items())[:6])
    if total > C:
        for call in (eng.events, lambda: eng.events_since(0)):
            with pytest.raises(L.EngineError) as err:
                call()
            assert err.value.code == L.E_STATE
    else:
        assert Counter(eng.events()) == Counter(ev0)
        since, tot = eng.events_since(0)
        assert tot == total and Counter(since) == Counter(ev0)
    # the records at and past the capacity are never copied; the last stored one is
    if C <= total:
        assert _raw(eng, L, C, 8) == ([], total)
        last, _ = _raw(eng, L, C - 1, 8)
        assert len(last) == 1 and not Counter(last) - Counter(ev0)


@pytest.mark.parametrize("which", CAPS)
@pytest.mark.parametrize("name", SAT)
def test_full_log_keeps_the_first_records_and_the_state(name, which):
    L, R, _F = _mods()
    case, specs = _batch(name)
    total = _twin(name)[2]
    C = _capacity(which, total)
    with _open(case, specs, C) as eng:
        eng.run()
        _check_saturated(eng, L, R.read_state(eng, specs), name, C)


def test_sliced_run_fills_the_log_like_the_oneshot_run():
    L, R, _F = _mods()
    name = SAT[3]
    case, specs = _batch(name)
    total = _twin(name)[2]
    C = total // 2
    with _open(case, specs, C) as eng:
        slices, seen = 0, 0
        while eng.run(3):
            slices += 1
            cnt = ctypes.c_size_t(0)
            eng._chk(eng._lib.brc_read_events(eng._h, None, 0, ctypes.byref(cnt)))
            assert seen <= cnt.value <= total
            seen = cnt.value
        assert slices >= 2
        _check_saturated(eng, L, R.read_state(eng, specs), name, C)


def test_reset_restarts_the_count():
    L, R, _F = _mods()
    name = SAT[0]
    case, specs = _batch(name)
    total = _twin(name)[2]
    C = total // 2
    with _open(case, specs, C) as eng:
        eng.run()
        _check_saturated(eng, L, R.read_state(eng, specs), name, C)
        eng.reset()
        assert _raw(eng, L, 0, 8) == ([], 0) and eng.events() == [] and eng.stats()["events_dropped"] == 0
        inj = []
        for i, sp in enumerate(specs):
            inj += R._injections(sp, i)
        eng.inject(inj)
        eng.run()
        _check_saturated(eng, L, R.read_state(eng, specs), name, C)
