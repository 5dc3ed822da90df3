"""GPU: the wide key-lifetime kernel (csrc/brc_life_wide.h; n in 65..256, constant and slow-set delays) of an engine
created with BRC_FLAG_WIDE_LIFE, against the C oracle per instance and against the wide step kernel of an unflagged
engine array for array.  tests/wide_life_workloads.py has the batches; tests/test_wide_life_workloads.py proves their
preconditions on the oracle.  Before the feature brc_create refused the flag bit."""
import os

import pytest

from tests import wide_life_workloads as WL
from tests.state_compare import state_mismatches

pytestmark = pytest.mark.gpu

NAMES = [b.name for b in WL.batches()]


def _L():
    from byzantinerandomizedconsensus_amd import _lib
    return _lib


def _open(batch, flag, specs=None, q=None, wide_windows=None, offset=None):
    """The engine of one batch, proposing by itself (Philox draws or loaded ids), not yet run."""
    from byzantinerandomizedconsensus_amd.engine import Engine
    from tests import engine_runner as R
    from tests import wide_records_runner as F
    L = _L()
    specs = batch.specs if specs is None else specs
    kw = F.engine_kw(specs, 0, batch.q if q is None else q)
    if offset is not None:
        kw["instance_offset"] = offset
    eng = Engine(wide_life=flag, wide_windows=batch.wide_windows if wide_windows is None else wide_windows,
                 proposals=L.PROPOSALS_LOADED if batch.proposals == "loaded" else L.PROPOSALS_PHILOX, **kw)
    try:
        if batch.proposals == "loaded":
            eng.load_proposals(R._loaded_proposals(specs))
    except Exception:
        eng.close()
        raise
    return eng


def _run(batch, flag, **kw):
    from tests import engine_runner as R
    with _open(batch, flag, **kw) as eng:
        before = eng.last_kernel()
        eng.run()
        kernel = eng.last_kernel()
        assert before == kernel == ("life" if flag else "step"), (before, kernel)
        st = R.read_state(eng, kw.get("specs") or batch.specs)
        print(batch.name, "flag" if flag else "step", "kernel_ms %.2f" % eng.last_kernel_ms(),
              [{k: r[k] for k in WL.CKEYS} for r in st["inst"][:8]])
    return st


def _strip(st):
    """lane_loads and max_t count a kernel's own work (tests/test_gpu_life.py)."""
    return dict(st, stats={k: v for k, v in st["stats"].items() if k not in ("lane_loads", "max_t")})


def oracle_mismatches(batch, st, res=None, specs=None):
    """Differences from the oracle (the comparison of tests/test_gpu_wide_windows.py::oracle_mismatches): status, t_stop,
    msgs_sent, arrivals, cell_steps, deliveries, every honest replica's record; over a whole batch also the round
    histogram and the decision histogram."""
    out = []
    specs = batch.specs if specs is None else specs
    whole = res is None
    res = WL.oracle_results(batch) if whole else res
    hon = [d for d in range(specs[0]["n"]) if d not in batch.byz]
    hist, counts, undecided, dis = [0] * 66, {}, 0, 0
    for i, (exp, dec, delivers) in res.items():
        r = st["inst"][i]
        out += [("oracle", i, k, r[k], exp[k]) for k in WL.CKEYS if r[k] != exp[k]]
        if r["deliveries"] != delivers:
            out.append(("oracle", i, "deliveries", r["deliveries"], delivers))
        for d in hon:
            rep, mine = st["reps"][i][d], dec.get(d, [])
            if rep["decide_count"] != len(mine):
                out.append(("oracle", i, d, "decide_count", rep["decide_count"], len(mine)))
            if mine:
                got = (rep["first_decide_round"], rep["first_decide_t"], rep["first_decide_value"])
                if got != mine[0] or rep["last_decide_value"] != mine[-1][2]:
                    out.append(("oracle", i, d, "decisions", got, rep["last_decide_value"], mine[0], mine[-1][2]))
        if bool(r["decided"]) != all(d in dec for d in hon):
            out.append(("oracle", i, "decided", r["decided"]))
        firsts = [dec[d][0] for d in hon if d in dec]
        undecided += len(hon) - len(firsts)
        for (_r, _t, v) in firsts:
            counts[v] = counts.get(v, 0) + 1
        dis += len({v for (_r, _t, v) in firsts}) > 1
        hist[min(max(rr for (rr, _t, _v) in firsts), 65) if len(firsts) == len(hon) else 0] += 1
    if whole:
        want = {lab: counts.get(v, 0) for v, lab in enumerate(("-1", "0", "1", "3"))}
        want["undecided"] = undecided
        if st["hist"] != hist:
            out.append(("oracle", "round_histogram", st["hist"], hist))
        if st["dec"] != (want, dis):
            out.append(("oracle", "decisions", st["dec"], (want, dis)))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_batch_equals_oracle_and_step_kernel(name):
    batch = WL.by_name()[name]
    life = _run(batch, True)
    assert life["stats"]["running"] == 0
    assert not any(r["status"] == "overflow" for r in life["inst"])
    if batch.stepcap:
        assert all(r["status"] == "stepcap" for r in life["inst"])
    diff = oracle_mismatches(batch, life)
    assert not diff, (name, diff[:8])
    step = _run(batch, False)
    diff = state_mismatches(_strip(step), _strip(life), "step kernel vs lifetime kernel")
    assert not diff, (name, diff[:8])


def test_overflow_parity_at_half_the_window():
    """The window-16 batch at window 8: BRC_OVERFLOW on both kernels, at the same step and with the same counters."""
    batch = WL.by_name()[WL.Q16]
    life = _run(batch, True, q=8, wide_windows=False)
    step = _run(batch, False, q=8, wide_windows=False)
    assert any(r["status"] == "overflow" for r in life["inst"]), [r["status"] for r in life["inst"]]
    diff = state_mismatches(_strip(step), _strip(life), "step kernel vs lifetime kernel at window 8")
    assert not diff, diff[:8]


def test_reset_and_reset_at():
    from tests import engine_runner as R
    batch = WL.by_name()[WL.RESET]
    other = WL.OFFSET + 4
    with _open(batch, True) as eng:
        eng.run()
        first = R.read_state(eng, batch.specs)
        eng.reset()
        assert eng.last_kernel() == "life"
        eng.run()
        again = R.read_state(eng, batch.specs)
        eng.reset_at(other)
        eng.run()
        assert eng.last_kernel() == "life"
        moved = R.read_state(eng, batch.specs)
    diff = state_mismatches(first, again, "first run vs after brc_reset")
    assert not diff, diff[:8]
    assert not oracle_mismatches(batch, again)
    with _open(batch, True, offset=other) as eng:
        eng.run()
        fresh = R.read_state(eng, batch.specs)
    diff = state_mismatches(fresh, moved, "fresh engine at the offset vs brc_reset_at")
    assert not diff, diff[:8]
    # instances 4 .. 7 of the first run are instances 0 .. 3 at the other offset
    assert [r for r in moved["inst"][:4]] == [r for r in first["inst"][4:]]


def _cfg(n=70, **kw):
    L = _L()
    base = dict(n=n, f=n // 3, instances=1, protocol="consensus", seed=1, delay_model=L.DELAY_SLOWSET, delay_max=8,
                round_cap=1, step_cap=400, key_window=8, proposals=L.PROPOSALS_PHILOX)
    base.update(kw)
    return base


def test_refusals():
    from byzantinerandomizedconsensus_amd.engine import Engine
    L = _L()

    def refused(word, **kw):
        flags = {k: kw.pop(k) for k in ("wide_records", "wide_values", "wide_windows") if k in kw}
        with pytest.raises(L.EngineError) as err:
            Engine(wide_life=True, **flags, **_cfg(**kw))
        assert err.value.code == L.E_INVALID and word in str(err.value), str(err.value)

    refused("n > 64", n=64)
    refused("peer_mode", peer_mode=L.PEER_CONNECTION)
    refused("protocol", protocol="brb", proposals=L.PROPOSALS_NONE)
    refused("proposals", proposals=L.PROPOSALS_NONE)
    refused("delay_model", delay_model=L.DELAY_UNIFORM, delay_max=4)
    refused("delay_model", delay_model=L.DELAY_GEOMETRIC)
    refused("delay_max", delay_max=16)
    refused("event_capacity", event_capacity=1024)
    refused("byz_pattern", byz_pattern=L.BYZ_EQUIVOCATE, variants=2, key_window=4, byzantine=(3,))
    refused("BRC_FLAG_WIDE_RECORDS", wide_records=True)
    refused("BRC_FLAG_WIDE_RECORDS", wide_values=True)
    refused("field ranges", key_window=16)                         # windows above 8 need BRC_FLAG_WIDE_WINDOWS as well
    refused("field ranges", mode=L.MODE_SPEC, variants=2, key_window=4)
    # (an LDS carve that does not fit is refused too, but no accepted window reaches it: 8,192 slots take 92,736 B)
    assert WL.lds_bytes_life_wide(256, 32, 1, False) == 92736
    old = os.environ.get("BRC_KERNEL")
    os.environ["BRC_KERNEL"] = "step"
    try:
        refused("BRC_KERNEL=step")
    finally:
        os.environ.pop("BRC_KERNEL", None)
        if old is not None:
            os.environ["BRC_KERNEL"] = old
    # what the flag takes: every mode, constant delays, windows 16 / 32 with BRC_FLAG_WIDE_WINDOWS
    for kw in (dict(), dict(mode=L.MODE_SPEC), dict(mode=L.MODE_BEB), dict(delay_model=L.DELAY_CONST, delay_const=3),
               dict(n=256, f=85), dict(key_window=4, variants=2), dict(key_window=16, wide_windows=True),
               dict(n=130, f=43, key_window=32, wide_windows=True)):
        ww = kw.pop("wide_windows", False)
        with Engine(wide_life=True, wide_windows=ww, **_cfg(**kw)) as eng:
            assert eng.last_kernel() == "life"


def test_lifetime_only_engine_refuses_injections_and_stepped_runs():
    from byzantinerandomizedconsensus_amd.engine import Engine
    L = _L()
    with Engine(wide_life=True, **_cfg()) as eng:
        assert eng.last_kernel() == "life"
        with pytest.raises(L.EngineError) as err:
            eng.inject([dict(t=0, kind=L.INJ_PROPOSE, instance=0, node=1, value=1)])
        assert err.value.code == L.E_UNSUPPORTED and "key-lifetime kernel" in str(err.value)
        with pytest.raises(L.EngineError) as err:
            eng.run(max_steps=1)
        assert err.value.code == L.E_UNSUPPORTED and "key-lifetime kernel" in str(err.value)
        eng.run()
        assert eng.last_kernel() == "life" and eng.stats()["running"] == 0


def test_unflagged_engine_stays_on_the_step_kernel():
    """... also under BRC_KERNEL=life, which selects nothing above 64 replicas."""
    from byzantinerandomizedconsensus_amd.engine import Engine
    old = os.environ.get("BRC_KERNEL")
    try:
        for env in (None, "life"):
            os.environ.pop("BRC_KERNEL", None)
            if env:
                os.environ["BRC_KERNEL"] = env
            with Engine(**_cfg()) as eng:
                assert eng.last_kernel() == "step"
                eng.run()
                assert eng.last_kernel() == "step" and eng.stats()["running"] == 0
    finally:
        os.environ.pop("BRC_KERNEL", None)
        if old is not None:
            os.environ["BRC_KERNEL"] = old


def test_512_instances_in_one_launch():
    """More workgroups than CUs: eight sampled instances against the oracle, the whole batch against the step kernel."""
    batch = WL.by_name()[WL.BIG]
    specs = WL.big_specs()
    life = _run(batch, True, specs=specs)
    assert life["stats"]["running"] == 0 and len(life["inst"]) == WL.BIG_COUNT
    diff = oracle_mismatches(batch, life, WL.big_oracle(), specs)
    assert not diff, diff[:8]
    step = _run(batch, False, specs=specs)
    diff = state_mismatches(_strip(step), _strip(life), "step kernel vs lifetime kernel, 512 instances")
    assert not diff, diff[:8]
