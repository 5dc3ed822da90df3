"""GPU: three-bit consensus value ids on the wide key-lifetime kernel (csrc/brc_life_wide.h V8; n in 65..256) of an engine
created with BRC_FLAG_WIDE_LIFE | BRC_FLAG_LIFE_VALUES, against the C oracle per instance and against the wide step
kernel of an Engine(wide_values=True) array for array.  tests/life_values_workloads.py has the batches;
tests/test_life_values_workloads.py proves their preconditions on the oracle.  Before the feature Engine() took no
life_values keyword and brc_create refused flag bit 128."""
import ctypes

import numpy as np
import pytest

from tests import life_values_workloads as LV
from tests.golden import specs as S
from tests.state_compare import state_mismatches

pytestmark = pytest.mark.gpu

NAMES = [b.name for b in LV.batches()]


def _L():
    from byzantinerandomizedconsensus_amd import _lib
    return _lib


def _open(batch, flag, specs=None, offset=None, loaded=True, life_values=None):
    """The engine of one batch, proposing by itself (loaded ids, or Philox draws), not yet run.  flag: the wide
    key-lifetime kernel with 3-bit ids (life_values: None = flag); else the wide step kernel with BRC_FLAG_WIDE_VALUES."""
    from byzantinerandomizedconsensus_amd.engine import Engine
    from tests import engine_runner as R
    L = _L()
    specs = batch.specs if specs is None else specs
    sp0 = specs[0]
    assert all(R._cfg_key(sp, not batch.load_masks) == R._cfg_key(sp0, not batch.load_masks) and sp["g"] == sp0["g"] + i
               for i, sp in enumerate(specs))
    kw = dict(n=sp0["n"], f=sp0["f"], instances=len(specs), protocol="consensus", seed=sp0["seed"],
              delay_model=sp0["delay_model"], delay_max=sp0["dmax"], delay_const=sp0.get("dconst", 1),
              round_cap=sp0["round_cap"], step_cap=sp0["step_cap"], key_window=batch.q, variants=batch.nv,
              byzantine=batch.cfg_byz if batch.load_masks else sp0["byzantine"],
              instance_offset=sp0["g"] if offset is None else offset,
              mode=L.MODE_BEB if sp0["mode"].startswith("beb") else L.MODE_REFERENCE,
              proposals=L.PROPOSALS_LOADED if loaded else L.PROPOSALS_PHILOX,
              byz_pattern=L.BYZ_EQUIVOCATE if batch.pattern else L.BYZ_NONE, wide_windows=batch.wide_windows)
    if flag:
        eng = Engine(wide_life=True, life_pattern=batch.pattern, life_values=flag if life_values is None else life_values, **kw)
    else:
        eng = Engine(wide_values=loaded, **kw)
    try:
        if batch.load_masks:
            eng.load_byzantine(R.mask_words([dict(n=sp0["n"], byzantine=sp["byzantine"]) for sp in specs]))
        if loaded:
            eng.load_proposals(R._loaded_proposals(specs))
    except Exception:
        eng.close()
        raise
    return eng


def _run(batch, flag, **kw):
    from tests import engine_runner as R
    specs = kw.get("specs") or batch.specs
    with _open(batch, flag, **kw) as eng:
        before = eng.last_kernel()
        eng.run()
        kernel = eng.last_kernel()
        assert before == kernel == ("life" if flag else "step"), (before, kernel)
        st = R.read_state(eng, specs)
        print(batch.name, "life" if flag else "step", "kernel_ms %.2f" % eng.last_kernel_ms(),
              [{k: r[k] for k in LV.CKEYS} for r in st["inst"][:3]], st["dec"])
        high = st["dec"] is not None and len(st["dec"][0]) > 5 and any(st["dec"][0][lab] for lab in S.VALUES8[4:])
        if high:
            # an id >= 4 was decided: the four-id read-out refuses
            L = _L()
            arr, dis = np.zeros(5, dtype=np.uint64), ctypes.c_uint64(0)
            with pytest.raises(L.EngineError) as err:
                eng._chk(eng._lib.brc_read_decisions(eng._h, arr.ctypes.data_as(ctypes.c_void_p), ctypes.byref(dis)))
            assert err.value.code == L.E_STATE and "brc_read_value_decisions" in str(err.value)
        st["high"] = high
    return st


def _strip(st):
    """lane_loads and max_t count a kernel's own work (tests/test_gpu_life.py); `high` is this module's note."""
    out = dict(st, stats={k: v for k, v in st["stats"].items() if k not in ("lane_loads", "max_t")})
    out.pop("high", None)
    return out


def oracle_mismatches(batch, st, res=None, specs=None):
    """Differences from the oracle: status, t_stop, msgs_sent, arrivals, cell_steps, deliveries, every honest replica's
    record (the instance's own Byzantine list); over a whole batch also the round histogram and the eight-id decision
    histogram (brc_read_value_decisions)."""
    out = []
    specs = batch.specs if specs is None else specs
    whole = res is None
    res = LV.oracle_results(batch) if whole else res
    hist, counts, undecided, dis = [0] * 66, {}, 0, 0
    for i, (exp, dec, delivers) in res.items():
        hon = [d for d in range(specs[i]["n"]) if d not in specs[i]["byzantine"]]
        r = st["inst"][i]
        out += [("oracle", i, k, r[k], exp[k]) for k in LV.CKEYS if r[k] != exp[k]]
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
        want = {lab: counts.get(v, 0) for v, lab in enumerate(S.VALUES8)}
        want["undecided"] = undecided
        if st["hist"] != hist:
            out.append(("oracle", "round_histogram", st["hist"], hist))
        if st["dec"] != (want, dis):
            out.append(("oracle", "decisions", st["dec"], (want, dis)))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_batch_equals_oracle_and_step_kernel(name):
    batch = LV.by_name()[name]
    life = _run(batch, True)
    assert life["stats"]["running"] == 0
    assert not any(r["status"] == "overflow" for r in life["inst"])
    if batch.oracle:
        diff = oracle_mismatches(batch, life)
        assert not diff, (name, diff[:8])
        # (tests/test_life_values_workloads.py: every batch but the one that stalls by arithmetic decides ids >= 4)
        assert life["high"] == any(v >= 4 for (_e, dec, _n) in LV.oracle_results(batch).values()
                                   for ds in dec.values() for (_r, _t, v) in ds[:1])
    else:
        assert life["high"] and all(r["status"] == "done" for r in life["inst"])
    step = _run(batch, False)
    diff = state_mismatches(_strip(step), _strip(life), "step kernel (wide_values) vs lifetime kernel (life_values)")
    assert not diff, (name, diff[:8])


def test_reset_and_reset_at():
    """brc_reset then a run equals the first run; brc_reset_at with the next instances' proposals loaded equals a fresh
    engine there: the HBM host-mask planes start from zero every time."""
    from tests import engine_runner as R
    batch = LV.by_name()[LV.RESET]
    other = LV.OFFSET + 1                     # (the majority id goes by g + i: every instance gets another one)
    moved_specs = [dict(batch._make(other + i, i), name="lv-moved/%d" % i, values=S.VALUES8) for i in range(LV.COUNT)]
    assert R._loaded_proposals(moved_specs).tolist() != R._loaded_proposals(batch.specs).tolist()
    with _open(batch, True) as eng:
        eng.run()
        first = R.read_state(eng, batch.specs)
        eng.reset()
        assert eng.last_kernel() == "life"
        eng.run()
        again = R.read_state(eng, batch.specs)
        eng.reset_at(other)
        eng.load_proposals(R._loaded_proposals(moved_specs))
        eng.run()
        assert eng.last_kernel() == "life"
        moved = R.read_state(eng, moved_specs)
    assert any(first["dec"][0][lab] for lab in S.VALUES8[4:])
    diff = state_mismatches(first, again, "first run vs after brc_reset")
    assert not diff, diff[:8]
    assert not oracle_mismatches(batch, again)
    with _open(batch, True, specs=moved_specs) as eng:
        eng.run()
        fresh = R.read_state(eng, moved_specs)
    diff = state_mismatches(fresh, moved, "fresh engine at the offset vs brc_reset_at")
    assert not diff, diff[:8]
    assert state_mismatches(first, moved, "the other proposals change the run")


@pytest.mark.parametrize("name", LV.BINARY)
def test_binary_proposals_equal_the_unflagged_lifetime_engine(name):
    """Philox-drawn binary proposals: Engine(wide_life=True, life_values=True) equals Engine(wide_life=True) in every
    read_state() field."""
    from tests import engine_runner as R
    batch = LV.by_name()[name]
    specs = LV.binary_specs(name)
    out = []
    for lv in (False, True):
        with _open(batch, True, specs=specs, loaded=False, life_values=lv) as eng:
            eng.run()
            assert eng.last_kernel() == "life" and bool(eng.cfg.flags & _L().FLAG_LIFE_VALUES) == lv
            out.append(R.read_state(eng, specs))
            print(name, "life_values" if lv else "wide_life", "kernel_ms %.2f" % eng.last_kernel_ms())
    diff = state_mismatches(out[0], out[1], "wide_life vs wide_life + life_values")
    assert not diff, diff[:8]
    assert out[0]["stats"]["running"] == 0 and any(r["status"] == "done" for r in out[0]["inst"])


def test_256_instances_in_one_launch():
    """As many workgroups as CUs: four sampled instances against the oracle, the whole batch against the step kernel."""
    batch = LV.by_name()[LV.BIG]
    specs = LV.big_specs()
    life = _run(batch, True, specs=specs)
    assert life["stats"]["running"] == 0 and len(life["inst"]) == LV.BIG_COUNT and life["high"]
    res = LV.big_oracle()
    firsts = {dec[0][0][2] for (_e, dec, _n) in res.values()}
    assert len(firsts) >= 2 and min(firsts) >= 4, firsts
    diff = oracle_mismatches(batch, life, res, specs)
    assert not diff, diff[:8]
    step = _run(batch, False, specs=specs)
    diff = state_mismatches(_strip(step), _strip(life), "step kernel vs lifetime kernel, 256 instances")
    assert not diff, diff[:8]


def test_eight_id_run_on_both_kernels():
    """A cfg5-sized committee (n = 128, f = 10, slow-set D = 8) with proposals drawn over ids 0 .. 7, 64 instances: the
    two kernels agree array for array; their kernel_ms are printed."""
    from byzantinerandomizedconsensus_amd.engine import Engine
    from tests import engine_runner as R
    L = _L()
    n, count = 128, 64
    kw = dict(n=n, f=10, instances=count, protocol="consensus", seed=0x17A1E128, delay_model=L.DELAY_SLOWSET, delay_max=8,
              round_cap=2, step_cap=LV.STEP_CAP, key_window=8, proposals=L.PROPOSALS_LOADED, instance_offset=LV.OFFSET)
    ids = np.array(LV.drawn_ids(n, count, 0x17A1E), dtype=np.int8)
    specs = [dict(values=S.VALUES8)]
    out = []
    for flags in (dict(wide_life=True, life_values=True), dict(wide_values=True)):
        with Engine(**flags, **kw) as eng:
            eng.load_proposals(ids)
            eng.run()
            print("eight-id", eng.last_kernel(), "kernel_ms %.2f" % eng.last_kernel_ms(), eng.stats()["cell_steps"])
            out.append(R.read_state(eng, specs))
    assert out[0]["stats"]["running"] == 0
    diff = state_mismatches(_strip(out[1]), _strip(out[0]), "step kernel vs lifetime kernel, drawn ids")
    assert not diff, diff[:8]


def _cfg(n=70, **kw):
    L = _L()
    base = dict(n=n, f=5, instances=1, protocol="consensus", seed=1, delay_model=L.DELAY_SLOWSET, delay_max=8,
                round_cap=1, step_cap=400, key_window=8, proposals=L.PROPOSALS_LOADED)
    base.update(kw)
    return base


def test_refusals():
    from byzantinerandomizedconsensus_amd.engine import Engine
    L = _L()
    with Engine(wide_life=True, life_values=True, **_cfg()) as eng:
        assert eng.last_kernel() == "life"
        with pytest.raises(L.EngineError) as err:
            eng.load_proposals([[8] * 70])
        assert err.value.code == L.E_INVALID and "[0, 7]" in str(err.value)
        eng.load_proposals([[7] * 70])
        assert eng.last_kernel() == "life"
        eng.run()
        assert eng.last_kernel() == "life" and eng.stats()["running"] == 0
    # without the flag: as before
    with Engine(wide_life=True, **_cfg()) as eng:
        with pytest.raises(L.EngineError) as err:
            eng.load_proposals([[4] * 70])
        assert err.value.code == L.E_INVALID and "[0, 3]" in str(err.value) and "BRC_FLAG_WIDE_VALUES" in str(err.value)
        eng.load_proposals([[3] * 70])
    for kw, word in ((dict(wide_life=False), "needs BRC_FLAG_WIDE_LIFE"), (dict(n=64), "n > 64"),
                     (dict(peer_mode=L.PEER_CONNECTION), "sender peers"), (dict(mode=L.MODE_SPEC), "BRC_MODE_SPEC")):
        wl = kw.pop("wide_life", True)
        with pytest.raises(L.EngineError) as err:
            Engine(wide_life=wl, life_values=True, **_cfg(**kw))
        assert err.value.code == L.E_INVALID and "BRC_FLAG_LIFE_VALUES" in str(err.value) and word in str(err.value), str(err.value)
    with pytest.raises(L.EngineError) as err:
        Engine(wide_life=True, life_values=True, wide_values=True, **_cfg())
    assert err.value.code == L.E_INVALID and "BRC_FLAG_WIDE_RECORDS / BRC_FLAG_WIDE_VALUES" in str(err.value)


def test_lifetime_only_engine_refuses_injections_and_stepped_runs():
    from byzantinerandomizedconsensus_amd.engine import Engine
    L = _L()
    with Engine(wide_life=True, life_values=True, **_cfg()) as eng:
        eng.load_proposals([[5] * 70])
        with pytest.raises(L.EngineError) as err:
            eng.inject([dict(t=0, kind=L.INJ_PROPOSE, instance=0, node=1, value=5)])
        assert err.value.code == L.E_UNSUPPORTED and "key-lifetime kernel" in str(err.value)
        with pytest.raises(L.EngineError) as err:
            eng.run(max_steps=1)
        assert err.value.code == L.E_UNSUPPORTED and "key-lifetime kernel" in str(err.value)
        eng.run()
        assert eng.last_kernel() == "life" and eng.stats()["running"] == 0
        assert eng.decisions(tuple(S.VALUES8))[0]["beta"] == 70
