"""GPU: the equivocation pattern (BRC_BYZ_EQUIVOCATE) on the wide key-lifetime kernel's pattern form
(csrc/brc_life_wide.h PAT) of an engine created with BRC_FLAG_WIDE_LIFE | BRC_FLAG_LIFE_PATTERN, against the C oracle per
instance (which runs the pattern as actions) and against an unflagged engine running the same byz_pattern on the wide
step kernel, array for array.  tests/life_pattern_workloads.py has the batches; tests/test_life_pattern_workloads.py
proves their preconditions on the oracle.  Before the feature brc_create refused flag bit 32."""
import pytest

from tests import life_pattern_workloads as LP
from tests.state_compare import state_mismatches

pytestmark = pytest.mark.gpu

NAMES = [b.name for b in LP.batches()]


def _L():
    from byzantinerandomizedconsensus_amd import _lib
    return _lib


def _open(batch, flag, offset=None, masks=None):
    """The engine of one batch: the engine's own pattern, proposing by itself (Philox draws or loaded ids), the
    instances' masks loaded where they differ (masks: other Byzantine lists, one per instance); not yet run."""
    from byzantinerandomizedconsensus_amd.engine import Engine
    from tests import engine_runner as R
    L = _L()
    specs = batch.specs
    sp0 = specs[0]
    assert all(R._cfg_key(sp, not batch.load_masks) == R._cfg_key(sp0, not batch.load_masks) and sp["g"] == sp0["g"] + i
               for i, sp in enumerate(specs))
    kw = dict(n=sp0["n"], f=sp0["f"], instances=len(specs), protocol="consensus", seed=sp0["seed"],
              delay_model=sp0["delay_model"], delay_max=sp0["dmax"], delay_const=sp0.get("dconst", 1),
              round_cap=sp0["round_cap"], step_cap=sp0["step_cap"], key_window=batch.q, variants=batch.nv,
              byzantine=batch.cfg_byz if batch.load_masks else sp0["byzantine"],
              instance_offset=sp0["g"] if offset is None else offset,
              mode=L.MODE_BEB if sp0["mode"].startswith("beb") else L.MODE_REFERENCE,
              proposals=L.PROPOSALS_LOADED if batch.proposals == "loaded" else L.PROPOSALS_PHILOX,
              byz_pattern=L.BYZ_EQUIVOCATE, wide_windows=batch.wide_windows)
    eng = Engine(wide_life=flag, life_pattern=flag, **kw)
    try:
        if batch.load_masks or masks is not None:
            lists = [sp["byzantine"] for sp in specs] if masks is None else masks
            eng.load_byzantine(R.mask_words([dict(n=sp0["n"], byzantine=b) for b in lists]))
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
        st = R.read_state(eng, batch.specs)
        print(batch.name, "flag" if flag else "step", "kernel_ms %.2f" % eng.last_kernel_ms(),
              [{k: r[k] for k in LP.CKEYS} for r in st["inst"][:8]])
    return st


def _strip(st):
    """lane_loads and max_t count a kernel's own work (tests/test_gpu_life.py)."""
    return dict(st, stats={k: v for k, v in st["stats"].items() if k not in ("lane_loads", "max_t")})


def oracle_mismatches(batch, st):
    """Differences from the oracle: status, t_stop, msgs_sent, arrivals, cell_steps, deliveries, every honest replica's
    record (the instance's own Byzantine list), the round histogram and the decision histogram."""
    out = []
    specs = batch.specs
    res = LP.oracle_results(batch)
    hist, counts, undecided, dis = [0] * 66, {}, 0, 0
    for i, (exp, dec, delivers) in res.items():
        hon = [d for d in range(specs[i]["n"]) if d not in specs[i]["byzantine"]]
        r = st["inst"][i]
        out += [("oracle", i, k, r[k], exp[k]) for k in LP.CKEYS if r[k] != exp[k]]
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
    want = {lab: counts.get(v, 0) for v, lab in enumerate(("-1", "0", "1", "3"))}
    want["undecided"] = undecided
    if st["hist"] != hist:
        out.append(("oracle", "round_histogram", st["hist"], hist))
    if st["dec"] != (want, dis):
        out.append(("oracle", "decisions", st["dec"], (want, dis)))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_batch_equals_oracle_and_step_kernel(name):
    batch = LP.by_name()[name]
    life = _run(batch, True)
    assert life["stats"]["running"] == 0
    assert not any(r["status"] == "overflow" for r in life["inst"])
    diff = oracle_mismatches(batch, life)
    assert not diff, (name, diff[:8])
    step = _run(batch, False)
    diff = state_mismatches(_strip(step), _strip(life), "step kernel vs lifetime kernel")
    assert not diff, (name, diff[:8])


def test_reset_reset_at_and_masks_loaded_again():
    from tests import engine_runner as R
    batch = LP.by_name()[LP.RESET]
    other = LP.OFFSET + 4
    rotated = LP.rotated_masks(batch)
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
        eng.reset_at(LP.OFFSET)
        eng.load_byzantine(R.mask_words([dict(n=batch.specs[0]["n"], byzantine=b) for b in rotated]))
        assert eng.last_kernel() == "life"
        eng.run()
        remasked = R.read_state(eng, batch.specs)
    diff = state_mismatches(first, again, "first run vs after brc_reset")
    assert not diff, diff[:8]
    assert not oracle_mismatches(batch, again)
    with _open(batch, True, offset=other) as eng:
        eng.run()
        fresh = R.read_state(eng, batch.specs)
    diff = state_mismatches(fresh, moved, "fresh engine at the offset vs brc_reset_at")
    assert not diff, diff[:8]
    with _open(batch, True, masks=rotated) as eng:
        eng.run()
        fresh = R.read_state(eng, batch.specs)
    diff = state_mismatches(fresh, remasked, "fresh engine with the other masks vs brc_load_byzantine after a reset")
    assert not diff, diff[:8]
    assert state_mismatches(first, remasked, "the other masks change the run")
    # ... and equal to the step kernel under the same masks
    with _open(batch, False, masks=rotated) as eng:
        eng.run()
        step = R.read_state(eng, batch.specs)
    diff = state_mismatches(_strip(step), _strip(remasked), "step kernel vs lifetime kernel, masks loaded again")
    assert not diff, diff[:8]


def _cfg(n=70, **kw):
    L = _L()
    base = dict(n=n, f=n // 3, instances=1, protocol="consensus", seed=1, delay_model=L.DELAY_SLOWSET, delay_max=8,
                round_cap=1, step_cap=400, key_window=4, variants=2, proposals=L.PROPOSALS_PHILOX,
                byz_pattern=L.BYZ_EQUIVOCATE, byzantine=(3, 66))
    base.update(kw)
    return base


def test_refusals():
    from byzantinerandomizedconsensus_amd.engine import Engine
    L = _L()

    def refused(word, wide_life=True, life_pattern=True, **kw):
        ww = kw.pop("wide_windows", False)
        with pytest.raises(L.EngineError) as err:
            Engine(wide_life=wide_life, life_pattern=life_pattern, wide_windows=ww, **_cfg(**kw))
        assert err.value.code == L.E_INVALID and word in str(err.value), str(err.value)

    # the flag alone: each case names it
    refused("BRC_FLAG_LIFE_PATTERN", wide_life=False)
    refused("BRC_FLAG_LIFE_PATTERN", wide_life=False, byz_pattern=L.BYZ_NONE)
    refused("BRC_FLAG_LIFE_PATTERN", n=64)
    refused("BRC_FLAG_LIFE_PATTERN", n=64, wide_life=False)
    refused("BRC_FLAG_LIFE_PATTERN", byz_pattern=L.BYZ_NONE)
    refused("BRC_FLAG_LIFE_PATTERN", peer_mode=L.PEER_CONNECTION)
    refused("BRC_FLAG_LIFE_PATTERN", mode=L.MODE_SPEC, variants=1, key_window=8)
    refused("BRC_FLAG_LIFE_PATTERN", mode=L.MODE_SPEC)
    refused("BRC_FLAG_LIFE_PATTERN", variants=1, key_window=8)
    # without the new flag BRC_FLAG_WIDE_LIFE still refuses a pattern
    refused("byz_pattern", life_pattern=False)
    # everything else BRC_FLAG_WIDE_LIFE requires
    refused("protocol", protocol="brb", proposals=L.PROPOSALS_NONE)
    refused("proposals", proposals=L.PROPOSALS_NONE)
    refused("delay_model", delay_model=L.DELAY_UNIFORM, delay_max=4)
    refused("delay_max", delay_max=16)
    refused("event_capacity", event_capacity=1024)
    refused("field ranges", key_window=8)                              # 8 x 2 needs BRC_FLAG_WIDE_WINDOWS as well
    # what the two flags take
    for kw in (dict(), dict(mode=L.MODE_BEB), dict(delay_model=L.DELAY_CONST, delay_const=3), dict(n=256, f=85),
               dict(variants=4, key_window=2), dict(key_window=8, wide_windows=True),
               dict(n=130, f=43, key_window=16, wide_windows=True)):
        ww = kw.pop("wide_windows", False)
        with Engine(wide_life=True, life_pattern=True, wide_windows=ww, **_cfg(**kw)) as eng:
            assert eng.last_kernel() == "life"


def test_lifetime_only_engine_refuses_injections_and_stepped_runs():
    from byzantinerandomizedconsensus_amd.engine import Engine
    L = _L()
    with Engine(wide_life=True, life_pattern=True, **_cfg()) as eng:
        assert eng.last_kernel() == "life"
        with pytest.raises(L.EngineError) as err:
            eng.inject([dict(t=0, kind=L.INJ_PROPOSE, instance=0, node=1, value=1)])
        assert err.value.code == L.E_UNSUPPORTED and "key-lifetime kernel" in str(err.value)
        with pytest.raises(L.EngineError) as err:
            eng.run(max_steps=1)
        assert err.value.code == L.E_UNSUPPORTED and "key-lifetime kernel" in str(err.value)
        eng.run()
        assert eng.last_kernel() == "life" and eng.stats()["running"] == 0
