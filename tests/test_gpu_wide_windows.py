"""GPU: key windows of 16 and 32 on the wide step kernels (n > 64) of an engine created with BRC_FLAG_WIDE_WINDOWS,
against the C oracle per instance.  tests/wide_window_workloads.py has one batch of eight instances per shape;
tests/test_wide_window_workloads.py proves their preconditions on the oracle.  Before the feature brc_create refused
the flag bit and every key_window * variants above 8 at n > 64."""
import pytest

from tests import wide_window_workloads as W
from tests.state_compare import state_mismatches

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in W.cases()]
HALVED = [c.name for c in W.cases() if c.half is not None]
LOG = 1 << 20
LOGGED_INSTANCES = 2          # an event-log run keeps the batch's first two instances (about 220,000 events each)


def _runner():
    from tests import engine_runner, wide_records_runner
    return engine_runner, wide_records_runner


def _L():
    from byzantinerandomizedconsensus_amd import _lib
    return _lib


def _open(case, specs=None, cap=0, q=None, flag=True):
    """The engine of one batch, every action injected, not yet run."""
    from byzantinerandomizedconsensus_amd.engine import Engine
    R, F = _runner()
    specs = case.specs if specs is None else specs
    eng = Engine(wide_windows=flag, wide_records=case.rec, wide_values=case.v8,
                 **F.engine_kw(specs, cap, case.q if q is None else q))
    try:
        eng.inject(F.injections(specs))
    except Exception:
        eng.close()
        raise
    return eng


def _read(eng, specs, cap):
    R, F = _runner()
    st = R.read_state(eng, specs)
    ev = None if not cap else [R.sort_result({"events": e})["events"] for e in R.instance_events(eng.events(), specs)]
    return st, ev


def oracle_mismatches(case, st, events=None, count=None):
    """Differences from the oracle: status, t_stop, msgs_sent, arrivals, cell_steps, deliveries, every honest replica's
    record, the ordered event lists where a log is on, the round histogram and the decision histogram."""
    out = []
    specs = case.specs[:count]
    hon = [d for d in range(specs[0]["n"]) if d not in case.byz]
    res = {i: r for i, r in W.oracle_results(case).items() if i < len(specs)}
    hist, counts, undecided, dis = [0] * 66, {}, 0, 0
    for i, (exp, dec, delivers) in res.items():
        r = st["inst"][i]
        out += [("oracle", i, k, r[k], exp[k]) for k in W.CKEYS if r[k] != exp[k]]
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
        if events is not None:
            out += [("oracle", i, k + " events", len(events[i][k]), len(exp["events"][k]))
                    for k in ("deliver", "decide", "send") if events[i][k] != exp["events"][k]]
        firsts = [dec[d][0] for d in hon if d in dec]
        undecided += len(hon) - len(firsts)
        for (_r, _t, v) in firsts:
            counts[v] = counts.get(v, 0) + 1
        dis += len({v for (_r, _t, v) in firsts}) > 1
        hist[min(max(rr for (rr, _t, _v) in firsts), 65) if len(firsts) == len(hon) else 0] += 1
    labels = specs[0]["values"] if len(specs[0]["values"]) == 8 else ("-1", "0", "1", "3")
    want = {lab: counts.get(v, 0) for v, lab in enumerate(labels)}
    want["undecided"] = undecided
    if st["hist"] != hist:
        out.append(("oracle", "round_histogram", st["hist"], hist))
    if st["dec"] != (want, dis):
        out.append(("oracle", "decisions", st["dec"], (want, dis)))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_workload_equals_oracle(name):
    L = _L()
    case = W.by_name()[name]
    with _open(case) as eng:
        assert eng.cfg.flags & L.FLAG_WIDE_WINDOWS and eng.cfg.key_window * eng.cfg.variants in (16, 32)
        eng.run()
        assert eng.last_kernel() == "step"
        st, _ev = _read(eng, case.specs, 0)
        print(name, "kernel_ms %.2f" % eng.last_kernel_ms(), [{k: r[k] for k in W.CKEYS} for r in st["inst"]])
    assert st["stats"]["running"] == 0
    assert not any(r["status"] == "overflow" for r in st["inst"])
    diff = oracle_mismatches(case, st)
    assert not diff, (name, diff[:8])


@pytest.mark.parametrize("name", W.LOGGED)
def test_event_log_equals_oracle(name):
    case = W.by_name()[name]
    specs = case.specs[:LOGGED_INSTANCES]
    with _open(case, specs, LOG) as eng:
        eng.run()
        st, ev = _read(eng, specs, LOG)
    assert st["stats"]["running"] == 0 and st["stats"]["events_dropped"] == 0
    diff = oracle_mismatches(case, st, ev, LOGGED_INSTANCES)
    assert not diff, (name, diff[:8])


@pytest.mark.parametrize("name", HALVED)
def test_half_the_window_overflows(name):
    """The window is in use: the same batch on a flagged engine at half the window stops an instance with BRC_OVERFLOW."""
    case = W.by_name()[name]
    with _open(case, q=case.half) as eng:
        eng.run()
        res = eng.instances_result()
    print(name, case.half, [r["status"] for r in res])
    assert any(r["status"] == "overflow" for r in res), [r["status"] for r in res]


def test_sliced_run_equals_oneshot():
    """brc_run(max_steps = 7) until nothing runs, at window 32: 4,096 slots of metadata, the activity ring and the key
    list's source rows persist across launches."""
    case = W.by_name()[W.SLICED]
    with _open(case) as eng:
        eng.run()
        whole, _ = _read(eng, case.specs, 0)
    with _open(case) as eng:
        slices = 1
        while eng.run(7):
            slices += 1
        got, _ = _read(eng, case.specs, 0)
    assert slices > 4
    diff = state_mismatches(whole, got, "one-shot vs slices of 7")
    assert not diff, diff[:8]
    assert not oracle_mismatches(case, got)


def test_reset_then_the_same_results():
    R, F = _runner()
    case = W.by_name()[W.RESET]
    with _open(case) as eng:
        eng.run()
        first, _ = _read(eng, case.specs, 0)
        eng.reset()
        eng.inject(F.injections(case.specs))
        eng.run()
        again, _ = _read(eng, case.specs, 0)
    diff = state_mismatches(first, again, "first run vs after brc_reset")
    assert not diff, diff[:8]
    assert not oracle_mismatches(case, again)


def test_unflagged_parity():
    """An existing wide shape at window 8: flag off against flag on, identical results (and the oracle's)."""
    case = W.parity_case()
    out = []
    for flag in (False, True):
        with _open(case, flag=flag) as eng:
            eng.run()
            out.append(_read(eng, case.specs, 0)[0])
    diff = state_mismatches(out[0], out[1], "flagless vs flagged")
    assert not diff, diff[:8]
    assert not oracle_mismatches(case, out[1])


def _cfg(n=70, **kw):
    L = _L()
    base = dict(n=n, f=5, instances=1, protocol="consensus", seed=1, delay_model=L.DELAY_SLOWSET, delay_max=8,
                round_cap=1, step_cap=400, key_window=16)
    base.update(kw)
    return base


def test_refusals():
    """None of these launches a kernel."""
    from byzantinerandomizedconsensus_amd.engine import Engine
    L = _L()

    def refused(word, flag=True, **kw):
        with pytest.raises(L.EngineError) as err:
            Engine(wide_windows=flag, **_cfg(**kw))
        assert err.value.code == L.E_INVALID and word in str(err.value), str(err.value)

    refused("n > 64", n=64)                                       # the narrow kernels take the window without the flag
    Engine(**_cfg(n=64)).close()
    refused("BRC_MODE_SPEC", mode=L.MODE_SPEC)
    refused("BRC_MODE_SPEC", mode=L.MODE_SPEC, key_window=8)
    refused("sender peers", peer_mode=L.PEER_CONNECTION)
    refused("field ranges", key_window=64)
    refused("field ranges", key_window=32, variants=2)
    # without the flag: today's refusals
    refused("field ranges", flag=False)
    refused("field ranges", flag=False, n=130, key_window=8, variants=2)
    refused("field ranges", flag=False, mode=L.MODE_BEB, key_window=32)
    # NPAD 256, key window 32, per-link delays above 8: the carve is 164,016 B
    for model in (L.DELAY_UNIFORM, L.DELAY_GEOMETRIC):
        refused("exceeds the kernel's LDS", n=130, key_window=32, delay_model=model, delay_max=16)
    # ... everything else at 32 slots per lane fits
    for kw in (dict(n=130, key_window=32, delay_max=16), dict(n=130, key_window=16, variants=2, delay_model=L.DELAY_GEOMETRIC, delay_max=16),
               dict(n=130, key_window=32, delay_model=L.DELAY_UNIFORM, delay_max=8), dict(n=128, key_window=32, delay_model=L.DELAY_GEOMETRIC, delay_max=16),
               dict(n=256, key_window=16, delay_model=L.DELAY_GEOMETRIC, delay_max=16, mode=L.MODE_BEB)):
        Engine(wide_windows=True, **_cfg(**kw)).close()
    # the flags combine
    Engine(wide_windows=True, wide_records=True, wide_values=True, **_cfg()).close()


def test_create_equals_the_acceptance_model():
    """brc_create against wide_window_workloads.accepted over the whole grid (n = 70 / 130, every delay model and DM,
    16 and 32 slots per replica in every split), flagged and flagless, SPEC and connection peers: what the model takes
    is created, what it refuses is BRC_E_INVALID.  No step kernel is launched."""
    from byzantinerandomizedconsensus_amd.engine import Engine
    L = _L()
    model_of = {W.I.CONST: L.DELAY_CONST, W.UNIF: L.DELAY_UNIFORM, W.SLOW: L.DELAY_SLOWSET, W.GEO: L.DELAY_GEOMETRIC}
    wrong = []
    for n in W.GRID_N:
        for model, dmax in W.GRID_DELAYS:
            for q, nv in W.GRID_SLOTS:
                kw = _cfg(n=n, f=n // 3, delay_model=model_of[model], delay_max=dmax, key_window=q, variants=nv)
                for flag, mode, conn in ((True, L.MODE_REFERENCE, False), (True, L.MODE_BEB, False), (False, L.MODE_REFERENCE, False),
                                         (True, L.MODE_SPEC, False), (True, L.MODE_REFERENCE, True)):
                    if mode == L.MODE_SPEC and nv != 1:
                        continue                                  # refused above 64 replicas whatever the window
                    want = W.accepted(n, W.I.SPEC if mode == L.MODE_SPEC else W.REF, q, nv, model, dmax, conn=conn, flag=flag)
                    try:
                        Engine(wide_windows=flag, mode=mode, peer_mode=L.PEER_CONNECTION if conn else L.PEER_SENDER, **kw).close()
                        got = True
                    except L.EngineError as err:
                        assert err.code == L.E_INVALID, str(err)
                        got = False
                    if got != want:
                        wrong.append((n, model, dmax, q, nv, flag, mode, conn, got, want))
    assert not wrong, wrong[:8]


def test_class_api_engine_takes_window_16():
    """A 70-node sender-peer consensus cluster creates its engine with BRC_FLAG_WIDE_WINDOWS and key_window 16; a
    broadcast cluster of the same peers keeps window 8 and no such flag."""
    from byzantinerandomizedconsensus_amd import network
    L = _L()
    network.reset()
    try:
        peers = tuple(("localhost", 9400 + i) for i in range(70))
        for cons in (True, False):
            c = network.Cluster(peers, dict(network.settings(), peer_mode="sender"))
            c.N, c.f = 70, 23
            c.nodes = {i: object() for i in range(70)}
            if cons:
                c.add_consensus(object(), 0)
            c._create_engine()
            try:
                cfg = c.engine.cfg
                assert (cfg.key_window, bool(cfg.flags & L.FLAG_WIDE_WINDOWS)) == ((16, True) if cons else (8, False))
                assert cfg.variants == 1 and cfg.n == 70
            finally:
                c.engine.close()
    finally:
        network.reset()
