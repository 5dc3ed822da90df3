"""GPU: the slot generation tags of the non-lean narrow step kernels (brc_step at NPAD 4 .. 32, and at NPAD 64 with
general keys or connection peers) across many resets on ONE engine.  Their cells are never swept: a reset keeps each
slot's 13-bit generation and the cells, and a cell reads as stale while its tag differs from the slot's, so
exactness rests on the host's count of the allocations (csrc/brc_engine.hip gen_used; DESIGN.md section 3, "Key
slots").  tests/gen_tag_workloads.py has the walks; tests/test_gen_tag_workloads.py proves their preconditions.

Per compared epoch, bit-exact: instances_result(), replicas(), stats(), round_histogram, decisions and the sorted
event lists equal the oracle on every instance, and every read_state() field equals a fresh engine's for the same
batch (nothing excluded)."""
import time

import pytest

from tests import gen_tag_workloads as W
from tests.test_gpu_interleaved import oracle_mismatches
from tests.test_gpu_step_noevent import state_mismatches

pytestmark = pytest.mark.gpu

LOG = 1 << 20
_FRESH, _INJ = {}, {}


def _runner():
    from tests import engine_runner
    return engine_runner


def _L():
    from byzantinerandomizedconsensus_amd import _lib
    return _lib


def injections(batch):
    if batch.name not in _INJ:
        R = _runner()
        _INJ[batch.name] = [x for i, sp in enumerate(batch.specs) for x in R._injections(sp, i)]
    return _INJ[batch.name]


def fresh(case, batch, cap):
    """The batch on an engine of its own: once per batch and log setting."""
    if (batch.name, cap) not in _FRESH:
        R = _runner()
        if cap:
            _FRESH[(batch.name, cap)] = R.run_batch_noevents(batch.specs, event_capacity=cap, with_events=True, **case.open_kw())
        else:
            _FRESH[(batch.name, cap)] = (R.run_batch_noevents(batch.specs, **case.open_kw()), None)
    return _FRESH[(batch.name, cap)]


def run_epoch(eng, batch, cap):
    R = _runner()
    eng.inject(injections(batch))
    eng.run()
    assert eng.last_kernel() == "step"
    st = R.read_state(eng, batch.specs)
    ev = [R.sort_result({"events": e})["events"] for e in R.instance_events(eng.events(), batch.specs)] if cap else None
    return st, ev


def epoch_mismatches(case, batch, cap, st, ev, skip=()):
    want, want_ev = fresh(case, batch, cap)
    out = [d for d in state_mismatches(want, st, "fresh engine vs epoch") if not (d[1] in ("inst", "replica") and d[2] in skip)]
    if cap:
        out += [("events vs fresh engine", i) for i, (a, b) in enumerate(zip(want_ev, ev)) if a != b and i not in skip]
    return out + [d for d in oracle_mismatches(batch, st, ev) if d[1] not in skip]


def walk(case, name, cap, compare=None):
    """Every epoch of the walk on one engine; compare(e) -> whether epoch e is read and compared (default: all).
    Returns the first failing epoch's (number, mismatches), or None."""
    R = _runner()
    epochs = case.walk(name)
    batches = {}
    for tag, _off, specs in epochs:
        batches.setdefault(tag, W.Batch(case, name, tag, specs))
    t0 = time.time()
    with R.open_batch([dict(sp, actions=[]) for sp in epochs[0][2]], event_capacity=cap, **case.open_kw()) as eng:
        off = epochs[0][1]
        for e, (tag, o, _specs) in enumerate(epochs):
            if e:
                if o != off:
                    eng.reset_at(o)
                    off = o
                else:
                    eng.reset()
            batch = batches[tag]
            if compare is None or compare(e):
                st, ev = run_epoch(eng, batch, cap)
                assert st["stats"]["running"] == 0 and st["stats"]["events_dropped"] == 0, (case.name, name, e, st["stats"])
                diff = epoch_mismatches(case, batch, cap, st, ev)
                if diff:
                    return e, diff
            else:
                eng.inject(injections(batch))
                eng.run()
    print(case.name, name, "log" if cap else "nolog", len(epochs), "epochs", "%.2f s" % (time.time() - t0))
    return None


# every walk with an event log; without one (the EV = false builds) once per cell layout and packing: 1-word tagged
# cells packed (NPAD 4, 16 instances a wave; NPAD 16 re-keyed) and alone in the wave (NPAD 64), 5-word connection-peer
# cells packed (NPAD 8) and alone (NPAD 64)
NOLOG = (("p4", "wrap"), ("p16", "wrap_at"), ("n40-xref", "wrap"), ("n6-conn", "wrap"), ("n40-conn", "wrap"))
WRAPS = [(c.name, w, cap) for c in W.cases() for w in ("wrap", "wrap_at") if w in c.walks for cap in (LOG, 0)
         if cap or (c.name, w) in NOLOG]


@pytest.mark.parametrize("name,shape,cap", WRAPS, ids=["%s-%s-%s" % (n, w, "log" if c else "nolog") for n, w, c in WRAPS])
def test_tag_wrap_by_bare_keys(name, shape, cap):
    """K byz_key records of one key per epoch advance its slot's tag K times, which the host has to know: after
    8192 / K epochs the slot would stand at a tag it wrote cells under, and their F_DEL flags would swallow the
    epoch's deliveries.  Every epoch is compared, with an event log and (NOLOG) on the EV = false builds."""
    case = W.by_name()[name]
    if shape == "wrap_at":
        (ta, _oa, a), (tb, _ob, b) = case.walk(shape)[:2]
        fa, fb = fresh(case, W.Batch(case, shape, ta, a), cap)[0], fresh(case, W.Batch(case, shape, tb, b), cap)[0]
        assert state_mismatches(fa, fb, "A vs B"), "the two id ranges give one result: nothing is shown"
    bad = walk(case, shape, cap)
    assert bad is None, (name, shape, "first failing epoch", bad[0], bad[1][:8])


@pytest.mark.parametrize("name", [c.name for c in W.cases() if "full_clear" in c.walks])
def test_epochs_across_the_full_clear(name):
    """One SEND at phase index 4000 books a thousand generations per epoch: brc_reset clears fully before the
    seventh epoch.  The epochs before it, the clearing one and those after it all equal a fresh engine."""
    case = W.by_name()[name]
    bad = walk(case, "full_clear", LOG)
    assert bad is None, (name, "first failing epoch", bad[0], bad[1][:8])


def test_s_limit_stops_the_instance_at_the_action():
    """Key window 2: after an epoch at phase index 4000, a SEND at s_limit - 1 runs and equals the oracle; a SEND at
    s_limit stops its instance with BRC_OVERFLOW at the step of the action; its packed siblings equal the oracle.
    The full clear follows, and the third epoch equals a fresh engine again."""
    R = _runner()
    case = W.by_name()["p8"]
    (ta, _o, first), (tb, _o, second), _third = case.walk("s_limit")
    A, B = W.Batch(case, "s_limit", ta, first), W.Batch(case, "s_limit", tb, second)
    lim = second[1]["probe"][1]
    with R.open_batch([dict(sp, actions=[]) for sp in first], event_capacity=LOG, **case.open_kw()) as eng:
        st, ev = run_epoch(eng, A, LOG)
        assert not epoch_mismatches(case, A, LOG, st, ev)
        eng.reset()
        st, ev = run_epoch(eng, B, LOG)
        r = st["inst"][1]
        t_act = [a["t"] for a in second[1]["actions"] if a["s"] == lim]
        print("s_limit", lim, r)
        assert r["status"] == "overflow" and [r["t_stop"]] == t_act and r["deliveries"] == 0, r
        # on a fresh engine the same SEND is below the limit and runs
        assert fresh(case, B, LOG)[0]["inst"][1]["status"] == "quiescent"
        diff = [d for d in epoch_mismatches(case, B, LOG, st, ev, skip=(1,)) if d[1] != "stats"]
        assert not diff, diff[:8]
        assert st["inst"][0]["status"] == "quiescent" and st["inst"][0]["deliveries"] == 6
        eng.reset()
        st, ev = run_epoch(eng, A, LOG)
        assert not epoch_mismatches(case, A, LOG, st, ev)


@pytest.mark.parametrize("name", [c.name for c in W.cases() if "consensus" in c.walks])
def test_consensus_epochs_across_the_full_clear(name):
    """The consensus pass allocates inside the kernel (send_key_now): gen_base crosses GEN_FULL_CLEAR once, and the
    walk goes on to where an engine that never cleared would be out of tags.  Every 16th epoch, the four around the
    clear and the last equal the first, which the oracle pins.  (Measured: c8-spec 197 epochs of 800 steps, 17 s --
    a step of these small batches costs about 100 us whatever the batch, and the generations booked per step are
    fixed by Q, so a higher round cap does not shorten it.)"""
    case = W.by_name()[name]
    epochs = case.walk("consensus")
    used = case.consensus_used(epochs[0][2])
    _bases, clears = W.host_walk([used] * len(epochs))
    near = set(range(clears[0] - 2, clears[0] + 2)) | {len(epochs) - 1}
    bad = walk(case, "consensus", LOG, compare=lambda e: e % 16 == 0 or e in near)
    assert bad is None, (name, "first failing epoch", bad[0], "full clear at", clears, bad[1][:8])


def test_budget_refusal_is_reachable_and_reset_recovers():
    """8192 KEYs of one key in one epoch would bring the tag back within the epoch, where nothing can clear:
    brc_run refuses (BRC_E_STATE, "slot generation budget exhausted") before anything runs, and after brc_reset
    the engine runs a batch that equals the oracle."""
    R, L = _runner(), _L()
    case = W.by_name()["p8"]
    tag, _off, specs = case.walk("wrap")[0]
    batch = W.Batch(case, "wrap", tag, specs)
    b = case.byz[0]
    keys = [dict(t=1 + j, kind=L.INJ_KEY, instance=2, node=b, kp=b, s=0, value=1) for j in range(8192)]
    with R.open_batch([dict(sp, actions=[], step_cap=9000) for sp in specs], event_capacity=LOG, **case.open_kw()) as eng:
        eng.inject(keys)
        with pytest.raises(L.EngineError) as err:
            eng.run()
        assert err.value.code == L.E_STATE and "slot generation budget exhausted" in str(err.value), str(err.value)
        assert all(r["t_now"] == 0 for r in eng.instances_result())
        eng.reset()
        st, ev = run_epoch(eng, batch, LOG)
        assert not oracle_mismatches(batch, st, ev)


@pytest.mark.parametrize("cap", (LOG, 0), ids=("log", "nolog"))
@pytest.mark.parametrize("kind", sorted(W.slowset4_specs()))
def test_n4_slowset_fresh_engine_equals_oracle(kind, cap):
    """n = 4 under slow-set delays on a fresh engine, 16 instances in one wave item and three in the next.  The
    NPAD 4 kernel took the slow lanes of the NEXT instance of the item for senders of this one (its 8-bit link
    masks kept bits 4 .. 7 of the shifted ballot): arrivals came out too high wherever neighbours had slow replicas."""
    from oracle import oracle
    from tests import golden_io
    R = _runner()
    specs = W.slowset4_specs()[kind]
    if cap:
        got = R.run_batch(specs, event_capacity=cap)
    else:
        st = R.run_batch_noevents(specs)
        got = st["inst"]
    bad = []
    for sp, r in zip(specs, got):
        exp = oracle.run(sp)
        bad += [(sp["name"], k, r[k], exp[k]) for k in W.I.CKEYS if r[k] != exp[k]]
        if cap and r["events"] != golden_io.canonical_events(exp["events"]):
            bad.append((sp["name"], "events"))
        if not cap and r["deliveries"] != exp["counts"]["deliver"]:
            bad.append((sp["name"], "deliveries", r["deliveries"], exp["counts"]["deliver"]))
    assert not bad, bad[:8]
