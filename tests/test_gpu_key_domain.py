"""64-bit seeds, coin seeds and global instance ids on every device call site of the Philox draw, against the C oracle.

Every random quantity of a run is draw(seed, g, a, purpose, b) of csrc/schedule.h: the key carries (seed_lo, seed_hi), the
counter (g_lo, g_hi), g = inst_offset + inst.  brc_step.h, brc_step_wide.h, brc_life.h and brc_life_wide.h each compute g
themselves and hoist Philox state in their own way, the packed kernels hold 2 to 16 instances with different g in one
wave, and every other GPU test passes seeds below 2^32 and ids near 777: key word k1 and counter word c1 are zero in every
launch they make.  tests/key_domain_workloads.py has fifteen families (one per draw site and way of holding g) in four
placements of the high bits -- seed-hi, g-hi, carry (the 2^32 boundary inside one wave item) and top (bit 63 of seed
and id) --; tests/test_key_domain_workloads.py proves on the oracle that each batch does real work and that the batch
a kernel computes after losing a high word (the low-word twin) gives another result.

Per batch, bit-exact and nothing excluded: the engine equals the oracle on every instance (status, t_stop, msgs_sent,
arrivals, cell_steps, deliveries, every honest replica's decide count, first decision and last value, decided), its
round_histogram(66) and decisions() equal the oracle's decide rows, and it differs from its low-word twin run on the
device (the precondition seen on the device: a test that silently built the twin would fail here).  A carry batch
also equals, record for record, two fresh engines created on either side of the boundary.  The lifetime families are
held to their kernel with last_kernel().

One family per kernel file runs again with an event log in placement g-hi (the EV = true builds; the key-lifetime
kernels take no log, so their batch runs again on the step kernel): state-identical, and the sorted DELIVER / DECIDE /
SEND lists equal the oracle's.  One engine per kernel file is re-keyed 777 -> 3 * 2^32 + 777 -> 2^64 - 100 -> 777 with
brc_reset_at and must equal fresh engines created there.

A result that equals the twin's names the lost word (the failure message says which twin it equals); a carry batch that
equals the engines created at the wrapped ids names the carry.

Wall time on an MI355X: 14 s for the 68 tests (60 batches with their twins, four event-log runs, four re-keyed
engines), the oracle runs of the n = 129 and n = 130 batches included.
"""
import pytest

from tests import fault_bound_workloads as F
from tests import key_domain_workloads as K
from tests import step_noevent_workloads as T
from tests.state_compare import oracle_mismatches, state_mismatches

pytestmark = pytest.mark.gpu

BATCHES = K.batches()
LOG = 1 << 21


def _runner():
    from tests import engine_runner
    return engine_runner


def _open(batch, specs=None, event_capacity=0, on_step=False):
    """The engine of a batch (or of a run of its specs), inputs in place, not yet run.  on_step: the key-lifetime
    families on the step kernel (BRC_KERNEL=step; an unflagged engine above 64), which takes an event log."""
    R = _runner()
    fam = batch.family
    specs = batch.specs if specs is None else specs
    pattern = fam.kind == "pattern"
    if fam.kind in ("step", "life") or on_step:
        return R.open_batch(specs, event_capacity=event_capacity, proposals=batch.run["proposals"], byz_pattern=pattern,
                            key_window=fam.q, kernel="step" if on_step else fam.kind)
    from byzantinerandomizedconsensus_amd import _lib as L
    from byzantinerandomizedconsensus_amd.engine import Engine
    from tests import wide_records_runner
    eng = Engine(wide_life=True, life_pattern=pattern, byz_pattern=L.BYZ_EQUIVOCATE if pattern else L.BYZ_NONE,
                 proposals=L.PROPOSALS_LOADED if batch.loaded else L.PROPOSALS_PHILOX,
                 **wide_records_runner.engine_kw(specs, event_capacity, fam.q))
    try:
        if batch.loaded:
            eng.load_proposals(R._loaded_proposals(specs))
    except Exception:
        eng.close()
        raise
    return eng


def _kernel(batch, on_step=False):
    return "step" if batch.family.kind == "step" or on_step else "life"


def _run(batch, specs=None, **kw):
    with _open(batch, specs, **kw) as eng:
        assert eng.cfg.instance_offset == (batch.specs if specs is None else specs)[0]["g"]
        eng.run()
        assert eng.last_kernel() == _kernel(batch, kw.get("on_step", False)), (batch.label, eng.last_kernel())
        return _runner().read_state(eng, batch.specs)


def _records(st, lo=0, hi=None, packed=False):
    """The per-instance and per-replica records of instances lo .. hi - 1.  packed: without t_now, the engine time of
    the instance's wave item (include/brc.h), which on the packed kernels follows the instances it shares the item
    with -- the engines on either side of the boundary pack other instances together."""
    inst = [{k: v for k, v in r.items() if not (packed and k == "t_now")} for r in st["inst"][lo:hi]]
    return {"inst": inst, "reps": st["reps"][lo:hi], "hist": None, "dec": None, "stats": {}}


def _strip(st):
    """lane_loads and max_t count a kernel's own work (tests/test_gpu_life.py)."""
    return dict(st, stats={k: v for k, v in st["stats"].items() if k not in ("lane_loads", "max_t")})


def read_side_mismatches(batch, st):
    """round_histogram(66) and decisions() against the oracle's decide rows (every instance is compared)."""
    res = T.oracle_results(batch)
    assert len(res) == batch.count
    hist, counts, undecided, dis = F.expected_read_side(batch, res)
    want = {label: counts.get(v, 0) for v, label in enumerate(("-1", "0", "1", "3"))}
    want["undecided"] = undecided
    out = []
    if st["hist"] != hist:
        out.append(("oracle", "round_histogram", st["hist"], hist))
    if st["dec"] != (want, dis):
        out.append(("oracle", "decisions", st["dec"], (want, dis)))
    return out


@pytest.mark.parametrize("label", [b.label for b in BATCHES])
def test_batch_equals_oracle_and_differs_from_its_low_word_twin(label):
    b = K.by_label()[label]
    fam = b.family
    st = _run(b)
    s = st["stats"]
    print(label, K.INTENDED[fam.name], "kernel", _kernel(b), "instances compared", len(T.oracle_results(b)), "of", b.count,
          {k: s[k] for k in ("done", "quiescent", "stepcap", "overflow", "decided", "max_t")})
    assert s["running"] == 0 and s["overflow"] == 0 and s["instances"] == b.count, (label, s)
    vs_oracle = oracle_mismatches(b, st) + read_side_mismatches(b, st)
    equals = []
    if b.placement == "carry":
        c = fam.c
        (what, twin), = b.twins
        below, above = _run(b, b.specs[:c]), _run(b, b.specs[c:])
        wrapped = _run(twin, twin.specs[c:])                       # the ids a lost carry gives: 0, 1, ...
        pk = fam.npad < 64
        split = (state_mismatches(_records(st, 0, c, pk), _records(below, packed=pk), "first c instances vs an engine created below 2^32") +
                 state_mismatches(_records(st, c, None, pk), _records(above, packed=pk), "the others vs an engine created at 2^32"))
        if not state_mismatches(_records(st, c, None, pk), _records(wrapped, packed=pk), ""):
            equals.append("an engine created at id 0: the carry into g_hi is lost")
        shown = state_mismatches(_records(above, packed=pk), _records(wrapped, packed=pk), "engine at 2^32 vs engine at 0")
        assert not vs_oracle and not split and not equals, (label, vs_oracle[:6], split[:6], equals)
        assert shown, (label, "the engines at 2^32 and at 0 give one result: nothing is shown")
        return
    for what, twin in b.twins:
        low = _run(twin)
        if not state_mismatches(st, low, what):
            equals.append("its twin with " + what)
    assert not vs_oracle, (label, vs_oracle[:8], "equals", equals)
    assert not equals, (label, "the batch equals", equals)


@pytest.mark.parametrize("kernel_file", sorted(K.PER_KERNEL_FILE))
def test_event_log_twin_equals_the_batch_and_the_oracles_event_lists(kernel_file):
    R = _runner()
    b = K.by_label()[K.PER_KERNEL_FILE[kernel_file] + "-g-hi"]
    free = _run(b)
    on_step = b.family.kind != "step"
    with _open(b, event_capacity=LOG, on_step=on_step) as eng:
        eng.run()
        assert eng.last_kernel() == "step"
        twin = R.read_state(eng, b.specs)
        events = [R.sort_result({"events": ev})["events"] for ev in R.instance_events(eng.events(), b.specs)]
    assert twin["stats"]["events_dropped"] == 0 and twin["stats"]["running"] == 0, (kernel_file, twin["stats"])
    diff = (state_mismatches(_strip(free), _strip(twin), "lifetime kernel vs step kernel with an event log") if on_step
            else state_mismatches(free, twin, "event-free vs twin"))
    diff += oracle_mismatches(b, twin) + read_side_mismatches(b, twin)
    assert not diff, (kernel_file, b.label, diff[:8])
    for i, (exp, _dec, _n) in F.oracle_results(b).items():
        for k in ("deliver", "decide", "send"):
            assert events[i][k] == exp["events"][k], (kernel_file, b.label, i, k, len(events[i][k]), len(exp["events"][k]))


@pytest.mark.parametrize("kernel_file", sorted(K.PER_KERNEL_FILE))
def test_reset_at_across_the_high_words_equals_fresh_engines(kernel_file):
    """One engine, created at 777: run, reset_at(3 * 2^32 + 777), run, reset_at(2^64 - 100), run, reset_at(777), run.
    Runs 2 and 3 equal fresh engines created at those offsets, run 4 equals run 1, and Engine.cfg.instance_offset reads
    back the value passed."""
    R = _runner()
    fam = K.family(K.PER_KERNEL_FILE[kernel_file])
    at = {off: K.consecutive(fam, fam.lo, K.CLO, off, fam.count) for off in (K.OFFSET, K.G_HI, K.TOP)}
    fresh = {off: _run(x) for off, x in at.items()}
    for a, b in ((K.OFFSET, K.G_HI), (K.G_HI, K.TOP), (K.OFFSET, K.TOP)):
        assert state_mismatches(fresh[a], fresh[b], ""), (kernel_file, a, b, "two id ranges give one result: nothing is shown")
    runs = []
    with _open(at[K.OFFSET]) as eng:
        assert eng.cfg.instance_offset == K.OFFSET
        for off in (None, K.G_HI, K.TOP, K.OFFSET):
            if off is not None:
                eng.reset_at(off)
                assert eng.cfg.instance_offset == off == int(eng.cfg.instance_offset)
            eng.run()
            assert eng.last_kernel() == _kernel(at[K.OFFSET])
            runs.append(R.read_state(eng, at[K.OFFSET].specs))
    for got, want, what in ((runs[0], fresh[K.OFFSET], "first run vs fresh engine"),
                            (runs[1], fresh[K.G_HI], "reset_at(3 * 2^32 + 777) vs fresh engine"),
                            (runs[2], fresh[K.TOP], "reset_at(2^64 - 100) vs fresh engine"),
                            (runs[3], runs[0], "reset_at(777) vs the first run")):
        diff = state_mismatches(want, got, what)
        assert not diff, (kernel_file, diff[:8])
