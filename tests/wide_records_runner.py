"""Engines created with BRC_FLAG_WIDE_RECORDS (Engine(wide_records=True)) for tests/test_gpu_restricted_msg_wide.py:
engine_runner.open_batch passes no such keyword, so the batch is opened here; the injections, the bulk read-out
and the interleaved driver are engine_runner's own."""
from byzantinerandomizedconsensus_amd import _lib as L
from byzantinerandomizedconsensus_amd.engine import Engine
from tests import engine_runner as R


def engine_kw(specs, event_capacity=0, key_window=None):
    sp0 = specs[0]
    assert all(R._cfg_key(sp) == R._cfg_key(sp0) and sp["g"] == sp0["g"] + i for i, sp in enumerate(specs))
    spec_mode = sp0["mode"] in ("spec", "spec_brb")
    if spec_mode:
        key_window = sp0["window"]
    elif key_window is None:
        key_window = sp0.get("key_window") or 8 // sp0.get("nv", 1)
    protocol = {"spec": "consensus", "spec_brb": "brb", "beb": "brb", "beb_consensus": "consensus"}.get(sp0["mode"], sp0["mode"])
    mode = L.MODE_SPEC if spec_mode else (L.MODE_BEB if sp0["mode"].startswith("beb") else L.MODE_REFERENCE)
    return dict(n=sp0["n"], f=sp0["f"], instances=len(specs), protocol=protocol, seed=sp0["seed"],
                delay_model=sp0["delay_model"], delay_max=sp0["dmax"], delay_const=sp0.get("dconst", 1),
                round_cap=sp0.get("round_cap", 0), step_cap=sp0.get("step_cap", 10000), key_window=key_window,
                variants=sp0.get("nv", 1), byzantine=sp0.get("byzantine", ()), event_capacity=event_capacity,
                instance_offset=sp0["g"], mode=mode, coin_seed=sp0.get("coin_seed", 0),
                peer_mode=L.PEER_CONNECTION if sp0.get("peer_mode") == "connection" else L.PEER_SENDER)


def injections(specs, garbage=None):
    """Every spec's injections; garbage(i, j): bits at and above n ORed into the j-th ECHO / READY of instance i."""
    out = []
    for i, sp in enumerate(specs):
        for j, x in enumerate(R._injections(sp, i)):
            if garbage is not None and x["kind"] == L.INJ_MSG:
                x = dict(x, dst=x["dst"] | garbage(i, j))
            out.append(x)
    return out


def open_flagged(specs, event_capacity=0, key_window=None, inject=True, garbage=None, wide_records=True):
    """The engine of one batch with the record kernels, the specs' actions injected (inject) but not yet run."""
    eng = Engine(wide_records=wide_records, **engine_kw(specs, event_capacity, key_window))
    try:
        if inject:
            eng.inject(injections(specs, garbage))
    except Exception:
        eng.close()
        raise
    return eng


def run_flagged(specs, event_capacity=0, key_window=None, garbage=None):
    """(read_state(), the event log per instance sorted canonically or None)."""
    with open_flagged(specs, event_capacity, key_window, garbage=garbage) as eng:
        eng.run()
        assert eng.last_kernel() == "step"
        st = R.read_state(eng, specs)
        if not event_capacity:
            return st, None
        return st, [R.sort_result({"events": ev})["events"] for ev in R.instance_events(eng.events(), specs)]


def run_flagged_interleaved(specs, policy, event_capacity=0, key_window=None, trace=None):
    with open_flagged(specs, event_capacity, key_window, inject=False) as eng:
        return R.drive_interleaved(eng, specs, policy, (), trace)
