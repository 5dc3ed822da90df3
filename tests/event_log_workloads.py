"""Workload table of tests/test_gpu_event_log.py (GPU) and tests/test_event_log_workloads.py (its preconditions, on
the oracle alone): batches whose whole event log -- every brc_event field, the value id and the BRC_EV_COPY records
included -- is held to the oracle's broadcast rows (oracle.run(..., kinds=(..., "broadcasts"))).

A case: name, kind ("storm" / "value"), batches (lists of specs in harness format, tests/golden/specs.py; the specs of
one batch share a configuration and have consecutive global ids), opener (how test_gpu_event_log opens a batch:
"batch" engine_runner.open_batch, "flagged" wide_records_runner.open_flagged, "values" an engine created with
BRC_FLAG_WIDE_VALUES and loaded proposals) and open_kw(), the opener's keywords.

Storm cases: specs._kat's K4 scaled up under connection-identity peers (core/brbroadcast.py:69).  Node 0 and the
replicas above the coalition are honest; the coalition (replicas 1 .. B) READYs a key of Byzantine origin 1, four
READYs per step in an order drawn per instance, and three of those READYs are injected again one step later (the
repeated injected broadcast: a COPY event).  Every honest replica then holds more than f READYs and no ECHO entry, so
each further READY makes it broadcast READY again (:118-119) until its 2f + 1-th delivers: most of the log is COPY
records.  One case per connection-kernel NPAD class (n strictly inside the pad), constant delay 1 or the slow-set
schedule with D = 4, IPW = 64 / NPAD instances per wave: 3 IPW + 1 instances on the packed kernels from global id
777, 5 at NPAD 64, 3 on the wide kernels.  Two cases have a sender-peer twin, whose log must hold no COPY record.

Value cases: existing spec builders.  One tests/step_noevent_workloads.py case per (kernel, NPAD, MODE, NLR / WV)
(any DM: the log call does not depend on it; the BRB batches where the table has one, else the smallest n), cut to the
longest prefix of its instances whose events number less than 2^17; values8_specs() in both peer modes;
general_keys_specs() (n = 40); one wide_values_workloads batch (ids 4 .. 7), one wide_xsend_workloads and one
restricted_msg_wide_workloads batch (SEND events logged from records); cons_equivocate_n16 / cons_equivocate4_n16
(2 and 4 key variants); a SPEC consensus batch at n = 70 whose first round ends in the common coin; cons_deliver_n6
(direct deliver() calls).
"""
import random

from tests import step_noevent_workloads as T
from tests.golden import specs as S

OFFSET = T.OFFSET
LIMIT = 1 << 17                          # events of one case (all batches)
RING_MAX = 255                           # csrc/brc_internal.h: one byte counts a cell's sends of one type in one step
COIN = 0xC017C01C                        # the two instances of the SPEC case draw different coins in round 1
CONST, SLOW = T.CONST, T.SLOW
KINDS = ("deliver", "decide", "send", "broadcasts")


class Case:
    def __init__(self, name, kind, make, opener="batch", kw=None, three_bit=False, twin_of=None):
        self.name, self.kind, self._make, self.opener, self.kw = name, kind, make, opener, dict(kw or {})
        self.three_bit, self.twin_of = three_bit, twin_of
        self._batches = None

    @property
    def batches(self):
        if self._batches is None:
            self._batches = [list(b) for b in self._make()]
            assert all(sp["g"] == b[0]["g"] + i for b in self._batches for i, sp in enumerate(b))
        return self._batches

    @property
    def specs(self):
        return [sp for b in self.batches for sp in b]

    @property
    def connection(self):
        return self.batches[0][0].get("peer_mode") == "connection"

    def open_kw(self):
        return dict(self.kw)


# ---- the oracle, once per spec -----------------------------------------------------------------------------------
_ORACLE = {}


def oracle_run(sp):
    """The oracle's run of sp with all four lists; decide rows carry value ids."""
    from oracle import oracle
    key = sp["name"]
    if key not in _ORACLE:
        _ORACLE[key] = oracle.run(dict(sp, values=None), kinds=KINDS)
    return _ORACLE[key]


def event_count(sp, exp):
    """Records the engine logs for sp: deliveries, decisions, first broadcasts and (connection peers) copies."""
    rows = exp["events"]["broadcasts"]
    sends = len(rows) if sp.get("peer_mode") == "connection" else sum(r[6] for r in rows)
    return exp["counts"]["deliver"] + exp["counts"]["decide"] + sends


def fitting_prefix(specs, budget=LIMIT - 1):
    """The longest prefix of specs (at least one) whose events number at most budget."""
    out, total = [], 0
    for sp in specs:
        total += event_count(sp, oracle_run(sp))
        if out and total > budget:
            break
        out.append(sp)
    return out


# ---- storm cases -------------------------------------------------------------------------------------------------
RATE = 4
#          n   f   coalition  model  dmax  instances
STORMS = ((7, 2, 6, CONST, 1, 25),
          (13, 4, 6, SLOW, 4, 13),
          (20, 6, 8, SLOW, 4, 7),
          (40, 13, 15, CONST, 1, 5),
          (70, 23, 26, SLOW, 4, 3),
          (130, 43, 46, CONST, 1, 3))
TWINS = (13, 70)


def storm_spec(n, f, nbyz, model, dmax, g, peer):
    seed = 0x570A0000 + n
    rng = random.Random(seed * 1000003 + g)
    byz = list(range(1, nbyz + 1))
    order = byz[:]
    rng.shuffle(order)
    seq = [(j // RATE, S.READY, b) for j, b in enumerate(order)]
    seq += [(t + 1, S.READY, b) for (t, _ty, b) in rng.sample(seq, 3)]
    name = "storm-n%d-%s" % (n, peer)
    sp = S._kat(n, f, sorted(seq), byz, key=(1, 0), name="storm-n%d" % n)
    sp["actions"][0]["value"] = g % 4                 # the key's value id: carried by every SEND / COPY / DELIVER
    return S.clone(sp, peer_mode=peer, g=g, seed=seed, delay_model=model, dmax=dmax, dconst=1,
                   name="%s/%d" % (name, g - OFFSET))


def _storms(out):
    for (n, f, nbyz, model, dmax, count) in STORMS:
        for peer in ("connection",) + (("sender",) if n in TWINS else ()):
            def make(a=(n, f, nbyz, model, dmax), count=count, peer=peer):
                return [[storm_spec(*a, OFFSET + i, peer) for i in range(count)]]
            out.append(Case("storm-n%d-%s" % (n, peer), "storm", make, kw=dict(proposals="inject", key_window=4),
                            twin_of=None if peer == "connection" else "storm-n%d-connection" % n))


# ---- value cases -------------------------------------------------------------------------------------------------
def instantiation_cases():
    """{(kernel, NPAD, MODE, NLR / WV): the step_noevent_workloads case taken for it}"""
    best = {}
    for c in T.cases():
        kernel, npad, _dm, mode, x = c.inst
        rank = (c.consensus, c.specs[0]["n"] if npad > 32 else 0, c.name)
        key = (kernel, npad, mode, x)
        if key not in best or rank < best[key][0]:
            best[key] = (rank, c)
    return {k: c for k, (_r, c) in best.items()}


def _groups(specs):
    """Batches of a golden group (engine_runner.run_specs' rule: one configuration, consecutive global ids)."""
    from tests.engine_runner import _cfg_key
    out = []
    for sp in specs:
        if out and _cfg_key(out[-1][-1]) == _cfg_key(sp) and out[-1][-1]["g"] + 1 == sp["g"]:
            out[-1].append(sp)
        else:
            out.append([sp])
    return out


def _named(group, specs):
    return [dict(sp, name=sp.get("name", "%s/%d" % (group, i))) for i, sp in enumerate(specs)]


def spec_coin_specs():
    """SPEC consensus at n = 70, f = 23 with Philox proposals: no value is proposed by more than (n + f) / 2 = 46.5
    replicas, so every phase-2 key of round 1 carries "-1", no value is counted and round 2 starts from the common
    coin (tests/test_event_log_workloads.py proves it on the oracle)."""
    return [dict(S.spec_cons_spec(70, 23, 0xE7C01070, SLOW, 4, OFFSET + i, round_cap=1, window=4, coin_seed=COIN),
                 name="spec-coin-n70/%d" % i) for i in range(2)]


W256_SPEC_WV4 = ("wide", 256, T.SPEC, 4)


def w256_spec_wv4_specs():
    """The table's one batch on brc_step_wide<256, *, true, SPEC, 4> is SPEC consensus at n = 129: 203,004 events in one
    instance.  This is SPEC broadcast at n = 130 on the same instantiation (slow-set delays up to 6: DM 8, two link
    delays, a carve below 40 KB -- tests/test_event_log_workloads.py checks step_noevent_workloads.instantiation)."""
    def make(g):
        rng = random.Random(0xE7256000 + g)
        sends = [(rng.randint(0, 3), o, 0) for o in rng.sample(range(129), 3) + [129]]
        return dict(S.spec_brb_spec(130, 43, 0xE7256130, SLOW, 6, g, sends, window=4), name="w256-brb-spec-x4/%d" % (g - OFFSET))
    return [make(OFFSET + i) for i in range(3)]


def _values(out):
    for key, c in sorted(instantiation_cases().items()):
        if key == W256_SPEC_WV4:
            out.append(Case("inst-w256-brb-spec-x4", "value", lambda: [w256_spec_wv4_specs()], kw=dict(proposals="inject", key_window=4)))
        else:
            out.append(Case("inst-" + c.name, "value", lambda c=c: [fitting_prefix(c.specs)], kw=c.open_kw()))
        out[-1].inst = key
    G8, GK = S.values8_specs(), S.general_keys_specs()
    for group, specs in sorted(G8.items()) + sorted(GK.items()):
        out.append(Case(group, "value", lambda group=group, specs=specs: _groups(_named(group, specs)),
                        kw=dict(proposals="inject"), three_bit=group.startswith(("cons_values", "conn_cons_values"))))

    def golden(group):
        return _groups(_named(group, S.scenario_groups()[group]))
    for group in ("cons_equivocate_n16", "cons_equivocate4_n16", "cons_deliver_n6"):
        out.append(Case(group, "value", lambda group=group: golden(group), kw=dict(proposals="inject")))

    def wide(module, name):
        import importlib
        return importlib.import_module("tests." + module).by_name()[name]
    out.append(Case("wv-128-maj", "value", lambda: [wide("wide_values_workloads", "wv-128-maj").specs], opener="values",
                    kw=dict(key_window=8, wide_records=False), three_bit=True))
    out.append(Case("xw-128-ref-unif", "value", lambda: [wide("wide_xsend_workloads", "xw-128-ref-unif").specs],
                    opener="flagged", kw=dict(key_window=4)))
    out.append(Case("rw-128-ref-cons", "value", lambda: [wide("restricted_msg_wide_workloads", "rw-128-ref-cons").specs],
                    opener="flagged", kw=dict(key_window=8)))
    out.append(Case("spec-coin-n70", "value", lambda: [spec_coin_specs()], kw=dict(proposals="philox", key_window=4)))


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        out = []
        _storms(out)
        _values(out)
        assert len({c.name for c in out}) == len(out)
        _CASES = out
    return _CASES


def by_name():
    return {c.name: c for c in cases()}


def names(kind=None):
    return [c.name for c in cases() if kind is None or c.kind == kind]


# the saturation cases of tests/test_gpu_event_log.py: a packed narrow batch (n = 7, 3 IPW + 1 instances), the lean
# n = 64 register-mask kernel, a wide 128 batch with sender peers, the n = 70 storm
def saturation_names():
    inst = instantiation_cases()
    return ("storm-n7-connection", "inst-" + inst[("step", 64, T.REF, 2)].name, "inst-" + inst[("wide", 128, T.REF, 0)].name,
            "storm-n70-connection")
