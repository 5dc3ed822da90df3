"""Workload table of tests/test_gpu_step_noevent.py (GPU) and tests/test_step_noevent_workloads.py (its
preconditions, on the oracle alone): one small batch per event-log-free instantiation of the step
kernels, brc_step<NPAD, DM, false, MODE, NLR> (csrc/brc_step.h) and brc_step_wide<NPAD, DM, false, MODE, WV>
(csrc/brc_step_wide.h).  tests/engine_runner.run_batch always asks for an event log, so every parity test on
top of it launches the EV = true builds; bench.py and configs.py time the EV = false ones.

A case: name, specs (harness format, tests/golden/specs.py; consecutive global ids from OFFSET), how its
inputs reach the engine (run: the keywords of engine_runner.open_batch) and inst, the instantiation
brc_create's rules pick for it -- instantiation() restates those rules (pick_npad, pick_dm, regmask,
wide_wv4, KMODE_CONN, KMODE_XREF) and the LDS carve the wide_wv4 rule needs.

Shapes: the packed narrow kernels (IPW = 64 / NPAD instances per wave) run 3 IPW + 1 instances from global
id 777 (three full wave items and a tail item with one live segment, not aligned to IPW), NPAD = 64 runs
5 instances, the wide kernels 3.  n alternates between the pad and a size strictly inside it.
"""
import random

from tests.golden import specs as S

OFFSET = 777
COIN = 0xC017C017
REF, SPEC, BEB, CONN, XREF = 0, 1, 2, 3, 4          # MODE template arguments (KMODE_CONN = 3, KMODE_XREF = 4)
MODE_NAMES = {REF: "ref", SPEC: "spec", BEB: "beb", CONN: "conn", XREF: "xref"}
CONST, UNIF, SLOW, GEO = 0, 1, 2, 3
MODEL_NAMES = {CONST: "const", UNIF: "unif", SLOW: "slow", GEO: "geo"}


def full_set():
    """The 108 compiled EV = false instantiations (the launch tables of brc_step.h, brc_kern_64r.hip and
    brc_step_wide.h)."""
    out = set()
    for dm in (4, 8, 16):
        for mode in (REF, SPEC, BEB, CONN):
            for npad in (4, 8, 16, 32, 64):
                out.add(("step", npad, dm, mode, 0))
            for npad in (128, 256):
                out.add(("wide", npad, dm, mode, 0))
        out.add(("step", 64, dm, XREF, 0))
        for mode in (REF, SPEC, BEB):
            out.add(("step", 64, dm, mode, 2))
            if dm <= 8:
                for npad in (128, 256):
                    out.add(("wide", npad, dm, mode, 4))
    return out


# ---- brc_create's rules (csrc/brc_engine.hip, csrc/brc_internal.h) ----------------------------------
def pick_npad(n):
    p = 4
    while p < n:
        p *= 2
    return p


def pick_dm(d):
    return 4 if d <= 4 else 8 if d <= 8 else 16


def delay_values(model, dmax):
    return 1 if model == CONST else (2 if dmax > 1 else 1) if model == SLOW else dmax


def lds_bytes_wide(npad, q, nv, model, dmax, spec, conn):
    """lds_bytes_wide() of brc_internal.h (CHUNK_W = 4, BRC_WIDE_DCW = 2)."""
    dm = pick_dm(dmax)
    nk = npad * nv * q
    nkw = (nk + 63) // 64
    nw = npad // 64
    rs = 16 if dm <= 8 else 32
    planes = model in (UNIF, GEO)
    xw = 8 * delay_values(model, dmax) if conn else ({4: 2, 8: 3, 16: 4}[dm] + 1 if planes else delay_values(model, dmax))
    cons = (q * npad + 1) // 2 if spec else 4 * nw * npad
    return (8 * (nk + rs * nkw + min(nkw, 2) * npad + cons + 2 * 4 * xw * 2 * nw + 16 * nw)
            + q * npad + 8 * nkw + 2 * nk + 4 * (12 + 2 * 4 * nw))


def instantiation(sp, key_window):
    """(kernel, NPAD, DM, MODE, NLR or WV) brc_create picks for a spec run without an event log."""
    npad, dm = pick_npad(sp["n"]), pick_dm(sp["dmax"])
    conn = sp.get("peer_mode") == "connection"
    spec = sp["mode"] in ("spec", "spec_brb")
    mode = CONN if conn else SPEC if spec else BEB if sp["mode"].startswith("beb") else REF
    q = sp["window"] if spec else key_window
    nl = delay_values(sp["delay_model"], sp["dmax"])
    if npad > 64:
        wv4 = (dm <= 8 and sp["delay_model"] in (CONST, SLOW) and not conn and
               lds_bytes_wide(npad, q, sp.get("nv", 1), sp["delay_model"], sp["dmax"], spec, conn) <= 40 * 1024)
        return ("wide", npad, dm, mode, 4 if wv4 else 0)
    if npad == 64 and not conn:
        if sp.get("general_keys"):
            return ("step", 64, dm, XREF, 0)                 # e->general: KMODE_XREF
        return ("step", 64, dm, mode, 2 if nl <= 2 else 0)   # e->regmask: launch_step_64r
    return ("step", npad, dm, mode, 0)


# The wide_wv4 rule asks for an LDS carve of at most 40 KB.  Under REFERENCE and BEB the carve holds the host
# masks hm[4][NW][NPAD] u64 (cons_words_wide): 32 KB at NPAD = 256, and with the smallest key window (2) and
# one link delay the rest brings it to 44,784 B.  No configuration brc_create accepts reaches these four; the
# launch table of brc_step_wide.h compiles them all the same.
UNREACHABLE = {
    ("wide", 256, 4, REF, 4): "wide_wv4 needs lds_bytes <= 40 KB; REFERENCE at NPAD 256 carves >= 44,784 B",
    ("wide", 256, 8, REF, 4): "wide_wv4 needs lds_bytes <= 40 KB; REFERENCE at NPAD 256 carves >= 44,784 B",
    ("wide", 256, 4, BEB, 4): "wide_wv4 needs lds_bytes <= 40 KB; BEB at NPAD 256 carves >= 44,784 B",
    ("wide", 256, 8, BEB, 4): "wide_wv4 needs lds_bytes <= 40 KB; BEB at NPAD 256 carves >= 44,784 B",
}


def min_lds_wide_256(spec):
    """The smallest carve any accepted configuration gives at NPAD = 256 on the constant / slow-set models."""
    return min(lds_bytes_wide(256, q, 1, model, d, spec, False)
               for q in (2, 4, 8) for model, d in ((CONST, 1), (SLOW, 1), (SLOW, 8)))


# ---- the cases ---------------------------------------------------------------------------------------
N_INSIDE = {4: 3, 8: 7, 16: 13, 32: 31}
N_64 = (64, 50, 64, 37, 64, 45)
N_128 = (70, 96, 65, 81)
N_256 = (129, 140, 133)
DMAX = {4: (4, 3), 8: (8, 5, 7, 6), 16: (12, 16, 9, 14)}


def _cons(mode, n, f, seed, model, dmax, g, round_cap, q, **kw):
    if mode == SPEC:
        return S.spec_cons_spec(n, f, seed, model, dmax, g, round_cap=round_cap, window=q, coin_seed=COIN, **kw)
    if mode == BEB:
        return S.beb_cons_spec(n, f, seed, model, dmax, g, round_cap=round_cap, **kw)
    if mode == CONN:
        return S.cons_spec(n, f, seed, model, dmax, g, round_cap=round_cap, peer_mode="connection", **kw)
    return S.cons_spec(n, f, seed, model, dmax, g, round_cap=round_cap, **kw)


def _brb(mode, n, f, seed, model, dmax, g, sends, **kw):
    if mode == SPEC:
        return S.spec_brb_spec(n, f, seed, model, dmax, g, sends, window=4, **kw)
    if mode == BEB:
        return S.beb_spec(n, seed, model, dmax, g, sends, **kw)
    if mode == CONN:
        return S.brb_spec(n, f, seed, model, dmax, g, sends, peer_mode="connection", **kw)
    return S.brb_spec(n, f, seed, model, dmax, g, sends, **kw)


# Adjustments found on the oracle alone (tests/test_step_noevent_workloads.py's conditions).  The reference
# protocol ignores a SEND that arrives after an ECHO of its key (core/brbroadcast.py:74-82), so under per-link
# delays a replica whose link from the origin takes three steps or more never echoes: uniform delays up to 4
# stall every instance before its first decision, geometric ones most.  Where the instantiation allows it the
# case takes a two-class model, else a geometric schedule (and a fault bound) on which some instance decides.
TUNED = {
    # the engine's key window (BRC_OVERFLOW is its own limit, not the protocol's): both builds
    # stopped these two with it at the table's default window, as measured on an MI355X
    "n16-dm16-beb": dict(q=16),
    "n64-dm8-spec-x2": dict(q=8),
    "n4-dm4-ref": dict(model=GEO, dmax=3, f=1),
    "n4-dm4-beb": dict(model=GEO, dmax=3, f=1),
    "n4-dm8-conn": dict(model=GEO, dmax=5, f=1),
    "n4-dm16-ref": dict(model=GEO, dmax=9, f=1),
    "n4-dm16-beb": dict(model=GEO, dmax=9, f=1),
    "n8-dm4-conn": dict(model=GEO, dmax=3, f=2),
    "n8-dm8-conn": dict(model=GEO, dmax=5, f=2),
    "n8-dm16-conn": dict(model=GEO, dmax=9, f=2),
    "n16-dm4-conn": dict(model=GEO, dmax=3, f=5),
    "n16-dm8-conn": dict(model=GEO, dmax=5, f=4),
    "n16-dm16-conn": dict(model=GEO, dmax=9, f=5, bump=1),
    "n32-dm4-conn": dict(model=GEO, dmax=3, f=10),
    "n32-dm8-conn": dict(model=GEO, dmax=5, f=7),
    "n32-dm16-ref": dict(model=GEO, dmax=9, f=7),
    "n32-dm16-conn": dict(model=GEO, dmax=9, f=7),
    "n64-dm4-xref": dict(model=GEO, dmax=3, f=13),
    "n64-dm8-ref": dict(model=GEO, dmax=5, f=9),
    "n64-dm8-xref": dict(model=GEO, dmax=5, f=9),
    "n64-dm16-xref": dict(model=GEO, dmax=9, f=13, bump=1),
    "w128-dm8-ref": dict(model=GEO, dmax=5, f=23),
    "w128-dm8-conn": dict(model=GEO, dmax=5, f=21),
    "w128-dm16-conn": dict(model=GEO, dmax=9, f=21, bump=1),
    "w256-dm8-ref": dict(model=GEO, dmax=5, f=42),
    "w256-dm8-conn": dict(model=GEO, dmax=5, f=46),
    "w256-dm16-conn": dict(model=GEO, dmax=9, f=44),
}


class Case:
    def __init__(self, name, inst, make, count, run, key_window, consensus=True, constant=False):
        self.name, self.inst, self._make, self.count, self.run = name, inst, make, count, run
        self.key_window, self.consensus, self.constant = key_window, consensus, constant
        self._specs = None

    @property
    def specs(self):
        if self._specs is None:
            self._specs = [dict(self._make(OFFSET + i), name="%s/%d" % (self.name, i)) for i in range(self.count)]
        return self._specs

    def oracle_ids(self):
        """n <= 32: every instance; else the first, the last and one seeded id between them."""
        if self.specs[0]["n"] <= 32 or self.count <= 3:
            return list(range(self.count))
        return [0, random.Random("step-noevent/" + self.name).randrange(1, self.count - 1), self.count - 1]

    def open_kw(self):
        return dict(self.run, key_window=self.key_window)


def _case(cases, kernel, npad, dm, mode, x, idx, tune=None):
    """The consensus case meant for one instantiation; idx varies the shape choices along the table."""
    name = "%s%d-dm%d-%s%s" % ("w" if kernel == "wide" else "n", npad, dm, MODE_NAMES[mode], ("-x%d" % x) if x else "")
    two_class = x != 0                              # NLR 2 / WV 4: constant or slow-set delays
    dmax = DMAX[dm][idx % len(DMAX[dm])]
    if two_class:
        model = CONST if idx % 3 == 2 else SLOW
    else:
        model = GEO if idx % 2 else UNIF
        if npad == 64 and dmax < 3:
            dmax = 3                                # uniform delays up to 2 land on NLR 2
    if mode == XREF:
        n = 40
    elif npad <= 32:
        n = N_INSIDE[npad] if ((dm == 8) + mode) % 2 == 0 else npad     # every mode gets both along DM
    elif npad == 64:
        n = N_64[idx % len(N_64)]
    elif npad == 128:
        n = N_128[idx % len(N_128)]
    else:
        n = N_256[idx % len(N_256)]
    tune = TUNED.get(name, {}) if tune is None else tune
    model, dmax = tune.get("model", model), tune.get("dmax", dmax)
    f = tune.get("f", (n - 1) // 3)
    count = 5 if npad == 64 else 3 if npad > 64 else 3 * (64 // npad) + 1
    q = tune.get("q", (4, 8)[idx % 2] if mode == SPEC else 8)
    round_cap = (2, 1, 3)[idx % 3] if npad <= 64 else 1
    # silent replicas: the reference's phase end wants n - f + 1 deliveries, so at most f - 1 of them
    byz = []
    if idx % 3 == 1 and f >= 2:
        byz = [0, n - 1] if f >= 3 else [n - 1]
    loaded = idx % 5 == 3 and mode != XREF
    seed = 0x57E90000 + npad * 0x100 + dm * 0x10 + mode * 4 + x + 0x10000 * tune.get("bump", 0)
    kw = dict(byzantine=byz)
    if model == CONST:
        kw["dconst"] = dmax
    if mode == XREF:
        # general_keys_specs()-style inputs: five proposal strings (VALUES8 ids 1..5) at n = 40
        pats = [[4] * 30 + [1, 2, 3, 5] * 2 + [5, 5], [1, 2, 3, 4, 5] * 8, [5] * 29 + [1, 2, 3, 4] * 2 + [4, 3, 2]]

        def make(g, kw=kw):
            return dict(S.cons_spec(n, f, seed, model, dmax, g, round_cap=round_cap, proposals=pats[g % 3], **kw),
                        values=S.VALUES8, general_keys=True)
        run = dict(proposals="loaded")
    elif loaded:
        def make(g, kw=kw):
            rng = random.Random(seed * 1000003 + g)
            hi = 2 if mode == SPEC else 3          # SPEC proposes binary values ("0" / "1")
            return _cons(mode, n, f, seed, model, dmax, g, round_cap, q, proposals=[rng.randint(1, hi) for _ in range(n)], **kw)
        run = dict(proposals="loaded")
        name += "-loaded"
    else:
        def make(g, kw=kw):
            return _cons(mode, n, f, seed, model, dmax, g, round_cap, q, **kw)
        run = dict(proposals="philox")
    if byz:
        name += "-byz"
    cases.append(Case(name, (kernel, npad, dm, mode, x), make, count, run, q, constant=model == CONST))


def _equivocation(cases, mode):
    """cfg3's shape (configs.py times it in both protocols): n = 16, two key variants, five Byzantine
    replicas running the engine's own equivocation pattern (BRC_BYZ_EQUIVOCATE = specs.equivocation_actions)."""
    seed = 0x5EED0003
    # cfg3's own uniform delays up to 4 stall the reference protocol before any decision (TUNED's note), and
    # with f replicas equivocating only n - f keys deliver, one short of its phase end: delays up to 2 and
    # f - 1 Byzantine replicas there
    byz, dmax = (list(range(11, 16)), 4) if mode == SPEC else (list(range(12, 16)), 2)

    def make(g):
        return _cons(mode, 16, 5, seed, UNIF, dmax, g, 1, 4, byzantine=byz, nv=2, extra=S.equivocation_actions(16, byz))
    cases.append(Case("n16-dm4-%s-equivocate" % MODE_NAMES[mode], ("step", 16, 4, mode, 0), make, 13,
                      dict(proposals="philox", byz_pattern=True), 4))


def _brb_full(cases, npad, mode, idx):
    """BRB at n = NPAD: three or four SENDs (cheap on the oracle at n = 256), so the top waves' lanes carry
    real replicas.  Connection peers: test_gpu_parity.test_connection_brb_floods_vs_oracle's generator
    (Byzantine replicas re-send ECHO / READY of honest keys)."""
    n, f = npad, (npad - 1) // 3
    model, dmax = ((GEO, 4), (SLOW, 12), (GEO, 16), (SLOW, 6))[idx % 4]      # BEB runs with f = 0: no slow set
    seed = 0xB4B0000 + npad * 16 + mode
    allm = (1 << n) - 1

    byz = sorted(random.Random(seed).sample(range(n), 3)) if mode in (CONN, REF) else []

    def make(g):
        rng = random.Random(seed * 131 + g)
        honest = [o for o in range(n) if o not in byz]
        origins = rng.sample(honest[:-1], 3) + [honest[-1]] if g % 2 else rng.sample(honest[:-1], 2) + [honest[-1]]
        sends = [(rng.randint(0, 3), o, 0) for o in origins]
        extra = []
        if mode == CONN:
            for (t0, o, sq) in sends:
                for b in byz:
                    for _ in range(rng.randint(1, 3)):
                        extra.append(dict(t=t0 + rng.randint(0, 6), kind="byz", src=b, type=rng.choice([2, 3]),
                                          kp=o, s=sq, dst=allm))
        return _brb(mode, n, f, seed, model, dmax, g, sends, byzantine=byz, extra=extra)
    name = "w%d-brb-%s-%s%d" % (npad, MODE_NAMES[mode], MODEL_NAMES[model], dmax)
    sp = make(OFFSET)
    kwin = 4
    cases.append(Case(name, instantiation(sp, kwin), make, 3, dict(proposals="inject"), kwin, consensus=False))


_CASES = None


def cases():
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []
    idx = 0
    for inst in sorted(full_set() - set(UNREACHABLE)):
        idx += 1
        if inst in (("step", 16, 4, REF, 0), ("step", 16, 4, SPEC, 0)):
            _equivocation(out, inst[3])
            continue
        _case(out, *inst, idx)
    i = 0
    for npad in (128, 256):
        for mode in (REF, SPEC, BEB, CONN):
            _brb_full(out, npad, mode, i)
            i += 1
    assert len({c.name for c in out}) == len(out)
    _CASES = out
    return out


def by_name():
    return {c.name: c for c in cases()}


# ---- the oracle, once per spec -------------------------------------------------------------------------
_ORACLE = {}
VID = {v: i for i, v in enumerate(S.VALUES8)}       # VALUES is a prefix of VALUES8


def oracle_results(case):
    """{local id: (result, per replica [(round, t, value id) of every decide event], deliver count)} of the
    case's compared ids (threads: the C run releases the GIL)."""
    import concurrent.futures

    from oracle import oracle
    ids = case.oracle_ids()
    todo = [i for i in ids if (case.name, i) not in _ORACLE]
    if todo:
        with concurrent.futures.ThreadPoolExecutor(min(8, len(todo))) as ex:
            outs = list(ex.map(lambda i: oracle.run(case.specs[i], kinds=("decide",)), todo))
        for i, exp in zip(todo, outs):
            dec = {}
            for t, node, rnd, val in sorted(exp["events"]["decide"]):
                dec.setdefault(node, []).append((rnd, t, VID[val]))
            _ORACLE[(case.name, i)] = (exp, dec, exp["counts"]["deliver"])
    return {i: _ORACLE[(case.name, i)] for i in ids}


def link_delays(case):
    """The distinct link delays between the replicas of the case's compared instances."""
    from oracle.schedule import Schedule
    sp = case.specs[0]
    sch = Schedule(sp["n"], sp["f"], sp["seed"], sp["delay_model"], sp["dmax"], sp.get("dconst", 1))
    n = sp["n"]
    step = 1 if n <= 64 else 7                      # a sample of the links is enough at n > 64
    return {sch.delay(OFFSET + i, a, b) for i in case.oracle_ids()[:2] for a in range(0, n, step) for b in range(n)}
