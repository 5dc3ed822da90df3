"""Workload table of tests/test_gpu_key_layout.py (GPU) and tests/test_key_layout_workloads.py (its preconditions,
on the oracle alone): the run-time key-slot layout -- key window Q x key variants NV -- on every kernel family.

Every kernel addresses a key slot as (origin * NV + variant) * Q + (s & (Q - 1)); brc_step.h, brc_step_wide.h and
brc_life.h derive qsh, Qm and ksh = log2(Q) + log2(NV) from the two run-time parameters, the consensus passes fold
an origin's G = Q * NV consecutive slots, and SPEC switches its per-phase `seen` host masks on only when NV > 1.
The instantiation tables (step_noevent_workloads, typed_list_workloads, life_window_workloads) hold Q and NV still;
this one varies them on a few instantiations per family.

Case, instantiation() and the oracle cache are step_noevent_workloads' own.  A case adds: family ("packed", "lean",
"general64", "wide", "life", "pattern"), q, nv, split (None: no Byzantine actions) and kernel ("step" / "life").
accepted() restates which (Q, NV) brc_create takes (csrc/brc_engine.hip, csrc/brc_internal.h).

Byzantine actions: specs.variant_actions (every variant of an origin declared, SENT to disjoint destinations,
ECHOed and READYed to everyone), split "even" or "skewed".

The engine's own window limit: the reference protocol's phase leakage overruns a small window (BRC_OVERFLOW), which
the oracle does not model for REFERENCE and BEB.  At Q = 2 those modes run the broadcast protocol: honest SENDs with
sequence numbers 0 .. Q - 1 of three origins, so every slot of the window is in use, plus the variant keys.
"""
from tests import step_noevent_workloads as T
from tests.golden import specs as S

Case = T.Case
OFFSET = T.OFFSET
COIN = T.COIN
REF, SPEC, BEB, CONN, XREF = T.REF, T.SPEC, T.BEB, T.CONN, T.XREF
CONST, UNIF, SLOW, GEO = T.CONST, T.UNIF, T.SLOW, T.GEO
MODE_NAMES = T.MODE_NAMES
WINDOWS = (2, 4, 8, 16, 32, 64, 128)


# ---- brc_create's rules (csrc/brc_engine.hip, csrc/brc_internal.h) ----------------------------------
def cons_words(spec, msize, q, nv, nval=4):
    return (q * 64 * (msize if nv > 1 else 0) + q * 64 * 4 + 7) // 8 if spec else (nval * 64 * msize + 7) // 8


def lds_bytes_per_wave(npad, nk, nl, spec, q, nv, rs, lean, typed):
    """lds_bytes_per_wave() of brc_internal.h (WPB = 1, BRC_PSEG = 0, KPAD = 8, INJ_CACHE = 16)."""
    ipw = 64 // npad
    nkw = (nk + 63) // 64
    msize = 1 if npad <= 8 else npad // 8
    h_words = cons_words(spec, msize, q, nv, 4 if lean else 8)
    l_words = (nl * 64 * msize + 7) // 8
    klist_u16 = (nk + 16 + (36 if typed else 0)) * (2 if lean and not spec else 1)
    gen_words = 0 if lean else (ipw * nk + 3) // 4
    dbits_words = 0 if lean and spec else 64 * nkw
    injc_words = 0 if lean else 48
    return 8 * (ipw * nk + rs * nkw * (2 if lean else 1) + dbits_words + h_words + l_words + gen_words +
                (klist_u16 + 3) // 4 + injc_words)


def lds_bytes_life(nk, spec, q, nv, perlink):
    """lds_bytes_life() of brc_internal.h (life_hbm_meta: two-class form at Q >= 32)."""
    if not perlink and q >= 32:
        return 4 * 128 + 16 * 32 + 16 * ((nk + 63) // 64) + 8 * cons_words(spec, 8, q, nv)
    return ((4 * nk + (0 if perlink else 2 * nk) + 7) & ~7) + 8 * cons_words(spec, 8, q, nv)


def accepted(sp, q, kernel="auto", events=False, proposals="philox", byz_pattern=False):
    """The kernel a fresh run of the spec launches under key window q ("step" / "life"), or None where brc_create
    returns BRC_E_INVALID.  kernel: BRC_KERNEL (tests/engine_runner sets it at n in 33..64 only)."""
    n, nv, model, dmax = sp["n"], sp.get("nv", 1), sp["delay_model"], sp["dmax"]
    conn = sp.get("peer_mode") == "connection"
    spec = sp["mode"] in ("spec", "spec_brb")
    beb = sp["mode"].startswith("beb")
    consensus = sp["mode"] in ("consensus", "spec", "beb_consensus")
    general = bool(sp.get("general_keys"))
    if q not in WINDOWS or nv not in (1, 2, 4) or q * nv > (128 if not spec and n <= 64 else 8):
        return None
    if (conn and (spec or beb)) or (n > 64 and spec and nv != 1) or (byz_pattern and nv < 2):
        return None
    if general and 32 < n <= 64 and not conn and (spec or beb):
        return None
    npad, dm = T.pick_npad(n), T.pick_dm(dmax)
    rs = 16 if dm <= 8 else 32
    wide = npad > 64
    nk = npad * nv * q
    nkw = (nk + 63) // 64
    nl = T.delay_values(model, dmax)
    general = general and npad == 64 and not conn
    regmask = npad == 64 and not conn and nl <= 2 and not general
    lean = npad == 64 and not conn and not general
    if wide:
        lds = T.lds_bytes_wide(npad, q, nv, model, dmax, spec, conn)
    else:
        typed = lean and not events and not beb
        lds = lds_bytes_per_wave(npad, nk, 0 if regmask else nl, spec, q, nv, rs, lean, typed)
    perlink = model in (UNIF, GEO)
    eligible = (npad == 64 and consensus and not general and proposals != "inject" and not events and not byz_pattern and
                dmax <= (16 if perlink else 8) and lds_bytes_life(nk, spec, q, nv, perlink) <= 160 * 1024 and
                not (perlink and q * nv > 32))
    big = lean and q * nv > 32
    if not wide and conn and lds > 160 * 1024 and eligible:
        big = True
    life = eligible and kernel != "step" and (kernel == "life" or conn or not perlink or big)
    if big and not life:
        return None
    if not big and ((wide and nkw > npad // 8) or lds > 160 * 1024):
        return None
    return "life" if life else "step"


def max_window(sp, nv, **kw):
    """The largest key window brc_create accepts for the spec's shape with nv variants on the step kernel."""
    ok = [q for q in WINDOWS if accepted(dict(sp, nv=nv), q, kernel="step", **kw) == "step"]
    return max(ok) if ok else None


# ---- specs ------------------------------------------------------------------------------------------------
BYZ = {7: [6], 16: [3, 15], 40: [0, 17, 39], 50: [0, 49], 64: [0, 31, 63], 70: [1, 64, 69], 130: [0, 65, 129]}
FAULTS = {7: 2, 16: 5, 40: 13, 50: 16, 64: 21, 70: 23, 130: 43}


def _delay_kw(model, dmax):
    return dict(dconst=dmax) if model == CONST else {}


def brb_window_spec(mode, n, seed, model, dmax, g, q, nv, byz, extra):
    """Broadcast only: three honest origins SEND sequence numbers 0 .. q - 1 (key kp = origin * nv), one per step."""
    honest = [o for o in range(n) if o not in byz]
    origins = (honest[0], honest[len(honest) // 2], honest[-1])
    sends = [(s + i, o, s) for i, o in enumerate(origins) for s in range(q)]
    kw = dict(byzantine=byz, extra=extra, **_delay_kw(model, dmax))
    if mode == BEB:
        sp = S.beb_spec(n, seed, model, dmax, g, sends, **kw)
    elif mode == SPEC:
        sp = S.spec_brb_spec(n, FAULTS[n], seed, model, dmax, g, sends, window=q, **kw)
    else:
        sp = S.brb_spec(n, FAULTS[n], seed, model, dmax, g, sends, peer_mode="connection" if mode == CONN else "sender", **kw)
    for a in sp["actions"]:
        if a["kind"] == "brb_send":
            a["kp"] = a["node"] * nv
    sp["nv"] = nv
    return sp


def cons_spec(mode, n, seed, model, dmax, g, q, nv, byz, extra, round_cap):
    kw = dict(byzantine=byz, nv=nv, extra=extra, **_delay_kw(model, dmax))
    if mode == XREF:
        return dict(S.cons_spec(n, FAULTS[n], seed, model, dmax, g, round_cap=round_cap, **kw), general_keys=True)
    return T._cons(mode, n, FAULTS[n], seed, model, dmax, g, round_cap, q, **kw)


# Replacements found on the GPU (the engine's BRC_OVERFLOW, which the oracle does not model under REFERENCE / BEB),
# with the reason: (family, mode, n, Q, NV) -> dict(delay=(model, dmax)) or dict(protocol="brb").
TUNED = {
    # the non-lean kernels keep a slot busy until its key's last ECHO / READY arrival (brc_step.h send_key_now), so at
    # Q = 2 a SPEC replica's key s finds the slot of s - 2 busy under slow-set delays: 9 of 25 (n = 7), 1 of 13
    # (n = 16) and 1 of 3 (n = 70) instances stopped with BRC_OVERFLOW on an MI355X, NV = 1 and NV = 4 alike.  In
    # lock-step (a constant delay) key s - 2 is quiet one phase before s is SENT.
    ("packed", "spec", 7, 2, 4): dict(delay=(CONST, 2)),
    ("packed", "spec", 7, 2, 1): dict(delay=(CONST, 2)),
    ("packed", "spec", 16, 2, 4): dict(delay=(CONST, 2)),
    ("packed", "spec", 16, 2, 1): dict(delay=(CONST, 2)),
    ("wide", "spec", 70, 2, 1): dict(delay=(CONST, 2)),
}

# Cells of the issue's grid no configuration reaches, derived from brc_create's rules.
UNREACHABLE = {
    ("packed", SPEC, "nv4-qmax"): "SPEC takes Q * NV <= 8: with NV = 4 the largest window is the smallest, Q = 2",
    ("lean", SPEC, "nv4-qmax"): "SPEC takes Q * NV <= 8: with NV = 4 the largest window is the smallest, Q = 2",
}


class KCase(T.Case):
    def __init__(self, name, family, mode, q, nv, split, kernel, make, count, run, consensus, constant, tags=()):
        sp = make(OFFSET)
        inst = T.instantiation(sp, q) if kernel == "step" else ("life", 64, T.pick_dm(sp["dmax"]), mode, 0)
        if sp.get("wide_records"):
            inst = inst[:4] + (0,)                   # the record instantiations: no WV = 4 form
        T.Case.__init__(self, name, inst, make, count, run, q, consensus=consensus, constant=constant)
        self.family, self.mode, self.q, self.nv, self.split, self.kernel, self.tags = family, mode, q, nv, split, kernel, set(tags)
        self._twin = None

    def other_split(self):
        """The same case with the other split of the Byzantine actions (None without actions)."""
        return self._twin() if self._twin else None


def _count(n):
    npad = T.pick_npad(n)
    return 5 if npad == 64 else (3 if n <= 70 else 2) if npad > 64 else 3 * (64 // npad) + 1


_SEQ = [0]


def _add(out, family, mode, n, q, nv, model, dmax, split=None, kernel="step", protocol=None, round_cap=1, tags=(), flags=None):
    """One case.  protocol None: the broadcast protocol at Q = 2 under REFERENCE / BEB / connection peers (the
    module docstring), consensus elsewhere."""
    _SEQ[0] += 1
    tune = TUNED.get((family, MODE_NAMES[mode], n, q, nv), {})
    model, dmax = tune.get("delay", (model, dmax))
    name = "%s-n%d-%s-q%dv%d-%s%d%s%s" % (family, n, MODE_NAMES[mode], q, nv, T.MODEL_NAMES[model], dmax,
                                          ("-" + split) if split else "",
                                          "-rec" if flags and flags.get("wide_records") else ("-" + protocol[:4]) if protocol else "")
    protocol = tune.get("protocol", protocol)
    if protocol is None:
        protocol = "brb" if (q == 2 and mode != SPEC and kernel == "step") else "consensus"
    seed = 0x4B1A0000 + 0x100 * _SEQ[0] + tune.get("bump", 0)
    byz = BYZ[n]

    def maker(split):
        extra = S.variant_actions(n, byz, nv, split) if split else []

        def make(g):
            if protocol == "brb":
                sp = brb_window_spec(mode, n, seed, model, dmax, g, q, nv, byz, extra)
            else:
                sp = cons_spec(mode, n, seed, model, dmax, g, q, nv, byz, extra, round_cap)
            return dict(sp, **(flags or {}))
        return make
    # consensus: the propose actions are the Philox draws (not injected); the variant actions are injected
    run = dict(proposals="inject" if protocol == "brb" else "philox")
    if kernel == "life":
        run["kernel"] = "life"
    case = KCase(name, family, mode, q, nv, split, kernel, maker(split), _count(n), run, protocol != "brb", model == CONST, tags)
    if split:
        other = "skewed" if split == "even" else "even"
        case._twin = lambda: KCase(name + "/" + other, family, mode, q, nv, other, kernel, maker(other), case.count, run,
                                   protocol != "brb", model == CONST)
    out.append(case)
    return case


def _probe(mode, n, model, dmax, general=False):
    """A spec of the shape, for accepted() / max_window()."""
    sp = dict(n=n, mode={SPEC: "spec", BEB: "beb_consensus"}.get(mode, "consensus"), delay_model=model, dmax=dmax,
              peer_mode="connection" if mode == CONN else "sender")
    if general:
        sp["general_keys"] = True
    return sp


def _packed(out):
    i = 0
    for n in (7, 16):
        for mode in (REF, SPEC, BEB, CONN):
            model, dmax = ((UNIF, 3), (SLOW, 4), (GEO, 5), (CONST, 2))[i % 4]
            cmodel, cdmax = (GEO, 3) if mode in (REF, CONN) else (model, dmax)    # consensus: step_noevent's TUNED note
            i += 1
            pr = _probe(mode, n, cmodel, cdmax)
            split = "skewed" if n == 16 else "even"
            _add(out, "packed", mode, n, 2, 4, model, dmax, split, tags=("nv4-q2",))
            q4, q2 = max_window(pr, 4, events=True, proposals="inject"), max_window(pr, 2, events=True, proposals="inject")
            if q4 > 2:
                _add(out, "packed", mode, n, q4, 4, cmodel, cdmax, "even" if n == 16 else "skewed", round_cap=2, tags=("nv4-qmax",))
            _add(out, "packed", mode, n, q2, 2, cmodel, cdmax, split, round_cap=2, tags=("nv2-qmax",))
            _add(out, "packed", mode, n, 2, 1, model, dmax, None, tags=("nv1-q2",))


def _lean(out):
    two = ((SLOW, 4), (CONST, 2), (SLOW, 6))
    per = ((UNIF, 3), (GEO, 3), (GEO, 5))
    i = 0
    for mode in (REF, SPEC, BEB):
        cells = [(2, 4, "nv4-q2"), (4, 2, "q4v2"), (2, 2, "q2v2")]
        if mode != SPEC:
            pr = _probe(mode, 40, SLOW, 4)
            cells += [(max_window(pr, 4, events=True), 4, "nv4-qmax"), (max_window(pr, 2, events=True), 2, "nv2-qmax")]
        for j, (q, nv, tag) in enumerate(cells):
            form = (i + j) % 2                        # every mode runs both delay forms along its cells
            model, dmax = (two, per)[form][(i + j) % 3]
            if form and q > 2 and mode == REF:
                model, dmax = GEO, 3
            n = (40, 64)[(i + j // 2) % 2] if mode != SPEC else (40, 64, 40)[j]    # (the Python model's time at n = 64)
            split = ("skewed", "even")[j % 2] if n == 40 else ("even", "skewed")[j % 2]
            _add(out, "lean", mode, n, q, nv, model, dmax, split, tags=(tag, "perlink" if form else "twoclass"))
        i += 1


def _general64(out):
    pr = _probe(XREF, 40, SLOW, 4, general=True)
    _add(out, "general64", XREF, 40, 2, 4, SLOW, 4, "skewed", flags=dict(general_keys=True), tags=("nv4-q2",))
    _add(out, "general64", XREF, 40, max_window(pr, 4, events=True, proposals="inject"), 4, GEO, 3, "even",
         flags=dict(general_keys=True), tags=("nv4-qmax",))
    pc = _probe(CONN, 50, GEO, 3)
    _add(out, "general64", CONN, 50, 2, 4, UNIF, 3, "even", tags=("nv4-q2",))
    _add(out, "general64", CONN, 50, max_window(pc, 4, events=True, proposals="inject"), 4, GEO, 3, "skewed", tags=("nv4-qmax",))


def _wide(out):
    i = 0
    for mode in (REF, BEB, CONN):
        for (q, nv, tag) in ((2, 4, "nv4-q2"), (2, 2, "q2v2"), (4, 2, "q4v2")):
            n = (70, 130)[i % 2]
            model, dmax = ((SLOW, 4), (CONST, 1), (UNIF, 3), (SLOW, 8), (GEO, 3))[i % 5]
            if q > 2 and mode in (REF, CONN) and model == UNIF:
                model = GEO
            _add(out, "wide", mode, n, q, nv, model, dmax, ("skewed", "even")[(i // 2) % 2], tags=(tag,))
            i += 1
    _add(out, "wide", REF, 70, 2, 4, SLOW, 4, "skewed", protocol="consensus", tags=("nv4-q2", "delivered"))
    _add(out, "wide", REF, 70, 2, 4, SLOW, 6, "even", flags=dict(wide_records=True), tags=("nv4-q2", "records"))
    _add(out, "wide", SPEC, 70, 2, 1, SLOW, 4, None, round_cap=2, tags=("spec-q2v1",))
    _add(out, "wide", SPEC, 130, 2, 1, CONST, 1, None, protocol="brb", tags=("spec-q2v1",))   # (the Python model's time)


def _life(out):
    i = 0
    for mode in (REF, CONN):
        for q in (2, 16, 32):
            n = (40, 64, 50)[i % 3]
            model, dmax = ((CONST, 2), (SLOW, 5), (SLOW, 8))[i % 3]
            _add(out, "life", mode, n, q, 4, model, dmax, None, kernel="life", round_cap=(1, 3, 4)[i % 3],
                 tags=("nv4-q%d" % q, "twoclass"))
            i += 1
        _add(out, "life", mode, (64, 40)[mode == CONN], 2, 4, GEO, 3, None, kernel="life", tags=("nv4-q2", "perlink"))
    _add(out, "life", SPEC, 40, 2, 4, SLOW, 4, None, kernel="life", round_cap=2, tags=("nv4-q2", "twoclass"))
    _add(out, "life", SPEC, 50, 2, 4, UNIF, 3, None, kernel="life", round_cap=2, tags=("nv4-q2", "perlink"))


def _pattern(out):
    """BRC_BYZ_EQUIVOCATE with variants = 4: the engine's own pattern (expand_equivocate takes nv) against the oracle
    fed specs.equivocation_actions(n, byz, nv=4) -- two of the four variants of every Byzantine origin carry keys.
    n = 70 takes Q = 2 only (Q * NV <= 8): under slow-set delays up to 4 the reference protocol's phase leakage stopped
    1 of 3 instances with BRC_OVERFLOW on an MI355X, so that batch runs in lock-step (constant delay 1)."""
    for n, mode, model, dmax, q in ((16, SPEC, UNIF, 4, 2), (16, REF, UNIF, 2, 4), (40, REF, SLOW, 4, 4), (70, REF, CONST, 1, 2)):
        _SEQ[0] += 1
        seed = 0x4B1A0000 + 0x100 * _SEQ[0]
        byz = BYZ[n] if n != 16 else [12, 13, 14, 15]

        def make(g, n=n, mode=mode, model=model, dmax=dmax, q=q, seed=seed, byz=byz):
            return cons_spec(mode, n, seed, model, dmax, g, q, 4, byz, S.equivocation_actions(n, byz, nv=4), 1)
        name = "pattern-n%d-%s-q%dv4" % (n, MODE_NAMES[mode], q)
        out.append(KCase(name, "pattern", mode, q, 4, "pattern", "step", make, _count(n),
                         dict(proposals="philox", byz_pattern=True), True, False, ("nv4",)))


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        out = []
        _SEQ[0] = 0
        for part in (_packed, _lean, _general64, _wide, _life, _pattern):
            part(out)
        assert len({c.name for c in out}) == len(out), sorted(c.name for c in out)
        _CASES = out
    return _CASES


def by_name():
    return {c.name: c for c in cases()}


def engine_flags(case):
    """Engine keywords the specs carry beyond engine_runner's (BRC_FLAG_WIDE_RECORDS)."""
    return bool(case.specs[0].get("wide_records"))


# ---- the oracle, once per spec, every event list ------------------------------------------------------------
_EVENTS = {}


def oracle_events(case):
    """{local id: the oracle's deliver / decide / send lists, sorted canonically} of the compared ids.  Fills
    step_noevent_workloads' cache, so state_compare.oracle_mismatches runs the oracle no second time."""
    import concurrent.futures

    from oracle import oracle
    from tests import golden_io
    ids = case.oracle_ids()
    todo = [i for i in ids if (case.name, i) not in _EVENTS]
    if todo:
        with concurrent.futures.ThreadPoolExecutor(min(8, len(todo))) as ex:
            outs = list(ex.map(lambda i: oracle.run(case.specs[i]), todo))
        for i, exp in zip(todo, outs):
            dec = {}
            for t, node, rnd, val in sorted(exp["events"]["decide"]):
                dec.setdefault(node, []).append((rnd, t, T.VID[val]))
            T._ORACLE[(case.name, i)] = (exp, dec, exp["counts"]["deliver"])
            _EVENTS[(case.name, i)] = golden_io.canonical_events(exp["events"])
    return {i: _EVENTS[(case.name, i)] for i in ids}
