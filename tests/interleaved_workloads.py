"""Workload table of tests/test_gpu_interleaved.py (GPU) and tests/test_interleaved_workloads.py (its
preconditions, on the oracle alone): small batches whose actions reach the engine in pieces, between sliced
brc_run calls (tests/engine_runner.drive_interleaved).  Every other parity test injects a batch's whole action
list before the first brc_run; network.Cluster.run is the one consumer that injects while the engine runs.

A case: name, family (one per kernel family, FAMILIES), inst (the step-kernel instantiation brc_create picks,
step_noevent_workloads.instantiation), specs (harness format, at most 8, consecutive global ids from 777, one
configuration, action lists that differ per instance), key_window, and what the policies need:

  marks   {instance: {T}} (at_now): every action of the instance stamped T stays on the host until the instance
          stands at T.  A case gives these actions without a time (late); T is the first step >= late_lo at which
          an honest replica of the instance ECHOes (best-effort broadcast: delivers) in the oracle's run WITHOUT
          them -- a step at which a SEND lands there.  Adding actions at T changes nothing before T's actions.
  bounds  {instance: [G]} (after_quiet): actions from G on form the next group; the oracle's run of the group
          before ends QUIESCENT before G.  packed: several instances per wave item, a sibling still runs then.

Inputs tuned on the oracle, as in step_noevent_workloads.TUNED: the reference protocol gets slow-set or geometric
delays (uniform ones stall it), BRB streams leave gap * Q steps between two sequence numbers of one slot.
"""
from tests import step_noevent_workloads as T
from tests.golden import specs as S

OFFSET = T.OFFSET
REF, SPEC, BEB, CONN, XREF = T.REF, T.SPEC, T.BEB, T.CONN, T.XREF
CONST, UNIF, SLOW, GEO = T.CONST, T.UNIF, T.SLOW, T.GEO
CKEYS = ("status", "t_stop", "msgs_sent", "arrivals", "cell_steps")
STEP_CAP = 600
XSEND_MAX, INJ_CACHE = 16, 16                      # csrc/brc_internal.h
FAMILIES = ("packed4", "packed8", "packed16", "packed32", "lean64r-ref", "lean64r-spec", "lean64r-beb", "lean64-ref",
            "lean64-spec", "lean64-beb", "general64", "conn64", "wide128", "wide256")
# what the action lists must hold between them (test_interleaved_workloads checks each on the expanded lists)
CONTENT = ("staggered-propose", "wrapping-stream", "byz-key-msg", "deliver", "restricted-send", "extra-send",
           "over-inj-cache", "restricted-hi")


def stream(origin, count, gap, t0=0, s0=0):
    """BRB sends of one origin, sequence numbers s0 .. s0 + count - 1, gap steps apart."""
    return [(t0 + j * gap, origin, s0 + j) for j in range(count)]


def byz_msgs(t, srcs, keys, n):
    """ECHO and READY of every key from every src (raw Byzantine messages to all peers), at step t."""
    allm = (1 << n) - 1
    return [dict(t=t, kind="byz", src=b, type=typ, kp=kp, s=s, dst=allm) for b in srcs for typ in (S.ECHO, S.READY)
            for (kp, s) in keys]


def restricted_send(t, b, s, dst, value=0):
    """Byzantine origin b declares key (b, s) and SENDs it to the replicas of dst only."""
    return [dict(t=t, kind="byz_key", kp=b, s=s, value=value), dict(t=t, kind="byz", src=b, type=S.SEND, kp=b, s=s, dst=dst)]


class Case:
    def __init__(self, name, family, inst, make, count, key_window, consensus, late=None, late_lo=2, bounds=None,
                 packed=False, byz=()):
        self.name, self.family, self.inst, self._make, self.count = name, family, inst, make, count
        self.key_window, self.consensus, self._late, self.late_lo = key_window, consensus, late or {}, late_lo
        self.bounds, self.packed, self.byz = bounds or {}, packed, list(byz)
        self._specs = self._marks = None

    def base_specs(self):
        """The specs without the at_now actions."""
        return [dict(self._make(OFFSET + i, i), name="%s/%d" % (self.name, i), step_cap=STEP_CAP) for i in range(self.count)]

    def _build(self):
        from oracle import oracle
        specs, marks = self.base_specs(), {}
        for i, acts in sorted(self._late.items()):
            exp = oracle.run(specs[i], kinds=("deliver", "send"))
            steps = sorted({e[0] for e in exp["events"]["send"] if e[2] == S.ECHO and e[1] not in self.byz} if self.inst[3] != BEB
                           else {e[0] for e in exp["events"]["deliver"]})
            t = next(x for x in steps if x >= self.late_lo)
            specs[i] = dict(specs[i], actions=specs[i]["actions"] + [dict(a, t=t) for a in acts])
            marks[i] = {t}
        self._specs, self._marks = specs, marks

    @property
    def specs(self):
        if self._specs is None:
            self._build()
        return self._specs

    @property
    def marks(self):
        if self._marks is None:
            self._build()
        return self._marks

    def policies(self):
        """{label: engine_runner policy}"""
        from tests import engine_runner as R
        out = {"look1": R.lookahead(1), "look3": R.lookahead(3)}
        if self._late:
            out["at_now"] = R.at_now(self.marks)
        if self.bounds:
            out["after_quiet"] = R.after_quiet(self.bounds, self.packed)
        return out

    def open_kw(self):
        return dict(key_window=self.key_window)

    def prefix_spec(self, i, j):
        """Instance i with its action groups 0 .. j only."""
        g = self.bounds[i][j]
        sp = self.specs[i]
        return dict(sp, actions=[a for a in sp["actions"] if a["t"] < g])


def _without_propose(sp, node):
    return dict(sp, actions=[a for a in sp["actions"] if not (a["kind"] == "propose" and a["node"] == node)])


def _propose(sp, node):
    return [{k: v for k, v in a.items() if k != "t"} for a in sp["actions"] if a["kind"] == "propose" and a["node"] == node]


def _early(acts):
    """deliver_actions with their times folded into steps 0 .. 4 (best-effort consensus is done within a dozen steps)."""
    return [dict(a, t=a["t"] % 5) for a in acts]


def _send(o, s=0):
    return [dict(kind="brb_send", node=o, kp=o, s=s, payload="TEST %d.%d" % (o + 1, s))]


def _build():
    out = []

    def add(*a, **kw):
        out.append(Case(*a, **kw))

    # ---- packed narrow kernels ---------------------------------------------------------------------------
    # NPAD 4 (16 instances per wave: the 8 share one item): reference consensus, proposals at staggered times,
    # direct deliver() calls; node 3 of instances 1 and 6 proposes at_now, node 3 of instance 3 after the
    # instance went quiet (n - f + 1 = 4 deliveries end a phase: without node 3 it stalls)
    def p4(g, i):
        starts = [0, g % 3, 1 + g % 2, 90 if i == 3 else 0]
        sp = S.cons_spec(4, 1, 0x17E40004, GEO, 3, g, round_cap=4, starts=starts, extra=S.deliver_actions(4, 0x17E4 + g, count=4))
        return _without_propose(sp, 3) if i in (1, 6) else sp
    add("p4-ref-cons", "packed4", ("step", 4, 4, REF, 0), p4, 8, 8, True,
        late={i: _propose(S.cons_spec(4, 1, 0x17E40004, GEO, 3, OFFSET + i), 3) for i in (1, 6)}, bounds={3: [90]}, packed=True)

    # NPAD 8 (8 per wave): SPEC broadcast, two streams per instance whose sequence numbers wrap the key window
    # (Q = 4, 10 to 12 numbers); instance 4 stops after five numbers and resumes at step 90
    def p8(g, i):
        cnt = 10 + g % 3
        sends = stream(g % 7, cnt, 4) + stream((g + 3) % 7, cnt, 4, t0=1)
        if i == 4:
            sends = stream(g % 7, 5, 4) + stream(g % 7, 4, 4, t0=90, s0=5)
        return S.spec_brb_spec(7, 2, 0x17E40008, UNIF, 4, g, sends, window=4)
    add("p8-spec-brb", "packed8", ("step", 8, 4, SPEC, 0), p8, 8, 4, False,
        late={i: _send((OFFSET + i + 5) % 7) for i in (2, 5)}, bounds={4: [90]}, packed=True)

    # NPAD 16 (4 per wave, 7 instances: a full item and a tail of three): reference broadcast with two Byzantine
    # replicas -- a restricted SEND, 20 ECHO / READY records in one step (more than INJ_CACHE), extra SENDs of
    # one key (3-bit-id kernel); every instance but 2 also runs a stream; instance 2 resumes at step 120
    def p16(g, i):
        n, byz = 13, [11, 12]
        sends = [(0, 0, 0), (1, 3, 0), (g % 3, 5, 0)] + (stream(9, 5, 12) if i != 2 else [])
        extra = [dict(t=1, kind="brb_send", node=2, kp=0, s=0, payload="TEST 1.0"),
                 dict(t=2, kind="brb_send", node=0, kp=0, s=0, payload="TEST 1.0")]
        extra += restricted_send(0, 11, 0, 0b0101010101010) + [dict(t=0, kind="byz_key", kp=12, s=0, value=0)]
        extra += byz_msgs(2, byz, [(11, 0), (12, 0), (0, 0), (3, 0), (5, 0)], n)
        if i == 2:
            extra += [dict(t=120, kind="brb_send", node=8, kp=8, s=0, payload="TEST 9.0")] + byz_msgs(121, byz, [(8, 0)], n)
        return S.brb_spec(n, 4, 0x17E40010, SLOW, 8, g, sends, byzantine=byz, extra=extra)
    add("p16-ref-byz", "packed16", ("step", 16, 8, REF, 0), p16, 7, 8, False,
        late={i: _send(7) for i in (1, 5)}, bounds={2: [120]}, packed=True, byz=[11, 12])

    # NPAD 32 (2 per wave): consensus over best-effort broadcast, staggered proposals, direct deliver() calls
    def p32(g, i):
        starts = [(d * (g + 1)) % 4 for d in range(31)]
        return S.beb_cons_spec(31, 10, 0x17E40020, UNIF, 5, g, round_cap=3, starts=starts, extra=_early(S.deliver_actions(31, 0x17E5 + g, count=10)))
    add("p32-beb-cons", "packed32", ("step", 32, 8, BEB, 0), p32, 5, 8, True,
        late={i: [dict(kind="deliver", node=30 - i, kp=i, value=2), dict(kind="deliver", node=i, kp=30, value=1)] for i in (1, 4)},
        packed=True)

    # ---- NPAD 64, lean, register masks (constant / slow-set delays up to 8) ---------------------------------
    def r_ref(g, i):
        return S.cons_spec(64, 21, 0x5EED0004, SLOW, 8, g, round_cap=1, starts=[(d + g) % 3 for d in range(64)],
                           extra=S.deliver_actions(64, 0x17E6 + g, count=8))
    # (key window 8: at 4 the engine stops these with BRC_OVERFLOW, its own limit, one-shot and interleaved alike)
    add("n64r-ref-cons", "lean64r-ref", ("step", 64, 8, REF, 2), r_ref, 3, 8, True,
        late={1: [dict(kind="deliver", node=63, kp=5, value=2), dict(kind="deliver", node=0, kp=63, value=1)]})

    # SPEC refuses direct deliver() calls: broadcast streams that wrap Q = 4, constant delay 3
    def r_spec(g, i):
        return S.spec_brb_spec(45, 14, 0x17E40041, SLOW, 5, g, stream(g % 9, 7, 6) + stream(44, 6, 6, t0=2), window=4)
    add("n64r-spec-brb", "lean64r-spec", ("step", 64, 8, SPEC, 2), r_spec, 3, 4, False, late={i: _send(30) for i in (0, 2)})

    def r_beb(g, i):
        return S.beb_cons_spec(50, 16, 0x17E40042, SLOW, 5, g, round_cap=3, starts=[(d + 2 * g) % 3 for d in range(50)],
                               extra=_early(S.deliver_actions(50, 0x17E7 + g, count=8)))
    add("n64r-beb-cons", "lean64r-beb", ("step", 64, 8, BEB, 2), r_beb, 3, 8, True,
        late={1: [dict(kind="deliver", node=49, kp=3, value=2), dict(kind="deliver", node=0, kp=49, value=1)]})

    # ---- NPAD 64, lean, per-link delays (no register masks) ------------------------------------------------
    # reference broadcast: a stream that wraps Q = 8, a restricted SEND, Byzantine ECHO / READY; instance 2 resumes
    def l_ref(g, i):
        n, byz = 50, [48, 49]
        even = sum(1 << d for d in range(0, n, 2))
        sends = stream(g % 5, 11, 6) if i != 2 else stream(g % 5, 4, 6) + stream(g % 5, 7, 6, t0=150, s0=4)
        extra = restricted_send(1, 48, 0, even) + byz_msgs(3, byz, [(48, 0), (g % 5, 0)], n)
        return S.brb_spec(n, 16, 0x17E40043, GEO, 5, g, sends, byzantine=byz, extra=extra)
    add("n64-ref-brb", "lean64-ref", ("step", 64, 8, REF, 0), l_ref, 4, 8, False,
        late={i: _send(20) for i in (1, 3)}, bounds={2: [150]}, byz=[48, 49])

    def l_spec(g, i):
        return S.spec_brb_spec(64, 21, 0x17E40044, UNIF, 4, g, stream(g % 9, 7, 5) + stream(63, 6, 5, t0=2), window=4)
    add("n64-spec-brb", "lean64-spec", ("step", 64, 4, SPEC, 0), l_spec, 3, 4, False, late={i: _send(33) for i in (0, 2)})

    def l_beb(g, i):
        return S.beb_spec(37, 0x17E40045, UNIF, 6, g, stream(g % 11, 10, 3) + stream(36, 3, 7, t0=1))
    add("n64-beb-brb", "lean64-beb", ("step", 64, 8, BEB, 0), l_beb, 3, 8, False, late={1: _send(20)})

    # ---- NPAD 64, general keys (8-B tagged cells, extra SENDs) and connection peers ---------------------------
    def xref(g, i):
        extra = [dict(t=0, kind="brb_send", node=9, kp=0, s=0, payload="TEST 1.0"),
                 dict(t=1, kind="brb_send", node=0, kp=0, s=0, payload="TEST 1.0"),
                 dict(t=2 + g % 2, kind="brb_send", node=21, kp=2, s=0, payload="TEST 3.0")]
        sends = [(0, 0, 0), (0, 1, 0), (0, 2, 0)] + (stream(5, 3, 9, t0=100) if i == 2 else stream(5, 3, 9, t0=4))
        return dict(S.brb_spec(40, 13, 0x17E40046, SLOW, 4, g, sends, extra=extra), general_keys=True)
    add("n64-xref-brb", "general64", ("step", 64, 4, XREF, 0), xref, 3, 8, False,
        late={1: [dict(kind="brb_send", node=30, kp=1, s=0, payload="TEST 2.0")]}, bounds={2: [100]})

    def conn(g, i):
        n, byz = 40, [37, 38, 39]
        sends = [(0, 0, 0), (g % 3, 7, 0), (2, 20, 0)]
        extra = byz_msgs(2, byz, [(0, 0), (7, 0)], n) + byz_msgs(4, byz[:2], [(0, 0), (20, 0)], n)
        return S.brb_spec(n, 13, 0x17E40047, SLOW, 6, g, sends, byzantine=byz, extra=extra, peer_mode="connection")
    add("n64-conn-brb", "conn64", ("step", 64, 8, CONN, 0), conn, 3, 8, False,
        late={1: _send(11) + [dict(kind="byz", src=37, type=S.READY, kp=0, s=0, dst=(1 << 40) - 1)]}, byz=[37, 38, 39])

    # ---- wide kernels: a SEND restricted in the high destination words --------------------------------------
    def w128(g, i):
        n, byz = 70, [68, 69]
        dst = sum(1 << d for d in (1, 5, 33, 64, 66, 67))
        sends = [(0, 0, 0), (1 + g % 2, 57, 0)] + ([(80, 65, 0)] if i == 0 else [(3, 65, 0)])
        extra = restricted_send(1, 68, 0, dst) + byz_msgs(2, byz, [(68, 0), (0, 0)], n)
        return S.brb_spec(n, 23, 0x17E40080, SLOW, 8, g, sends, byzantine=byz, extra=extra)
    add("w128-ref-brb", "wide128", ("wide", 128, 8, REF, 4), w128, 2, 4, False, late={1: _send(40)}, bounds={0: [80]}, byz=[68, 69])

    def w256(g, i):
        n, byz = 140, [139]
        dst = sum(1 << d for d in range(3, n, 5))
        sends = [(0, 7, 0), (2, 130 - g % 2, 0)]
        extra = restricted_send(0, 139, 0, dst) + byz_msgs(3, byz, [(139, 0)], n)
        return S.spec_brb_spec(n, 46, 0x17E40100, GEO, 6, g, sends, byzantine=byz, extra=extra, window=4)
    add("w256-spec-brb", "wide256", ("wide", 256, 8, SPEC, 0), w256, 2, 4, False, late={0: _send(70)}, byz=[139])
    assert len({c.name for c in out}) == len(out)
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


def by_name():
    return {c.name: c for c in cases()}


# ---- extra SENDs beyond the table: pruned while the run goes on -----------------------------------------------
def pruning_spec():
    """n = 7 (a 3-bit-id kernel), one instance: origin 0 SENDs 24 keys, 12 steps apart, and nodes 1 and 2 SEND
    every key again one and two steps later -- 48 extra-SEND records (different steps: none merges), two within
    delay_max = 4 steps of each other.  brc_inject drops a record once q.t + delay_max < the item's step, so fed a
    few steps ahead the table never holds more than XSEND_MAX; injected at once it would, and is refused."""
    sends = stream(0, 24, 12)
    extra = [dict(t=t + o, kind="brb_send", node=o, kp=0, s=s, payload="TEST 1.%d" % s) for (t, _o, s) in sends for o in (1, 2)]
    return dict(S.brb_spec(7, 2, 0x17E400F0, SLOW, 4, OFFSET, sends, extra=extra), name="pruning/0", step_cap=STEP_CAP)


# ---- the oracle, once per spec -------------------------------------------------------------------------------
_ORACLE = {}
VID = T.VID


def oracle_run(sp):
    from oracle import oracle
    from tests import golden_io
    exp = oracle.run(sp)
    dec = {}
    for t, node, rnd, val in sorted(exp["events"]["decide"]):
        dec.setdefault(node, []).append((rnd, t, VID[val]))
    exp["events"] = golden_io.canonical_events(exp["events"])
    return exp, dec, exp["counts"]["deliver"]


def oracle_results(case):
    """{local id: (result with canonically sorted event lists, per replica [(round, t, value id) of every decide
    event], deliver count)} of every instance."""
    import concurrent.futures
    if case.name not in _ORACLE:
        specs = case.specs
        with concurrent.futures.ThreadPoolExecutor(min(8, len(specs))) as ex:
            _ORACLE[case.name] = dict(enumerate(ex.map(oracle_run, specs)))
    return _ORACLE[case.name]


def expected_read_side(case):
    """(round_histogram(66), decisions() counts by value id, undecided, disagreements) from the oracle's decide events."""
    hist, counts, undecided, dis = [0] * 66, {}, 0, 0
    hon = [d for d in range(case.specs[0]["n"]) if d not in case.byz]
    for _i, (_exp, dec, _d) in oracle_results(case).items():
        firsts = [dec[d][0] for d in hon if d in dec]
        undecided += len(hon) - len(firsts)
        for (_r, _t, v) in firsts:
            counts[v] = counts.get(v, 0) + 1
        dis += len({v for (_r, _t, v) in firsts}) > 1
        hist[min(max(r for (r, _t, _v) in firsts), 65) if len(firsts) == len(hon) else 0] += 1
    return hist, counts, undecided, dis
