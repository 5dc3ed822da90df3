"""Workload table of tests/test_gpu_time_axis.py (GPU) and tests/test_time_axis_workloads.py (its preconditions, on
the oracle alone): the time axis.  (1) Runs stopped by the step cap (BRC_STEPCAP: every kernel's own
``next > P.step_cap`` exit against brc_oracle.c's ``nt > sp->step_cap``), (2) runs at late steps, up to STEP_LIMIT.

A case: name, family, specs (harness format, tests/golden/specs.py; at most 8 instances, 3 on the wide kernels,
consecutive global ids from 777, one configuration), key_window, consensus, byz, and how its engine is created
(flags: BRC_FLAG_WIDE_RECORDS / BRC_FLAG_WIDE_VALUES; life: the key-lifetime kernel against the step kernel).

Caps.  caps(case) derives them from the oracle's uncapped run of the case, never by hand.  ref is the instance that
runs longest and t_last its last active step.  The expected result for cap c is the oracle's run of capped(sp, c):
step_cap = c and the actions with t <= c (brc_inject refuses t > step_cap).
  zero, one     caps 0 and 1
  mid           the step nearest t_last // 2 at which ref has arrivals (no action of its own) and stops with stepcap
  gap           the step nearest t_last // 2 with no activity in ref (its capped run ends with t_stop < cap) while
                messages are in flight (status stepcap), activity before and after it.  Two-class delays (constant,
                slow-set) leave such steps by themselves; the per-link cases get them from a late SEND of a Byzantine
                origin to ONE receiver over a link of three steps or more (slow_link).  The per-link form of the
                key-lifetime kernel takes no injection and has arrivals at every step: it has no gap cap
                (test_time_axis_workloads proves that it has none)
  last-1        t_last - 1: ref stops with stepcap, one step short
  last          t_last: every instance ends as it does without a cap
Every instance of a batch runs under the same cap; the ones that end before it are quiescent or done.

Late runs (the oracle is time-translation invariant: delays and coins do not depend on t).
  shift(sp, T0)        every action T0 later, step cap STEP_LIMIT
  two_bursts(sp, T0)   the original actions, and at T0 a second burst: the origin of a first-burst key SENDs sequence
                       number s + key_window (the same key slot, reused ~T0 steps later), and a Byzantine replica
                       ECHOes another first-burst key, still held in its slot, to everyone.  BRB cases only: a
                       consensus instance is DONE after its first burst and performs no later action
  cut                  shift by T0 = STEP_LIMIT - mid (the mid cap: the step nearest t_last // 2 at which ref stops with
                       stepcap), actions past STEP_LIMIT dropped: the run is stopped by STEP_LIMIT itself
The key-lifetime kernel takes none of them (no injection: its proposals are the Philox draws of step 0).

Time fields of the kernels and their widths (what the T0 values are chosen against):
  InstState.status / t_stop / q_until        16 bits each (brc_internal.h; packed as one u64 by every kernel's exit)
  key metadata t_send, t_quiet               16 bits each, NEVER = 0xFFFF (brc_step.h m_pack)
  general cells' ECHO / READY send steps     16 bits each (brc_step.h, word >> 32, word >> 48)
  cons1 first_decide_t                       16 bits
  wide record table, extra-SEND table time   16 bits (recs >> 16 & 0xFFFF), 24 bits (t << 16 below seg << 40)
  lean cells' ECHO / READY send offsets      7 bits from ItemState.epoch, moved by rebase() once t - ep > 100
  key-lifetime kernel relative send steps    16 bits (LIFE_NEVER = 0xFFFF)
  activity ring rows                         t & (RS - 1), RS = 16 or 32
  ItemState.t, InjDev.t, brc_event.t         32 bits
All 16-bit fields hold STEP_LIMIT + 16 = 60016; the powers of two under 60000 that bound something are 2^15 (a
16-bit time read as signed) and 2^7 (the lean offsets).  T0 = 59,900 for every family; the lean and the wide-records
cases also cross 32,768 and 128 (T0 = 2^k - t_last // 2, LATE_EXTRA).  A burst at step 0 and one at 59,900 make
rebase() jump ~60,000 steps at once.
"""
from tests import step_noevent_workloads as T
from tests.golden import specs as S

OFFSET = T.OFFSET
CONST, UNIF, SLOW, GEO = T.CONST, T.UNIF, T.SLOW, T.GEO
CKEYS = ("status", "t_stop", "msgs_sent", "arrivals", "cell_steps")
STEP_LIMIT = 60000                                  # csrc/brc_internal.h
T0 = 59900
RUN_CAP = 400                                       # the uncapped runs' step cap: far above every t_last
VID = T.VID


def slow_link(sp, src, lo=3):
    """The first honest receiver whose link from src takes lo steps or more in instance sp["g"]."""
    from oracle.schedule import Schedule
    sch = Schedule(sp["n"], sp["f"], sp["seed"], sp["delay_model"], sp["dmax"], sp.get("dconst", 1))
    return next(d for d in range(sp["n"]) if d not in sp["byzantine"] and sch.delay(sp["g"], src, d) >= lo)


def lone_send(sp, t, b, s=0):
    """sp with a late SEND of Byzantine origin b's key (b, s) to one receiver over a slow link: one message in flight."""
    d = slow_link(sp, b)
    return dict(sp, actions=sp["actions"] + [dict(t=t, kind="byz_key", kp=b, s=s, value=0),
                                             dict(t=t, kind="byz", src=b, type=S.SEND, kp=b, s=s, dst=1 << d)])


class Case:
    def __init__(self, name, family, make, count, key_window, consensus, byz=(), wide_records=False, wide_values=False,
                 life=False, msg=True, gap=True):
        self.name, self.family, self._make, self.count, self.key_window = name, family, make, count, key_window
        self.consensus, self.byz, self.wide_records, self.wide_values = consensus, list(byz), wide_records, wide_values
        self.life, self.msg, self.gap = life, msg, gap
        self._specs = None

    @property
    def specs(self):
        if self._specs is None:
            self._specs = [dict(self._make(OFFSET + i, i), name="%s/%d" % (self.name, i), step_cap=RUN_CAP) for i in range(self.count)]
        return self._specs

    @property
    def flagged(self):
        return self.wide_records or self.wide_values

    @property
    def brb(self):
        return not self.consensus


def capped(sp, c):
    return dict(sp, step_cap=c, actions=[a for a in sp.get("actions", []) if a["t"] <= c])


def shift(sp, t0):
    return dict(sp, step_cap=STEP_LIMIT, actions=[dict(a, t=a["t"] + t0) for a in sp["actions"]])


def first_keys(sp):
    """(origin, s) of the honest BRB SENDs of sp's action list, in list order."""
    out = []
    for a in sp["actions"]:
        if a["kind"] == "brb_send" and a["node"] == a["kp"] and (a["kp"], a["s"]) not in out:
            out.append((a["kp"], a["s"]))
    return out


def two_bursts(case, i, t0):
    """(spec, the reused-slot key) of instance i.  The second burst: the origin of the first first-burst key that every
    honest replica delivered (the same links, the same delays: the second delivers as well) SENDs s + key_window; where
    the family takes BRC_INJ_MSG and has a Byzantine replica, that replica ECHOes another first-burst key to everyone."""
    assert case.brb
    sp = case.specs[i]
    exp = oracle_results((case.name, "base"), case.specs)[i][0]
    hon = [d for d in range(sp["n"]) if d not in case.byz]
    keys = first_keys(sp)
    full = [k for k in keys if sorted(e[1] for e in exp["events"]["deliver"] if tuple(e[2:]) == k) == hon]
    (o, s) = full[0]
    held = next(k for k in keys if k != (o, s))
    q = sp["window"] if sp["mode"] == "spec_brb" else case.key_window
    acts = [dict(t=t0, kind="brb_send", node=o, kp=o, s=s + q, payload="TEST %d.%d" % (o + 1, s + q))]
    if case.msg and case.byz:
        acts.append(dict(t=t0, kind="byz", src=case.byz[0], type=S.ECHO, kp=held[0], s=held[1], dst=(1 << sp["n"]) - 1))
    return dict(sp, step_cap=STEP_LIMIT, actions=sp["actions"] + acts), (o, s + q)


# ---- the oracle, once per spec list -------------------------------------------------------------------------------
_ORACLE = {}


def oracle_run(sp):
    from oracle import oracle
    from tests import golden_io
    exp = oracle.run(sp)
    dec = {}
    for t, node, rnd, val in sorted(exp["events"]["decide"]):
        dec.setdefault(node, []).append((rnd, t, VID[val]))
    exp["events"] = golden_io.canonical_events(exp["events"])
    return exp, dec, exp["counts"]["deliver"]


def oracle_results(tag, specs):
    """[(result with canonically sorted event lists, per replica [(round, t, value id) of every decide event],
    deliver count)] per instance; tag names the spec list (cached)."""
    import concurrent.futures
    if tag not in _ORACLE:
        with concurrent.futures.ThreadPoolExecutor(min(8, len(specs))) as ex:
            _ORACLE[tag] = list(ex.map(oracle_run, specs))
    return _ORACLE[tag]


def expected_read_side(case, results):
    """(round_histogram(66), decision counts by value id, undecided, disagreements, stepcap count) from the oracle's
    results: an instance in which some honest replica has not decided counts in hist[0]."""
    hist, counts, undecided, dis = [0] * 66, {}, 0, 0
    hon = [d for d in range(case.specs[0]["n"]) if d not in case.byz]
    for (_exp, dec, _d) in results:
        firsts = [dec[d][0] for d in hon if d in dec]
        undecided += len(hon) - len(firsts)
        for (_r, _t, v) in firsts:
            counts[v] = counts.get(v, 0) + 1
        dis += len({v for (_r, _t, v) in firsts}) > 1
        hist[min(max(r for (r, _t, _v) in firsts), 65) if len(firsts) == len(hon) else 0] += 1
    return hist, counts, undecided, dis, sum(exp["status"] == "stepcap" for (exp, _dec, _d) in results)


def _light(sp):
    from oracle import oracle
    return oracle.run(sp, light=True)


_CAPS = {}


def caps(case):
    """{label: cap} (module docstring), and the reference instance: (caps, ref, t_last)."""
    if case.name in _CAPS:
        return _CAPS[case.name]
    runs = [_light(sp) for sp in case.specs]
    assert all(r["status"] in ("quiescent", "done") for r in runs), (case.name, runs)
    ref = max(range(case.count), key=lambda i: runs[i]["t_stop"])
    sp, t_last = case.specs[ref], runs[ref]["t_stop"]
    assert t_last >= 6, (case.name, t_last)
    own = {a["t"] for a in sp["actions"]}
    near = sorted(range(2, t_last - 1), key=lambda c: (abs(c - t_last // 2), c))
    out = {"zero": 0, "one": 1}
    for c in near:
        r = _light(capped(sp, c))
        if r["status"] != "stepcap":
            continue
        if "mid" not in out and r["t_stop"] == c and c not in own and r["arrivals"] > _light(capped(sp, c - 1))["arrivals"]:
            out["mid"] = c
        if "gap" not in out and case.gap and r["t_stop"] < c:
            out["gap"] = c
        if "mid" in out and ("gap" in out or not case.gap):
            break
    out["last-1"] = t_last - 1
    out["last"] = t_last
    _CAPS[case.name] = (out, ref, t_last)
    return _CAPS[case.name]


def capped_specs(case, c):
    return [capped(sp, c) for sp in case.specs]


def late_t0s_labels(case):
    return ("59900", "x32768", "x128") if case.name in LATE_EXTRA else ("59900",)


AT_NOW_STEP = {"n64-ref-brb": 3, "w128-rec-brb": 2}


def at_now_marks(case, t0):
    """{instance: {t0 + r}} for engine_runner.at_now on the case's shifted run: r = AT_NOW_STEP, a step whose actions
    (Byzantine ECHO / READY; on the wide-records case an ECHO to a subset, a record) stay on the host until the
    instance stands there.  Only instances that have arrivals at step r without those actions: run(1) stops there."""
    rel, marks = AT_NOW_STEP[case.name], {}
    for i, sp in enumerate(case.specs):
        without = dict(sp, actions=[a for a in sp["actions"] if a["t"] != rel])
        r, before = _light(capped(without, rel)), _light(capped(without, rel - 1))
        if len(without["actions"]) < len(sp["actions"]) and r["t_stop"] == rel and r["arrivals"] > before["arrivals"]:
            marks[i] = {t0 + rel}
    return marks


def late_t0s(case):
    """{label: T0}: 59,900 for every family; the lean and the wide-records cases also cross 2^15 and 2^7."""
    out = {"59900": T0}
    if case.name in LATE_EXTRA:
        t_last = caps(case)[2]
        out.update({"x32768": 32768 - t_last // 2, "x128": 128 - min(t_last // 2, 100)})
    return out


def cut_t0(case):
    """STEP_LIMIT falls on the case's mid cap (the step nearest t_last // 2 at which ref stops with stepcap)."""
    return STEP_LIMIT - caps(case)[0]["mid"]


def late_specs(case):
    """{label: (specs, reused-slot keys per instance or None)} of the case's late runs."""
    out = {}
    for lab, t0 in late_t0s(case).items():
        out["shift-" + lab] = ([shift(sp, t0) for sp in case.specs], None)
        if case.brb:
            both = [two_bursts(case, i, t0) for i in range(case.count)]
            out["bursts-" + lab] = ([b[0] for b in both], [b[1] for b in both])
    out["cut"] = ([capped(shift(sp, cut_t0(case)), STEP_LIMIT) for sp in case.specs], None)
    return out


# ---- the cases -----------------------------------------------------------------------------------------------------
def _stream(origin, count, gap, t0=0, s0=0):
    return [(t0 + j * gap, origin, s0 + j) for j in range(count)]


def _byz_msgs(t, srcs, keys, n, types=(S.ECHO, S.READY)):
    allm = (1 << n) - 1
    return [dict(t=t, kind="byz", src=b, type=typ, kp=kp, s=s, dst=allm) for b in srcs for typ in types for (kp, s) in keys]


def _build():
    out = []

    def add(*a, **kw):
        out.append(Case(*a, **kw))

    # ---- packed narrow kernels (two link classes, or one constant delay, leave gap steps)
    def p4(g, i):
        # (one slow replica of four keeps every step busy: constant delay 3, proposals staggered by multiples of it)
        return S.cons_spec(4, 1, 0x71AE0004, CONST, 3, g, round_cap=3, dconst=3, starts=[0, 3 * (g % 3), 3 * (g % 2), 6 * (i % 3)])
    add("p4-ref-cons", "packed4", p4, 8, 8, True)

    def p8(g, i):
        sends = _stream(g % 5, 2, 9) + [(1 + g % 2, 5, 0)]
        return S.spec_brb_spec(7, 2, 0x71AE0008, SLOW, 4, g, sends, window=4, byzantine=[6])
    add("p8-spec-brb", "packed8", p8, 8, 4, False, byz=[6])

    def p16(g, i):
        n, byz = 13, [11, 12]
        sends = [(0, 0, 0), (1, 3, 0), (g % 3, 5, 0)]
        extra = [dict(t=0, kind="byz_key", kp=11, s=0, value=0), dict(t=0, kind="byz", src=11, type=S.SEND, kp=11, s=0, dst=0b0101010101010),
                 dict(t=0, kind="byz_key", kp=12, s=0, value=0)]
        extra += _byz_msgs(2, byz, [(11, 0), (12, 0), (0, 0)], n)
        # ECHO / READY to a subset of the peers: records of the item's table
        extra += [dict(t=3, kind="byz", src=12, type=S.ECHO, kp=3, s=0, dst=0b0000111100001 | 1 << (g % 11)),
                  dict(t=4, kind="byz", src=11, type=S.READY, kp=5, s=0, dst=0b0011001100110)]
        return S.brb_spec(n, 4, 0x71AE0010, SLOW, 8, g, sends, byzantine=byz, extra=extra)
    add("p16-ref-byz", "packed16", p16, 7, 8, False, byz=[11, 12])

    def p32(g, i):
        return S.beb_cons_spec(31, 10, 0x71AE0020, SLOW, 5, g, round_cap=3, starts=[(d * (g + 1)) % 4 for d in range(31)])
    add("p32-beb-cons", "packed32", p32, 5, 8, True)

    # ---- lean kernels, register masks (two delay classes): consensus
    def r_ref(g, i):
        return S.cons_spec(40, 13, 0x71AE0040, SLOW, 8, g, round_cap=1, starts=[(d + g) % 3 for d in range(40)])
    add("n40r-ref-cons", "lean64r-ref", r_ref, 3, 8, True)

    def r_spec(g, i):
        return S.spec_cons_spec(40, 13, 0x71AE0041, CONST, 3, g, round_cap=2, window=4, coin_seed=T.COIN, dconst=3)
    add("n40r-spec-cons", "lean64r-spec", r_spec, 3, 4, True)

    # ---- lean kernels, per-link delays: broadcast, a lone late SEND over a slow link (gap steps)
    def l_ref(g, i):
        byz = [62, 63]
        sp = S.brb_spec(64, 9, 0x71AE0042, GEO, 5, g, [(0, g % 5, 0), (1, 40, 0), (2, 61, 0)], byzantine=byz,
                        extra=_byz_msgs(3, byz, [(g % 5, 0)], 64))
        return lone_send(sp, 40 + 3 * i, 63)
    add("n64-ref-brb", "lean64-ref", l_ref, 3, 8, False, byz=[62, 63])

    def l_spec(g, i):
        sp = S.spec_brb_spec(64, 21, 0x71AE0043, UNIF, 4, g, [(0, g % 9, 0), (2, 50, 0)], window=4, byzantine=[63])
        return lone_send(sp, 40 + 3 * i, 63)
    add("n64-spec-brb", "lean64-spec", l_spec, 3, 4, False, byz=[63])

    # ---- general keys (8-B tagged cells, extra SENDs), connection peers
    def xref(g, i):
        extra = [dict(t=0, kind="brb_send", node=9, kp=0, s=0, payload="TEST 1.0"),
                 dict(t=1, kind="brb_send", node=0, kp=0, s=0, payload="TEST 1.0"),
                 dict(t=2 + g % 2, kind="brb_send", node=21, kp=2, s=0, payload="TEST 3.0")]
        return dict(S.brb_spec(40, 13, 0x71AE0044, SLOW, 4, g, [(0, 0, 0), (0, 1, 0), (0, 2, 0), (4 + i, 5, 0)], extra=extra,
                               byzantine=[39]), general_keys=True)
    add("n40-xref-brb", "general64", xref, 3, 8, False, byz=[39])

    def c6(g, i):
        return S.cons_spec(6, 1, 0x71AE0006, CONST, 2, g, round_cap=2, dconst=2, starts=[0, 0, 2 * (g % 2), 2, 0, 4 * (i % 2)],
                           peer_mode="connection")
    add("n6-conn-cons", "conn8", c6, 8, 8, True)

    def c40(g, i):
        n, byz = 40, [37, 38, 39]
        extra = _byz_msgs(2, byz, [(0, 0), (7, 0)], n) + _byz_msgs(4, byz[:2], [(0, 0), (20, 0)], n)
        return S.brb_spec(n, 13, 0x71AE0047, SLOW, 6, g, [(0, 0, 0), (g % 3, 7, 0), (2, 20, 0)], byzantine=byz, extra=extra,
                          peer_mode="connection")
    add("n40-conn-brb", "conn64", c40, 3, 8, False, byz=[37, 38, 39])

    # ---- wide kernels
    def w_ref(g, i):
        return S.cons_spec(70, 3, 0x71AE0070, CONST, 3, g, round_cap=1, dconst=3, starts=[(d + i) % 2 for d in range(70)])
    add("w128-ref-cons", "wide128", w_ref, 3, 8, True)

    def w_spec(g, i):
        return S.spec_cons_spec(70, 23, 0x71AE0071, CONST, 2, g, round_cap=1, window=4, coin_seed=T.COIN, dconst=2)
    add("w128-spec-cons", "wide128", w_spec, 3, 4, True)

    def w256(g, i):
        byz = [129]
        return S.brb_spec(130, 43, 0x71AE0130, SLOW, 8, g, [(0, 7, 0), (2, 128 - g % 2, 0), (3 + i, 64, 0)], byzantine=byz,
                          extra=_byz_msgs(3, byz, [(7, 0)], 130))
    add("w256-ref-brb", "wide256", w256, 3, 4, False, byz=[129])

    # BRC_FLAG_WIDE_RECORDS: an ECHO to a subset of the peers (both destination words) and a second SEND of a key
    def wrec(g, i):
        n, byz = 70, [5, 66, 69]
        dst = sum(1 << d for d in (1, 9, 33, 64, 65, 67)) | 1 << (10 + g % 20)
        extra = [dict(t=2, kind="byz", src=69, type=S.ECHO, kp=0, s=0, dst=dst),
                 dict(t=1, kind="brb_send", node=65, kp=0, s=0, payload="TEST 1.0"),
                 dict(t=9 + i, kind="brb_send", node=67, kp=30, s=0, payload="TEST 31.0")]
        return S.brb_spec(n, 23, 0x71AE0072, SLOW, 8, g, [(0, 0, 0), (1, 30, 0)], byzantine=byz, extra=extra)
    add("w128-rec-brb", "wide128-records", wrec, 3, 4, False, byz=[5, 66, 69], wide_records=True)

    # BRC_FLAG_WIDE_VALUES: a majority of one three-bit value id (wide_values_workloads.majority)
    def wval(g, i):
        from tests import wide_values_workloads as V
        m = 4 + (g + i) % 4
        return dict(S.cons_spec(70, 5, 0x71AE0073, SLOW, 8, g, round_cap=1, byzantine=[5, 66, 69],
                                proposals=V.majority(70, g, m, 56, [v for v in range(8) if v != m])), values=S.VALUES8)
    add("w128-val-cons", "wide128-values", wval, 3, 8, True, byz=[5, 66, 69], wide_values=True)

    # ---- the key-lifetime kernel (Philox proposals, nothing injected), each form against the step kernel
    def life2(g, i):
        return S.cons_spec(40, 13, 0x71AE0048, SLOW, 8, g, round_cap=2)
    add("life-2class", "life", life2, 8, 8, True, life=True)

    def lifepl(g, i):
        return S.cons_spec(40, 13, 0x71AE0049, UNIF, 3, g, round_cap=2)
    add("life-perlink", "life", lifepl, 8, 8, True, life=True, gap=False)
    assert len({c.name for c in out}) == len(out)
    return out


LATE_EXTRA = ("n64-ref-brb", "n40r-ref-cons", "w128-rec-brb")
SLICED = ("p16-ref-byz", "n64-ref-brb", "w128-ref-cons", "w128-rec-brb")         # packed, lean, wide, wide-records
LATE_INTERLEAVED = ("n64-ref-brb", "w128-rec-brb")
_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


def by_name():
    return {c.name: c for c in cases()}


def step_cases():
    return [c for c in cases() if not c.life]


# ---- mixed items on the packed kernels: instances of one wave item that end differently under one cap --------------
class Mixed:
    """name, specs (all in ONE wave item: count <= 64 / NPAD), cap, want {instance: status}."""
    def __init__(self, name, specs, cap, want, key_window=8, byz=()):
        self.name, self.cap, self.want, self.key_window, self.byz = name, cap, want, key_window, list(byz)
        self.specs = [dict(sp, name="%s/%d" % (name, i), step_cap=cap) for i, sp in enumerate(specs)]
        self.consensus, self.flagged = False, False
        self.count = len(specs)


def mixed():
    """p8-ends: n = 7 (NPAD 8: the five share one wave item), slow-set delays up to 4, cap 12.
         0  one SEND at step 0: quiesces early
         1  no action at all: quiescent, t_stop 0
         2  a SEND at step 10: stops at the cap with messages in flight
         3  its last action, a SEND, at t == cap exactly: performed and counted, its messages never arrive
         4  a SEND at step 0 and another origin's at the cap
       p16-bound: bound_case()."""
    def b7(g, sends):
        return S.brb_spec(7, 2, 0x71AE00A0, SLOW, 4, g, sends)
    cap = 12
    ends = Mixed("p8-ends", [b7(OFFSET, [(0, 0, 0)]), b7(OFFSET + 1, []), b7(OFFSET + 2, [(10, 1, 0)]),
                             b7(OFFSET + 3, [(0, 2, 0), (cap, 3, 0)]), b7(OFFSET + 4, [(0, 4, 0), (cap, 0, 0)])],
                 cap, {0: "quiescent", 1: "quiescent", 2: "stepcap", 3: "stepcap", 4: "stepcap"})
    return [ends, bound_case()]


def bound_case():
    """The q_until question (brc_step.h: a segment goes QUIESCENT only at a step's end, by q_until <= t, and the
    STEPCAP exit stamps every segment still RUNNING; q_until is a bound, t + the largest link delay, not the
    segment's last real arrival).  A broadcast's bound is tight: maxout covers honest receivers only, and the
    slowest of them does get the message.  A SEND to a subset is where bound and arrival could part.
    n = 13, slow-set delays up to 8 (links of 1 and of 8 steps), Byzantine replica b (not in instance A's slow set).
      A  b declares its key and ECHOes it to everyone at step 0 (arrivals at 1 and 8); at step 10 it SENDs the key to
         ONE receiver over a link of 1 step.  The SEND lands at 11 and is ignored (the receiver has the ECHO:
         core/brbroadcast.py:74-82; SPEC-free reference protocol).  A's last arrival is step 11; a bound taken over all
         of b's links would be 18.
      B  a sibling in the same wave item: b's lone SEND at step 12 to one receiver over a link of 8 steps, which lands
         at 20, past the cap 15.
    The oracle: A quiescent (t_stop 11), B stepcap (t_stop 12)."""
    from oracle.schedule import Schedule
    seed, g = 0x71AE00B0, OFFSET
    sch = Schedule(13, 4, seed, SLOW, 8, 1)
    b = next(x for x in range(12, -1, -1) if not sch.is_slow(g, x))
    fast = next(d for d in range(13) if d != b and sch.delay(g, b, d) == 1)
    slow = next(d for d in range(13) if d != b and sch.delay(g + 1, b, d) == 8)
    base = S.brb_spec(13, 4, seed, SLOW, 8, g, [], byzantine=[b])
    key = dict(kind="byz_key", kp=b, s=0, value=0)
    a = dict(base, actions=[dict(key, t=0), dict(t=0, kind="byz", src=b, type=S.ECHO, kp=b, s=0, dst=(1 << 13) - 1),
                            dict(t=10, kind="byz", src=b, type=S.SEND, kp=b, s=0, dst=1 << fast)])
    bb = dict(base, g=g + 1, actions=[dict(key, t=12), dict(t=12, kind="byz", src=b, type=S.SEND, kp=b, s=0, dst=1 << slow)])
    m = Mixed("p16-bound", [a, bb], 15, {0: "quiescent", 1: "stepcap"}, byz=[b])
    m.t_stop = {0: 11, 1: 12}
    return m
