"""Workload table of tests/test_gpu_wide_windows.py (GPU) and tests/test_wide_window_workloads.py (its preconditions, on
the oracle alone): key windows of 16 and 32 phase indices per origin on the wide step kernels (n > 64) of an engine
created with BRC_FLAG_WIDE_WINDOWS.

A case is an interleaved_workloads.Case: COUNT = 8 instances, consecutive global ids from 777, one configuration, one
workgroup per instance, with

  q, nv     the tested key window and the key variants per origin (q * nv is 16 or 32: brc_create refuses it
            without the flag)
  half      q / 2 where a flagged engine at that window must stop an instance with BRC_OVERFLOW, else None (the
            shape's half-window leg is dropped, and the line below says why)
  rec, v8   the engine is created with BRC_FLAG_WIDE_RECORDS / BRC_FLAG_WIDE_VALUES as well

n = 70 pads to 128 (two waves, the last word partial), n = 130 to 256 (the third word partial).  Two silent Byzantine
replicas sit in different 64-replica words.  Slow-set delays with D = 8 unless said otherwise; the round caps are the
lowest at which the oracle's send log needs more than half the window (needs(), the CPU test).

  ww-128-ref-q16     n = 70   REF  round cap 5   window 16
  ww-128-ref-q32     n = 70   REF  round cap 9   window 32
  ww-128-beb-q16     n = 70   BEB  round cap 5   window 16
  ww-128-beb-q32     n = 70   BEB  round cap 10  window 32
  ww-256-ref-q16     n = 130  REF  round cap 4   window 16   (the lowest cap that needs more than 8; two instances of
                                                             the batch do.  SLOW_ORACLE: a run takes 9.4 to 10.8 s)
  ww-256-ref-q32     n = 130  REF  round cap 4   window 32   the same specs (one set of oracle runs serves both) on
                                                             8,192 key slots: the 146 KB carve with the host-mask
                                                             planes.  half = None: a window above 16 needs round cap 8
                                                             there, 19 s per oracle run, so no half window can be made
                                                             to overflow within the oracle's time; the batch needs 10
  ww-256-beb-q16     n = 130  BEB  round cap 5   window 16
  ww-256-beb-q32     n = 130  BEB  round cap 10  window 32
  ww-128-geo-q16     n = 70   BEB  round cap 5   window 16   geometric delays up to 16 (the DM = 16 build, per-link
                                                             delay planes; the reference protocol needs no more than
                                                             8 phases there before round 9)
  ww-128-nv2-q8      n = 70   REF  round cap 3   window 8, two key variants per origin (16 slots per replica lane)
  ww-128-v8-q16      n = 70   REF  round cap 5   window 16, BRC_FLAG_WIDE_VALUES: proposals of ids 4 .. 7
  ww-256-rec-q16     n = 130  REF  round cap 1   window 16, BRC_FLAG_WIDE_RECORDS: Byzantine origin 129 declares its
                                                 phase-0 key (slot 129 * 16 = 2064) and SENDs it to the low half; the
                                                 Byzantine replica 100 SENDs it to the rest one step later (an extra
                                                 SEND record) and ECHOes the key of origin 128 (slot 2048) to a
                                                 subset (a restricted record).  half = None: one round needs 3 phases;
                                                 the case pins the record words' key-slot field, not the window
"""
import random

from tests import interleaved_workloads as I
from tests import wide_values_workloads as V
from tests.golden import specs as S

OFFSET = I.OFFSET
REF, BEB = I.REF, I.BEB
UNIF, SLOW, GEO = I.UNIF, I.SLOW, I.GEO
CKEYS = I.CKEYS
COUNT = 8
BYZ70, BYZ130 = [5, 66], [7, 129]
BYZ130R = [7, 100, 129]
FLAG = 8                                     # include/brc.h BRC_FLAG_WIDE_WINDOWS


# the grid over which brc_create is held to accepted() (n, (delay model, delay_max), (key window, variants))
GRID_N = (70, 130)
GRID_DELAYS = ((I.CONST, 1), (SLOW, 4), (SLOW, 8), (UNIF, 4), (GEO, 8), (SLOW, 16), (UNIF, 16), (GEO, 16))
GRID_SLOTS = ((16, 1), (8, 2), (4, 4), (32, 1), (16, 2), (8, 4))


# ---- brc_create's rules for a flagged engine (csrc/brc_engine.hip, csrc/brc_internal.h) -------------------------
def lds_bytes_wide(npad, q, nv, xw, dm):
    """csrc/brc_internal.h lds_bytes_wide for the reference / best-effort protocols."""
    nk = npad * q * nv
    nkw, nw, rs = nk // 64, npad // 64, (16 if dm <= 8 else 32)
    return (8 * (nk + rs * nkw + min(nkw, 2) * npad + 4 * nw * npad + 2 * 4 * xw * 2 * nw + 16 * nw) +
            q * npad + 8 * nkw + 2 * nk + 4 * (12 + 2 * 4 * nw))


def xwords(model, dmax):
    dm = 4 if dmax <= 4 else 8 if dmax <= 8 else 16
    if model in (UNIF, GEO):
        return {4: 2, 8: 3, 16: 4}[dm] + 1
    return 1 if model == I.CONST or dmax == 1 else 2


def accepted(n, mode, q, nv, model=SLOW, dmax=8, conn=False, flag=True):
    """Does brc_create take (n > 64, key window q, nv variants)?  Without the flag: q * nv <= 8 (key_layout_workloads.
    accepted).  With it: sender peers, not SPEC, q * nv in (.. 8, 16, 32), and the LDS carve within 160 KB -- which
    leaves out exactly NPAD = 256 with q = 32 under uniform / geometric delays above 8 (the DM = 16 build's 32-row
    activity ring, five exchange words and a 32-deep deferred-SEND queue: 164,016 B)."""
    assert n > 64
    if not flag:
        return q * nv <= 8
    if conn or mode == I.SPEC or q * nv > 32:
        return False
    npad = 128 if n <= 128 else 256
    dm = 4 if dmax <= 4 else 8 if dmax <= 8 else 16
    return lds_bytes_wide(npad, q, nv, xwords(model, dmax), dm) <= 160 * 1024


def needs(exp, dmax):
    """The window the oracle's send log needs: the largest s_new - s_old + 1 over one origin's keys, where the key of
    phase index s_new was first SENT less than dmax steps after the last first-broadcast (SEND, ECHO or READY of any
    replica) of the key of s_old -- a proxy for the engine's t_quiet rule (brc_step_wide.h send_key)."""
    first, last = {}, {}
    for t, _src, typ, kp, s in exp["events"]["send"]:
        if typ == S.SEND:
            first.setdefault((kp, s), t)
        last[(kp, s)] = max(last.get((kp, s), 0), t)
    by = {}
    for (kp, s) in first:
        by.setdefault(kp, []).append(s)
    w = 0
    for kp, ss in by.items():
        ss.sort()
        for s2 in ss:
            old = next((s for s in ss if s < s2 and first[(kp, s2)] < last[(kp, s)] + dmax), None)
            if old is not None:
                w = max(w, s2 - old + 1)
    return w


def _cons(n, f, seed, model, dmax, byzs, cap, beb=False, nv=1, pat=None, extra=None, values=None):
    def make(g, i):
        mk = S.beb_cons_spec if beb else S.cons_spec
        sp = mk(n, f, seed, model, dmax, g, round_cap=cap, byzantine=byzs, nv=nv, proposals=pat(g, i) if pat else None,
                extra=extra(g, i) if extra else ())
        return dict(sp, values=values) if values else sp
    return make


def _build():
    out = []

    def add(name, npad, dm, mode, make, byzs, q, nv=1, half=True, rec=False, v8=False):
        c = I.Case(name, "wide%d" % npad, ("wide", npad, dm, mode, 0), make, COUNT, q, True, byz=byzs)
        c.q, c.nv, c.half, c.rec, c.v8 = q, nv, (q // 2 if half else None), rec, v8
        out.append(c)

    add("ww-128-ref-q16", 128, 8, REF, _cons(70, 23, 0x77AA0070, SLOW, 8, BYZ70, 5), BYZ70, 16)
    add("ww-128-ref-q32", 128, 8, REF, _cons(70, 23, 0x77AA0070, SLOW, 8, BYZ70, 9), BYZ70, 32)
    add("ww-128-beb-q16", 128, 8, BEB, _cons(70, 23, 0x77AA0070, SLOW, 8, BYZ70, 5, beb=True), BYZ70, 16)
    add("ww-128-beb-q32", 128, 8, BEB, _cons(70, 23, 0x77AA0070, SLOW, 8, BYZ70, 10, beb=True), BYZ70, 32)
    add("ww-256-ref-q16", 256, 8, REF, _cons(130, 43, 0x77AA0130, SLOW, 8, BYZ130, 4), BYZ130, 16)
    add("ww-256-ref-q32", 256, 8, REF, _cons(130, 43, 0x77AA0130, SLOW, 8, BYZ130, 4), BYZ130, 32, half=False)
    add("ww-256-beb-q16", 256, 8, BEB, _cons(130, 43, 0x77AA0130, SLOW, 8, BYZ130, 5, beb=True), BYZ130, 16)
    add("ww-256-beb-q32", 256, 8, BEB, _cons(130, 43, 0x77AA0130, SLOW, 8, BYZ130, 10, beb=True), BYZ130, 32)
    add("ww-128-geo-q16", 128, 16, BEB, _cons(70, 23, 0x77AA0070, GEO, 16, BYZ70, 5, beb=True), BYZ70, 16)
    add("ww-128-nv2-q8", 128, 8, REF, _cons(70, 23, 0x77AA0070, SLOW, 8, BYZ70, 3, nv=2), BYZ70, 8, nv=2)
    add("ww-128-v8-q16", 128, 8, REF,
        _cons(70, 23, 0x77AA0070, SLOW, 8, BYZ70, 5, values=S.VALUES8,
              pat=lambda g, i: V.majority(70, g, 4 + (g + i) % 4, 40, [v for v in range(1, 8) if v != 4 + (g + i) % 4])),
        BYZ70, 16, v8=True)

    def records(g, i):
        n, lo, hi = 130, 100, 129
        cut = 40 + (g * 7 + i) % 40
        low = (1 << cut) - 1
        sub = random.Random(0x77AAE000 + g).getrandbits(n) | 1 | 1 << 70 | 1 << 128
        return [dict(t=0, kind="byz_key", kp=hi, s=0, value=1 + i % 2),
                dict(t=0, kind="byz", src=hi, type=S.SEND, kp=hi, s=0, dst=low),
                dict(t=1, kind="byz", src=lo, type=S.SEND, kp=hi, s=0, dst=((1 << n) - 1) & ~low),
                dict(t=1, kind="byz", src=lo, type=S.ECHO, kp=128, s=0, dst=sub & ~(1 << 3))]
    add("ww-256-rec-q16", 256, 8, REF, _cons(130, 43, 0x77AA1130, SLOW, 8, BYZ130R, 1, extra=records), BYZ130R, 16,
        half=False, rec=True)
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


LOGGED = ("ww-128-ref-q16", "ww-256-beb-q16")        # also run with an event log
SLICED = "ww-128-ref-q32"                            # brc_run(max_steps = 7) repeated against one run
RESET = "ww-128-beb-q32"                             # brc_reset, then the same results
PARITY = "ww-128-par-q8"
SAME_SPECS = {"ww-256-ref-q32": "ww-256-ref-q16"}    # batches that differ in the engine's key window only
# the batches whose oracle runs are not held to ORACLE_SECONDS (tests/test_wide_window_workloads.py): the reference
# protocol at n = 130 needs round cap 4 before one origin keeps more than 8 phases in flight
SLOW_ORACLE = ("ww-256-ref-q16", "ww-256-ref-q32")


def oracle_results(case):
    """interleaved_workloads.oracle_results, computed once for batches of the same specs."""
    return I.oracle_results(by_name()[SAME_SPECS[case.name]] if case.name in SAME_SPECS else case)


def parity_case():
    """An existing wide shape (n = 70, reference protocol, window 8, round cap 2): flag off against flag on."""
    c = I.Case(PARITY, "wide128", ("wide", 128, 8, REF, 0), _cons(70, 23, 0x77AA0070, SLOW, 8, BYZ70, 2), COUNT, 8, True, byz=BYZ70)
    c.q, c.nv, c.half, c.rec, c.v8 = 8, 1, None, False, False
    return c
