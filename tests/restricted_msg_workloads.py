"""Workload table of tests/test_gpu_restricted_msg.py (GPU) and tests/test_restricted_msg_workloads.py (its
preconditions, on the oracle alone): a Byzantine replica ECHOes / READYs a key to a subset of the peers
(include/brc.h, "Restricted ECHO / READY") on every non-lean narrow step kernel.

A case is an interleaved_workloads.Case: one small batch, consecutive global ids from 777, one configuration,
action lists that differ per instance.  The instances of one packed wave item carry different destination sets
(drawn per instance), in four patterns by local id:

  0  ECHO to a subset at t0, READY to another subset one step later
  1  READY to a subset
  2  ECHO to every peer (the cell path), READY to a subset, then the ECHO again to a subset: every link is used,
     the remainder is empty (accepted, no record, no counter changes)
  3  ECHO to a subset, then the same ECHO to every peer: a record over the remaining links

Uniform per-link delays with D >= 3 spread one record's arrivals over several steps.  late: restricted records
without a time; Case stamps them with a step at which the instance has arrivals, and the at_now policy injects
them with t == t_now (the re-entered step).
"""
import random

from tests import interleaved_workloads as I
from tests.golden import specs as S

OFFSET = I.OFFSET
REF, SPEC, BEB, XREF = I.REF, I.SPEC, I.BEB, I.XREF
UNIF = I.UNIF
XSEND_MAX = I.XSEND_MAX
CKEYS = I.CKEYS


def ipw_of(n):
    return 1 if n > 32 else 64 // max(4, 1 << (n - 1).bit_length())


def subset(n, salt):
    """A proper, non-empty subset of the n peers."""
    return random.Random(0x2E57A000 + salt).randrange(1, (1 << n) - 1)


def msg(t, src, typ, key, dst):
    return dict(t=t, kind="byz", src=src, type=typ, kp=key[0], s=key[1], dst=dst)


def restricted(n, g, i, b, key, t0):
    """Instance i's pattern (module docstring) of Byzantine replica b on `key`, from step t0."""
    allm = (1 << n) - 1
    A, B = subset(n, 4 * g), subset(n, 4 * g + 1)
    p = i % 4
    if p == 0:
        return [msg(t0, b, S.ECHO, key, A), msg(t0 + 1, b, S.READY, key, B)]
    if p == 1:
        return [msg(t0 + 1, b, S.READY, key, B)]
    if p == 2:
        return [msg(t0, b, S.ECHO, key, allm), msg(t0 + 1, b, S.READY, key, B), msg(t0 + 2, b, S.ECHO, key, A)]
    return [msg(t0, b, S.ECHO, key, A), msg(t0 + 2, b, S.ECHO, key, allm)]


def byz_origin(b, n, value=0, payload=True):
    """Byzantine origin b declares key (b, 0) and SENDs it to every peer at step 0."""
    key = dict(t=0, kind="byz_key", kp=b, s=0, value=value)
    if payload:
        key["payload"] = "BYZ %d" % b
    return [key, dict(t=0, kind="byz", src=b, type=S.SEND, kp=b, s=0, dst=(1 << n) - 1)]


def widened(sp):
    """sp with every restricted ECHO / READY sent to all peers instead."""
    allm = (1 << sp["n"]) - 1
    return dict(sp, actions=[dict(a, dst=allm) if a["kind"] == "byz" and a["type"] != S.SEND else a for a in sp["actions"]])


def is_restricted(sp, a):
    return a["kind"] == "byz" and a["type"] != S.SEND and a["dst"] != (1 << sp["n"]) - 1


def table_records(specs):
    """Records each wave item's table holds when the batch is injected at once (nothing is pruned then), by
    brc_inject's rules: an extra SEND of a key already SENT and a Byzantine ECHO / READY over the links its
    (node, type, key) has not used (restricted, or after a restricted one) each take a record; records of one key,
    step, type and destination set merge.  {item: count}, and the instances with an empty remainder."""
    from oracle.oracle import expand_actions
    n = specs[0]["n"]
    allm, ipw = (1 << n) - 1, ipw_of(n)
    items, empty = {}, []
    for i, sp in enumerate(specs):
        recs, sent, sdst, used, hadrec = set(), {}, {}, {}, set()
        for a in expand_actions(sp["actions"], n):
            if a["kind"] == "brb_send" or (a["kind"] == "byz" and a["type"] == S.SEND):
                node, key = a.get("node", a.get("src")), (a["kp"], a["s"])
                dst = a.get("dst", allm) & ~sdst.get((node, key), 0)
                if sent.get(key, 0) and dst:
                    recs.add((key, a["t"], 0, dst))
                sent[key] = sent.get(key, 0) + 1
                sdst[(node, key)] = sdst.get((node, key), 0) | a.get("dst", allm)
            elif a["kind"] == "byz" and a["src"] in sp["byzantine"]:
                ident = (a["src"], a["type"], a["kp"], a["s"])
                dst = a["dst"]
                if dst != allm or ident in hadrec:
                    dst &= ~used.get(ident, 0)
                    hadrec.add(ident)
                    if dst:
                        recs.add(((a["kp"], a["s"]), a["t"], a["type"], dst))
                    else:
                        empty.append(i)
                used[ident] = used.get(ident, 0) | dst
        items[i // ipw] = items.get(i // ipw, 0) + len(recs)
    return items, empty


def _build():
    out = []

    def add(name, family, inst, make, count, consensus, key_window=8, late=None, byz=()):
        out.append(I.Case(name, family, inst, make, count, key_window, consensus, late=late, byz=byz))

    def brb(n, f, seed, byz, mode=None, every=1, general=False, dmax=4):
        b0, b1 = byz[0], byz[-1]

        def make(g, i):
            extra = byz_origin(b0, n)
            if i % every == 0:
                j = i // every
                # the honest origin's key and the Byzantine origin's key, alternating
                extra += restricted(n, g, j, b1, (0, 0) if j % 8 < 4 else (b0, 0), 1)
            sends = [(0, 0, 0)]
            if mode == "spec":
                sp = S.spec_brb_spec(n, f, seed, UNIF, dmax, g, sends, byzantine=byz, extra=extra, window=4)
            elif mode == "beb":
                sp = S.beb_spec(n, seed, UNIF, dmax, g, sends, byzantine=byz, extra=extra)
            else:
                sp = S.brb_spec(n, f, seed, UNIF, dmax, g, sends, byzantine=byz, extra=extra)
            return dict(sp, general_keys=True) if general else sp
        return make

    def cons(n, f, seed, byz, every=1, dmax=3):
        b0, b1 = byz[0], byz[-1]

        def make(g, i):
            extra = byz_origin(b0, n, value=1, payload=False)
            if b1 != b0:       # (one Byzantine replica: its ECHOes of its own key are the restricted ones)
                extra += [msg(1, b0, S.ECHO, (b0, 0), (1 << n) - 1)]
            if i % every == 0:
                j = i // every
                extra += restricted(n, g, j, b1, (j % (n - len(byz)), 0) if j % 8 < 4 else (b0, 0), 1)
            return S.cons_spec(n, f, seed, UNIF, dmax, g, round_cap=1, byzantine=byz, extra=extra)
        return make

    # NPAD 4 (16 instances per wave item): every second instance carries records, 12 in the full item
    add("rm-p4-ref-brb", "packed4", ("step", 4, 4, REF, 0), brb(4, 1, 0x2E570004, [3], every=2), 19, False, byz=[3])
    add("rm-p4-ref-cons", "packed4", ("step", 4, 4, REF, 0), cons(4, 1, 0x2E571004, [3], every=2), 19, True, byz=[3])
    # NPAD 8 (8 per item): 12 records in the full item; three instances get theirs at_now
    late8 = {i: [{k: v for k, v in a.items() if k != "t"} for a in restricted(7, OFFSET + i, 0, 6, (0, 0), 0)] for i in (1, 4, 9)}
    add("rm-p8-ref-brb", "packed8", ("step", 8, 4, REF, 0), brb(7, 2, 0x2E570008, [5, 6]), 11, False, late=late8, byz=[5, 6])
    add("rm-p8-ref-cons", "packed8", ("step", 8, 4, REF, 0), cons(7, 2, 0x2E571008, [5, 6]), 11, True, byz=[5, 6])
    add("rm-p8-beb-brb", "packed8", ("step", 8, 4, BEB, 0), brb(7, 0, 0x2E572008, [5, 6], mode="beb"), 9, False, byz=[5, 6])
    # NPAD 16 (4 per item)
    byz16 = [13, 14, 15]
    late16 = {i: [{k: v for k, v in a.items() if k != "t"} for a in restricted(16, OFFSET + i, 3, 15, (13, 0), 0)] for i in (0, 2, 5)}
    add("rm-p16-ref-brb", "packed16", ("step", 16, 4, REF, 0), brb(16, 5, 0x2E570010, byz16), 7, False, late=late16, byz=byz16)
    add("rm-p16-ref-cons", "packed16", ("step", 16, 4, REF, 0), cons(16, 5, 0x2E571010, byz16), 7, True, byz=byz16)
    add("rm-p16-spec-brb", "packed16", ("step", 16, 4, SPEC, 0), brb(16, 5, 0x2E572010, byz16, mode="spec"), 7, False,
        key_window=4, byz=byz16)
    # NPAD 32 (2 per item), delays up to 5
    byz32 = [22, 23, 24]
    add("rm-p32-ref-brb", "packed32", ("step", 32, 8, REF, 0), brb(25, 8, 0x2E570020, byz32, dmax=5), 5, False, byz=byz32)
    add("rm-p32-ref-cons", "packed32", ("step", 32, 8, REF, 0), cons(25, 8, 0x2E571020, byz32, dmax=5), 5, True, byz=byz32)
    # NPAD 64, general keys (one instance per wave)
    late64 = {1: [{k: v for k, v in a.items() if k != "t"} for a in restricted(40, OFFSET + 1, 0, 39, (0, 0), 0)]}
    add("rm-n64-xref-brb", "general64", ("step", 64, 4, XREF, 0), brb(40, 13, 0x2E570040, [38, 39], general=True), 3, False,
        late=late64, byz=[38, 39])

    # extra SENDs and restricted ECHO / READY records of ONE key injected at ONE step (NPAD 8): nodes 2 and 3 SEND
    # origin 0's payload again at step 2, where Byzantine 6 ECHOes it to one subset and READYs it to another
    def mix(g, i):
        n = 7
        extra = [dict(t=2, kind="brb_send", node=2 + j, kp=0, s=0, payload="TEST 1.0") for j in range(1 + i % 2)]
        extra += [msg(2, 6, S.ECHO, (0, 0), subset(n, 4 * g + 2)), msg(2, 6, S.READY, (0, 0), subset(n, 4 * g + 3)),
                  msg(3, 5, S.READY, (0, 0), subset(n, 4 * g))]
        return S.brb_spec(n, 2, 0x2E573008, UNIF, 4, g, [(0, 0, 0)], byzantine=[5, 6], extra=extra)
    add("rm-p8-mix-brb", "packed8", ("step", 8, 4, REF, 0), mix, 4, False, byz=[5, 6])
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


INTERLEAVED = ("rm-p8-ref-brb", "rm-p16-ref-brb", "rm-n64-xref-brb")


def overflow_spec():
    """n = 7, one instance: origin 0 SENDs XSEND_MAX + 1 keys, one step apart, and Byzantine 6 READYs each of them to
    a subset at step 40 -- one record each, injected at once: the last finds the table full."""
    n = 7
    sends = I.stream(0, XSEND_MAX + 1, 1)
    extra = [msg(40, 6, S.READY, (0, s), subset(n, 100 + s)) for (_t, _o, s) in sends]
    return dict(S.brb_spec(n, 2, 0x2E5700F0, UNIF, 3, OFFSET, sends, byzantine=[5, 6], extra=extra), name="overflow/0",
                step_cap=I.STEP_CAP, key_window=32)


oracle_results = I.oracle_results
