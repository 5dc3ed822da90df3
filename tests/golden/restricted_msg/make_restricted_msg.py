#!/usr/bin/env python3
"""Generate tests/golden/restricted_msg/restricted_msg.json from the REAL reference (build container only).

    python -O tests/golden/restricted_msg/make_restricted_msg.py

A Byzantine replica ECHOes / READYs a payload to part of the committee only (include/brc.h, "Restricted
ECHO / READY").  Every spec runs through the unmodified reference classes (``tests/golden/refharness.py``,
unchanged: its ``byz_send`` puts one raw message on each link of a destination mask) and through the C
oracle; the two must agree.  The JSON holds the specs, the reference's results in ``golden_io``'s compact
form, the oracle's cell-step counts, and the wire messages the Byzantine replicas sent (what
``wire.Codec.to_injections`` replays).  ``-O``: see ``tests/golden/make_golden.py``.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)

from oracle.schedule import Schedule  # noqa: E402
from oracle import oracle  # noqa: E402
from tests.golden import specs as S  # noqa: E402
from tests.golden.make_golden import compact, same  # noqa: E402
from tests.golden.refharness import run_spec  # noqa: E402

UNIF, SLOW = 1, 2


def halves(n):
    lo = (1 << ((n + 1) // 2)) - 1
    return lo, ((1 << n) - 1) & ~lo


def brb_case(n, f, seed, model, dmax, g, byz, t_echo, t_ready, again=None):
    """Byzantine origin byz[0] SENDs its key to all; byz[1] ECHOes it to the low half of the committee at
    t_echo and READYs it to the high half at t_ready; again: the step at which byz[1] ECHOes it to all."""
    b, c = byz[0], byz[1]
    allm = (1 << n) - 1
    lo, hi = halves(n)
    extra = [dict(t=0, kind="byz_key", kp=b, s=0, value=0, payload="BYZ %d" % b),
             dict(t=0, kind="byz", src=b, type=S.SEND, kp=b, s=0, dst=allm),
             dict(t=t_echo, kind="byz", src=c, type=S.ECHO, kp=b, s=0, dst=lo),
             dict(t=t_ready, kind="byz", src=c, type=S.READY, kp=b, s=0, dst=hi)]
    if again is not None:
        extra.append(dict(t=again, kind="byz", src=c, type=S.ECHO, kp=b, s=0, dst=allm))
    return S.brb_spec(n, f, seed, model, dmax, g, [(0, 0, 0)], byzantine=byz, extra=extra, step_cap=400)


def cons_case(g):
    """n = 7, round cap 1: Byzantine origin 5 proposes "0" to all; Byzantine replica 6 ECHOes that key and the
    honest proposals' keys of origins 0..2 to a subset each."""
    n, byz = 7, [5, 6]
    allm = (1 << n) - 1
    extra = [dict(t=0, kind="byz_key", kp=5, s=0, value=1),
             dict(t=0, kind="byz", src=5, type=S.SEND, kp=5, s=0, dst=allm),
             dict(t=1, kind="byz", src=5, type=S.ECHO, kp=5, s=0, dst=allm),
             dict(t=1, kind="byz", src=6, type=S.ECHO, kp=5, s=0, dst=0b0010110)]
    extra += [dict(t=1 + o, kind="byz", src=6, type=S.ECHO, kp=o, s=0, dst=(0b0101011 << o) & allm) for o in range(3)]
    extra += [dict(t=3, kind="byz", src=6, type=S.READY, kp=1, s=0, dst=0b1001001)]
    return S.cons_spec(n, 2, 0x2E570003, UNIF, 4, g, round_cap=1, byzantine=byz, extra=extra, step_cap=400)


def all_specs():
    out = [brb_case(7, 2, 0x2E570001, UNIF, 4, g, [5, 6], 1, 2) for g in range(2)]
    out += [brb_case(16, 5, 0x2E570002, SLOW, 8, g, [11, 12, 13, 14, 15], 1, 3) for g in range(2)]
    out += [brb_case(7, 2, 0x2E570001, UNIF, 4, 2 + g, [5, 6], 1, 2, again=4) for g in range(2)]
    out += [cons_case(g) for g in range(2)]
    for i, sp in enumerate(out):
        sp["name"] = "restricted_msg/%d" % i
    return out


def main():
    if __debug__:
        sys.exit("run with python -O (the reference asserts N > 5f)")
    cases = []
    for sp in all_specs():
        ref = run_spec(sp, Schedule)
        orc = oracle.run(sp)
        if not same(ref, orc):
            sys.exit("ORACLE MISMATCH in %s: %r" % (sp["name"], [(k, ref[k], orc[k]) for k in
                                                                 ("status", "t_stop", "msgs_sent", "arrivals")]))
        byz = set(sp["byzantine"])
        cases.append({"spec": sp, "result": compact(ref), "cell_steps": orc["cell_steps"],
                      "wire_byz": sorted(w for w in ref["wire"] if w[1] in byz)})
        print("%-22s %-10s t_stop %3d msgs %5d arrivals %5d" % (sp["name"], ref["status"], ref["t_stop"],
                                                              ref["msgs_sent"], ref["arrivals"]))
    with open(os.path.join(HERE, "restricted_msg.json"), "w") as fh:
        json.dump({"group": "restricted_msg", "generator": "tests/golden/restricted_msg/make_restricted_msg.py",
                   "source": "unmodified reference classes via tests/golden/refharness.py", "cases": cases},
                  fh, separators=(",", ":"))


if __name__ == "__main__":
    main()
