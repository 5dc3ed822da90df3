#!/usr/bin/env python3
"""Generate tests/golden/fault_bounds/fault_bounds.json from the REAL reference (build container only).

    python -O tests/golden/fault_bounds/make_fault_bounds.py

Fault bounds off f = (n - 1) // 3 and committees below 4.  tests/golden/make_golden.py draws f from 0 .. (n - 1) // 3 and
n from 4 up, so the other fixtures pin the oracle's four thresholds (> n - f, 2 * count > n + f, > 2 * f, > f) only where
a slip in one of them can coincide with the right answer.  Every spec here runs through the unmodified reference classes
(``tests/golden/refharness.py``, unchanged) and through the C oracle; the two must agree.  The JSON holds the specs, the
reference's results in ``golden_io``'s compact form (raw upcall order included) and the oracle's cell-step counts.
``-O``: see ``tests/golden/make_golden.py``.

n in {1, 2, 3, 4, 7, 10}, f from {0, (n - 1) // 3 + 1, ceil(n / 2), n - 1}, the broadcast and the consensus protocol,
slow-set and uniform delays.  The regimes (tests/test_fault_bound_workloads.py asserts them on the stored results):

  * n + f odd and n + f even (the ECHO quorum 2 * count > n + f);
  * 2 * f + 1 above the honest replicas: no READY quorum, nothing is delivered (n = 2 f = 1, n = 4 f = 2, n = 7 f = 4,
    n = 10 f = 5, every f = n - 1 above n = 1, and n = 7 f = 3 with one silent replica);
  * n - f <= 2 (n = 1 f = 0, n = 2 f = 0, n = 3 f = 1): the reference ends a phase on delivery n - f + 1 (its ``>``), so
    n = 3 f = 1 ends one on the third delivery, and n = 2 f = 0 -- two origins, two deliveries, a count that EQUALS
    n - f -- never does;
  * f = 0: no slow replica; f = n - 1: one fast replica.
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
SEED = 0xFB0D0000


def f_choices(n):
    return sorted({0, (n - 1) // 3 + 1, (n + 1) // 2, n - 1} & set(range(n)))


def brb(n, f, model, dmax, g, byz=()):
    honest = [o for o in range(n) if o not in byz]
    sends = [(i % 3, o, 0) for i, o in enumerate(honest)]
    return S.brb_spec(n, f, SEED + 16 * n + f, model, dmax, g, sends, byzantine=byz, step_cap=400)


def cons(n, f, model, dmax, g, cap, byz=()):
    return S.cons_spec(n, f, SEED + 0x1000 + 16 * n + f, model, dmax, g, round_cap=cap, byzantine=byz, step_cap=400)


def all_specs():
    out = [brb(1, 0, SLOW, 3, 0),                   # n + f odd; the one replica delivers its own key
           cons(1, 0, UNIF, 3, 1, 1),               # one delivery = n - f: no phase end
           cons(2, 0, SLOW, 2, 2, 2),               # n + f even; two deliveries = n - f: no phase end
           brb(2, 1, UNIF, 3, 3),                   # n + f odd; READY quorum 3 of 2 replicas
           cons(3, 1, UNIF, 2, 4, 2),               # n + f even; n - f = 2: a phase ends on the third delivery
           brb(3, 2, SLOW, 3, 5),                   # f = n - 1: one fast replica
           cons(4, 0, SLOW, 4, 6, 2),               # f = 0: no slow replica
           cons(4, 2, UNIF, 3, 7, 1),               # READY quorum 5 of 4 replicas
           brb(4, 3, SLOW, 2, 8),
           cons(7, 3, SLOW, 3, 9, 2),               # READY quorum 7 of 7: every replica is needed
           cons(7, 3, SLOW, 3, 10, 1, byz=[6]),     # ... and one is silent: nothing is delivered
           brb(7, 4, UNIF, 4, 11),                  # n + f odd; READY quorum 9 of 7
           brb(7, 0, UNIF, 2, 12),
           cons(10, 4, SLOW, 3, 13, 1),             # n + f even: ECHO quorum 8, READY quorum 9 of 10
           brb(10, 5, UNIF, 3, 14),                 # n + f odd; READY quorum 11 of 10
           brb(10, 9, SLOW, 2, 15)]
    for i, sp in enumerate(out):
        assert sp["f"] in f_choices(sp["n"]), (sp["n"], sp["f"])
        sp["name"] = "fault_bounds/%d" % i
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
        cases.append({"spec": sp, "result": compact(ref), "cell_steps": orc["cell_steps"]})
        print("%-18s n %2d f %d %-9s %-10s t_stop %3d msgs %5d arrivals %5d deliver %3d decide %2d" % (
            sp["name"], sp["n"], sp["f"], sp["mode"], ref["status"], ref["t_stop"], ref["msgs_sent"], ref["arrivals"],
            len(ref["events"]["deliver"]), len(ref["events"]["decide"])))
    with open(os.path.join(HERE, "fault_bounds.json"), "w") as fh:
        json.dump({"group": "fault_bounds", "generator": "tests/golden/fault_bounds/make_fault_bounds.py",
                   "source": "unmodified reference classes via tests/golden/refharness.py", "cases": cases},
                  fh, separators=(",", ":"))


if __name__ == "__main__":
    main()
