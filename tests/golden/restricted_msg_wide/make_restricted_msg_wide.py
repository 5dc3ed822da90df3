#!/usr/bin/env python3
"""Generate tests/golden/restricted_msg_wide/restricted_msg_wide.json from the REAL reference (build container only).

    python -O tests/golden/restricted_msg_wide/make_restricted_msg_wide.py

The wide-committee sibling of tests/golden/restricted_msg/: n = 70 (NPAD 128, two destination words), f = 23,
broadcast under uniform delays up to 4.  Byzantine replica 68 ECHOes the honest origin's key to a subset with members
below and above replica 64, and READYs it to another such subset one step later; a second pair of runs has it ECHO the
key to every peer afterwards (the links it used carry nothing again).  Every spec runs through the unmodified
reference classes (``tests/golden/refharness.py``: ``byz_send`` puts one raw message on each link of a destination
mask) and through the C oracle; the two must agree.  The JSON holds the specs, the reference's results in
``golden_io``'s compact form, the oracle's cell-step counts and the wire messages the Byzantine replicas sent (what
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

UNIF = 1
N, F, SEED, DMAX = 70, 23, 0x2E570070, 4
BYZ = [68]
# both sets have members on either side of replica 64 (the second destination word starts there)
ECHO_DST = sum(1 << d for d in list(range(0, 40, 3)) + [41, 63, 64, 66, 69])
READY_DST = sum(1 << d for d in list(range(1, 64, 2)) + [65, 67, 68])


def brb_case(g, again=None):
    """Honest origin 0 SENDs its key; Byzantine 68 ECHOes it to ECHO_DST at step 1 and READYs it to READY_DST at
    step 2; again: the step at which 68 ECHOes it to every peer."""
    allm = (1 << N) - 1
    extra = [dict(t=1, kind="byz", src=68, type=S.ECHO, kp=0, s=0, dst=ECHO_DST),
             dict(t=2, kind="byz", src=68, type=S.READY, kp=0, s=0, dst=READY_DST)]
    if again is not None:
        extra.append(dict(t=again, kind="byz", src=68, type=S.ECHO, kp=0, s=0, dst=allm))
    return S.brb_spec(N, F, SEED, UNIF, DMAX, g, [(0, 0, 0)], byzantine=BYZ, extra=extra, step_cap=400)


def all_specs():
    out = [brb_case(0), brb_case(1, again=3)]
    for i, sp in enumerate(out):
        sp["name"] = "restricted_msg_wide/%d" % i
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
        print("%-26s %-10s t_stop %3d msgs %5d arrivals %5d" % (sp["name"], ref["status"], ref["t_stop"],
                                                              ref["msgs_sent"], ref["arrivals"]))
    with open(os.path.join(HERE, "restricted_msg_wide.json"), "w") as fh:
        json.dump({"group": "restricted_msg_wide",
                   "generator": "tests/golden/restricted_msg_wide/make_restricted_msg_wide.py",
                   "source": "unmodified reference classes via tests/golden/refharness.py", "cases": cases},
                  fh, separators=(",", ":"))


if __name__ == "__main__":
    main()
