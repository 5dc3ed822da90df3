#!/usr/bin/env python3
"""Generate tests/golden/wide_xsend/wide_xsend.json from the REAL reference (build container only).

    python -O tests/golden/wide_xsend/make_wide_xsend.py

A second SEND of one key above 64 replicas (the reference keys its broadcast state by the payload string,
core/brbroadcast.py:38-44, so a payload SENT by two nodes, or again by its own, is one key with several SENDs).
n = 70 (NPAD 128, two destination words), f = 23, Byzantine {68}, sender peers.  Origin 0's payload is SENT again by
node 65 and by node 0 itself, origin 66's payload is SENT by node 3 as well, and Byzantine replica 68 SENDs origin 0's
key to {1, 5, 63, 64, 69}.  Four runs: under uniform delays up to 4 and under slow-set delays up to 8, each with node
65's SEND ahead of node 0's repeat and with node 0's repeat ahead of every other node's.  Every spec runs through the
unmodified reference classes (``tests/golden/refharness.py``) and through the C oracle; the two must agree.  The JSON
holds the specs, the reference's results in ``golden_io``'s compact form, the oracle's cell-step counts and the wire
messages of the SENDs (what ``wire.Codec.to_injections`` replays).  ``-O``: see ``tests/golden/make_golden.py``.
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
N, F, SEED = 70, 23, 0x2E590070
BYZ = [68]
BYZ_DST = sum(1 << d for d in (1, 5, 63, 64, 69))


def again(t, node, key):
    return dict(t=t, kind="brb_send", node=node, kp=key[0], s=key[1], payload="TEST %d.%d" % (key[0] + 1, key[1]))


def brb_case(g, model, dmax, own_first):
    """Origins 0 and 66 SEND their payloads at step 0.  own_first False: node 65 SENDs origin 0's at step 0, node 0
    again at step 1; True: node 0 again at step 1, node 65 at step 2.  Node 3 SENDs origin 66's at step 2, Byzantine
    68 SENDs origin 0's key to BYZ_DST at step 1 (own_first: at step 2)."""
    extra = [again(2 if own_first else 0, 65, (0, 0)), again(1, 0, (0, 0)), again(2, 3, (66, 0)),
             dict(t=2 if own_first else 1, kind="byz", src=68, type=S.SEND, kp=0, s=0, dst=BYZ_DST)]
    return S.brb_spec(N, F, SEED, model, dmax, g, [(0, 0, 0), (0, 66, 0)], byzantine=BYZ, extra=extra, step_cap=400)


def all_specs():
    out = [brb_case(0, UNIF, 4, False), brb_case(1, SLOW, 8, False), brb_case(2, UNIF, 4, True), brb_case(3, SLOW, 8, True)]
    for i, sp in enumerate(out):
        sp["name"] = "wide_xsend/%d" % i
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
        # kept small: the event lists as counts and digests (compact()'s form for long runs), the DELIVER upcalls in
        # the reference's order, and the SENDs' wire messages [t, src, dst, envelope] grouped over their destinations
        # as [t, src, hex mask of dst, envelope] (tests/test_wide_xsend_workloads.wire_messages expands them)
        res = compact(ref)
        res["events"] = {"decide": res["events"]["decide"]}
        res["raw_order"] = {"deliver": res["raw_order"]["deliver"]}
        groups = {}
        for t, src, dst, env in ref["wire"]:
            if json.loads(env)["type"] == S.SEND:
                groups[(t, src, env)] = groups.get((t, src, env), 0) | 1 << dst
        cases.append({"spec": sp, "result": res, "cell_steps": orc["cell_steps"],
                      "wire_send": sorted([t, src, "%x" % m, env] for (t, src, env), m in groups.items())})
        print("%-14s %-10s t_stop %3d msgs %5d arrivals %5d cell_steps %5d" % (
            sp["name"], ref["status"], ref["t_stop"], ref["msgs_sent"], ref["arrivals"], orc["cell_steps"]))
    with open(os.path.join(HERE, "wide_xsend.json"), "w") as fh:
        json.dump({"group": "wide_xsend", "generator": "tests/golden/wide_xsend/make_wide_xsend.py",
                   "source": "unmodified reference classes via tests/golden/refharness.py", "cases": cases},
                  fh, separators=(",", ":"))


if __name__ == "__main__":
    main()
