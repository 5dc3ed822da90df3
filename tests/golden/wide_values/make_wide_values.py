#!/usr/bin/env python3
"""Generate tests/golden/wide_values/wide_values.json from the REAL reference (build container only).

    python -O tests/golden/wide_values/make_wide_values.py

More than three proposal strings above 64 replicas (the reference keys a replica's value table by the payload
string, core/byzantinerandomizedconsensus.py:57-60).  n = 70 (NPAD 128), f = 23, sender peers, ``values = VALUES8``,
round cap 2.  Three runs, the proposal patterns of ``cons_values_n40`` scaled to 70 replicas:

    0  uniform delays up to 4   a majority of id 4 ("alpha"), every other string of ids 1..5 present
    1  slow-set delays up to 8  a five-way split of ids 1..5, which ends in "-1"
    2  constant delay 1         a majority of id 5 ("beta") with a tail of ids 1..4

Every spec runs through the unmodified reference classes (``tests/golden/refharness.py``) and through the C oracle;
the two must agree.  The JSON holds the specs, the reference's results in ``golden_io``'s compact form cut down to
counts, digests, the decide events and the decide upcalls in the reference's order, and the oracle's cell-step
counts.  ``-O``: see ``tests/golden/make_golden.py``.  The cases run in three processes side by side; the harness
time of each is printed and recorded in the JSON (``harness_seconds``): 11 s, 100 s and 85 s on 8 cores, so every
case keeps round cap 2.

What the reference does with these settings: under uniform delays its broadcast stalls at this size (70 DELIVERs,
no decision, QUIESCENT at step 10 -- as in ``cons_uniform_n70``); under slow-set and constant delays every replica
decides twice, always "-1": with f = 23 a phase ends after n - f + 1 = 48 deliveries and needs 2 |hosts| > n + f = 93
for a value, and the 22 phase-1 messages still to come count in the phase-2 window.  The fixture therefore pins the
traffic, the steps and the decide upcalls of five-string runs to the reference; that a decision carries a new id is
held to the oracle by ``tests/wide_values_workloads.py`` (small f).
"""
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)

from oracle.schedule import Schedule  # noqa: E402
from oracle import oracle  # noqa: E402
from tests.golden import specs as S  # noqa: E402
from tests.golden.make_golden import compact, same  # noqa: E402
from tests.golden.refharness import run_spec  # noqa: E402

CONST, UNIF, SLOW = 0, 1, 2
N, F, SEED = 70, 23, 0x3B170070
PATTERNS = [[4] * 52 + [1, 2, 3, 5] * 4 + [5, 5],
            [1, 2, 3, 4, 5] * 14,
            [5] * 51 + [1, 2, 3, 4] * 4 + [4, 3, 2]]
MODELS = [(UNIF, 4), (SLOW, 8), (CONST, 1)]
ROUND_CAP = [2, 2, 2]


def all_specs():
    out = []
    for g, ((model, dmax), pat) in enumerate(zip(MODELS, PATTERNS)):
        assert len(pat) == N
        sp = dict(S.cons_spec(N, F, SEED + g, model, dmax, g, round_cap=ROUND_CAP[g], proposals=pat), values=S.VALUES8)
        sp["name"] = "wide_values/%d" % g
        out.append(sp)
    return out


def one_case(sp):
    t0 = time.time()
    ref = run_spec(sp, Schedule)
    dt = time.time() - t0
    orc = oracle.run(sp)
    if not same(ref, orc):
        return {"mismatch": [(k, ref[k], orc[k]) for k in ("status", "t_stop", "msgs_sent", "arrivals")]}
    res = compact(ref)
    raw = [list(r) for r in ref["events"]["decide"]]
    res["events"] = {"decide": res["events"]["decide"]}
    res["raw_order"] = {"decide": raw}
    return {"spec": sp, "result": res, "cell_steps": orc["cell_steps"], "harness_seconds": round(dt)}


def main():
    if __debug__:
        sys.exit("run with python -O (the reference asserts N > 5f)")
    specs = all_specs()
    with ProcessPoolExecutor(len(specs)) as pool:
        cases = list(pool.map(one_case, specs))
    for sp, c in zip(specs, cases):
        if "mismatch" in c:
            sys.exit("ORACLE MISMATCH in %s: %r" % (sp["name"], c["mismatch"]))
        r = c["result"]
        print("%-14s %-10s t_stop %3d msgs %7d arrivals %7d cell_steps %6d decide %3d  harness %5d s" % (
            sp["name"], r["status"], r["t_stop"], r["msgs_sent"], r["arrivals"], c["cell_steps"],
            r["counts"]["decide"], c["harness_seconds"]))
    with open(os.path.join(HERE, "wide_values.json"), "w") as fh:
        json.dump({"group": "wide_values", "generator": "tests/golden/wide_values/make_wide_values.py",
                   "source": "unmodified reference classes via tests/golden/refharness.py", "cases": cases},
                  fh, separators=(",", ":"))


if __name__ == "__main__":
    main()
