"""Comparisons of engine_runner.read_state() results, for the tests of tests/typed_list_workloads.py: two runs of one
batch field by field, and one run against the C oracle (through step_noevent_workloads.oracle_results).  The same
comparisons as tests/test_gpu_step_noevent.py makes for its own table; nothing is left out of either."""
from tests import step_noevent_workloads as T

CKEYS = ("status", "t_stop", "msgs_sent", "arrivals", "cell_steps")


def state_mismatches(a, b, what):
    """Differences between two read_state() results of one batch: every instances_result() field, every
    replicas() record, round_histogram, decisions and every stats() field."""
    out = []
    if len(a["inst"]) != len(b["inst"]):
        return [(what, "instances", len(a["inst"]), len(b["inst"]))]
    for i, (x, y) in enumerate(zip(a["inst"], b["inst"])):
        out += [(what, "inst", i, k, x[k], y[k]) for k in x if x[k] != y[k]]
    for i, (x, y) in enumerate(zip(a["reps"], b["reps"])):
        for d, (p, q) in enumerate(zip(x, y)):
            out += [(what, "replica", i, d, k, p[k], q[k]) for k in p if p[k] != q[k]]
    if a["hist"] != b["hist"]:
        out.append((what, "round_histogram", a["hist"], b["hist"]))
    if a["dec"] != b["dec"]:
        out.append((what, "decisions", a["dec"], b["dec"]))
    out += [(what, "stats", k, v, b["stats"][k]) for k, v in a["stats"].items() if v != b["stats"][k]]
    return out


def oracle_mismatches(case, st):
    """Differences from the oracle on the case's compared instances: status, t_stop, msgs_sent, arrivals,
    cell_steps, deliveries, and every honest replica's decide count, first decision and last decided value."""
    out = []
    byz = set(case.specs[0]["byzantine"])
    for i, (exp, dec, delivers) in T.oracle_results(case).items():
        r = st["inst"][i]
        out += [("oracle", i, k, r[k], exp[k]) for k in CKEYS if r[k] != exp[k]]
        if r["deliveries"] != delivers:
            out.append(("oracle", i, "deliveries", r["deliveries"], delivers))
        for d, rep in enumerate(st["reps"][i]):
            if d in byz:
                continue
            mine = dec.get(d, [])
            if rep["decide_count"] != len(mine):
                out.append(("oracle", i, d, "decide_count", rep["decide_count"], len(mine)))
            if mine:
                got = (rep["first_decide_round"], rep["first_decide_t"], rep["first_decide_value"])
                if got != mine[0]:
                    out.append(("oracle", i, d, "first decision", got, mine[0]))
                if rep["last_decide_value"] != mine[-1][2]:
                    out.append(("oracle", i, d, "last value", rep["last_decide_value"], mine[-1][2]))
        want = all(d in dec for d in range(case.specs[0]["n"]) if d not in byz) and case.consensus
        if bool(r["decided"]) != want:
            out.append(("oracle", i, "decided", r["decided"], want))
    return out
