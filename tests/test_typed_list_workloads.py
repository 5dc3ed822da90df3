"""Preconditions of tests/test_gpu_typed_lists.py, on the oracle alone (no GPU): the cases of
tests/typed_list_workloads.py do the work they are meant to put in front of the type-sorted key list."""
import pytest

from oracle import oracle
from tests import typed_list_workloads as W
from tests.golden import specs as S


def test_case_names_are_unique_and_cover_both_modes():
    names = [c.name for c in W.cases()]
    assert len(names) == len(set(names))
    assert any("-ref-" in n for n in names) and any("-spec-" in n for n in names)


@pytest.mark.parametrize("mode", ["ref", "spec"])
def test_merge_case_brings_a_stored_key_word_up_again(mode):
    """At MERGE_STEP, under the consensus protocol, the typed list's walk over the delivering keys goes through key
    words 0, 1, ... in the READY segment (word 0 is stored when word 1 starts) and then to key word 0 again in the
    later ECHO + READY segment -- the store that has to merge with the word written earlier in the step.  The
    consensus pass depends on the merged word: exactly n - f keys deliver there, all of them are needed to end the
    phase, and the replicas that have proposed do end it at that step."""
    case = W.by_name()["typed-%s-merge" % mode]
    assert case.count >= 16 and case.key_window == W.MERGE_Q and case.consensus
    sp = case.specs[0]
    assert sp["mode"] in ("consensus", "spec")                   # the consensus pass reads the delivery words
    assert sp["delay_model"] == 0 and sp["dconst"] == 3          # every link three steps
    if mode == "spec":
        assert sp["window"] == W.MERGE_Q                         # the engine's key window on the SPEC kernels
    n, f = sp["n"], sp["f"]
    t0 = W.MERGE_T0[W.T.SPEC if mode == "spec" else W.T.REF]      # deliveries a phase end needs
    assert t0 == (n - f if mode == "spec" else n - f + 1)
    exp = oracle.run(sp)
    honest = {d for d in range(n) if d not in sp["byzantine"]}
    walk = W.delivery_word_walk(exp, W.MERGE_Q, W.MERGE_STEP, sp["dconst"])
    # t0 keys, all of phase 0: origins 0 .. t0 - 1, each delivered by every honest replica at MERGE_STEP
    assert sorted((kp, s) for _, kp, s, _ in walk) == [(o, 0) for o in range(t0)], walk
    for o in range(t0):
        got = {node for t, node, k, s in exp["events"]["deliver"] if (k, s) == (o, 0) and t == W.MERGE_STEP}
        assert got == honest, (o, sorted(got))
    # READY segment: words 0 (seven keys), 1, ..; then the ECHO + READY segment: key (1, 0), word 0 again
    ready, later = [e for e in walk if e[0] == "R"], [e for e in walk if e[0] != "R"]
    assert walk == ready + later and later == [("ER", 1, 0, 0)], walk
    words = [w for _, _, _, w in ready]
    assert words == sorted(words) and words.count(0) == 7 and set(words) == set(range((t0 + 7) // 8)), words
    a, b = words[0], words[7]
    order = W.SEGMENT_ORDER.index
    assert a == later[0][3] and b != a and order(later[0][0]) > order("R"), walk
    inj = [x for x in sp["actions"] if x["kind"] == "byz"]
    assert [(x["t"] + 3, x["type"], x["kp"], x["s"]) for x in inj] == [(W.MERGE_STEP, S.ECHO, 1, 0)]
    # the phase ends on exactly these deliveries: every replica that proposed at step 0 SENDs its phase-1 key at
    # MERGE_STEP, none earlier; one delivery fewer and it could not
    proposers = {a["node"] for a in sp["actions"] if a["kind"] == "propose" and a["t"] == 0}
    assert len(proposers) == t0
    sent1 = {}
    for t, node, typ, kp, s in exp["events"]["send"]:
        if typ == S.SEND and s == 1:
            sent1[node] = min(t, sent1.get(node, t))
    assert all(sent1.get(d) == W.MERGE_STEP for d in proposers), sorted(sent1.items())[:8]


@pytest.mark.parametrize("name", ["typed-ref-kdst", "typed-ref-stagger", "typed-ref-unif4-cap3", "typed-ref-n33"])
def test_cases_do_real_work(name):
    case = W.by_name()[name]
    exp = oracle.run(case.specs[0], kinds=("decide",))
    assert exp["status"] in ("done", "quiescent") and exp["cell_steps"] > 0 and exp["counts"]["deliver"] > 0, (name, exp["status"])
