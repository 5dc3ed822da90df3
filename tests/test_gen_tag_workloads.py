"""Preconditions of tests/test_gpu_gen_tags.py, on the oracle and in plain Python (no GPU): every epoch of every
walk does real work, the wrap schedules bring a slot back to a tag it wrote cells under while the host's earlier
book-keeping (max phase index / Q + 2 per epoch) sees nothing, and the full-clear schedules cross GEN_FULL_CLEAR
where the table says."""
import pytest

from tests import gen_tag_workloads as W
from tests.golden import specs as S

CASES = W.cases()
PARAMS = W.walk_params()


def _batches(case, walk):
    """The distinct batches of a walk: {tag: specs}."""
    return {tag: specs for tag, _off, specs in case.walk(walk)}


def test_table_names_every_tagged_family_and_walk():
    assert {c.family for c in CASES} == set(W.FAMILIES)
    assert {w for c in CASES for w in c.walks} == set(W.WALKS)
    for fam in W.FAMILIES:
        assert any("wrap" in c.walks for c in CASES if c.family == fam), fam
    for c in CASES:
        assert c.count <= 8 and set(c.walks) <= set(W.WALKS)
        for w in c.walks:
            for _tag, off, specs in c.walk(w):
                assert [sp["g"] for sp in specs] == list(range(off, off + c.count)) and off >= W.OFFSET
    # connection peers (5 words per cell) at NPAD 64 and NPAD 8, a SPEC case whose probed key wraps Q, BEB
    by = W.by_name()
    assert by["n40-conn"].msgs and by["n6-conn"].msgs and by["p8-spec"].probe_s >= by["p8-spec"].key_window
    # NPAD 4: the instances of the batch share one wave item
    assert by["p4"].count <= 16 and by["p4"].n == 4


@pytest.mark.parametrize("name,walk", PARAMS)
def test_every_epoch_does_real_work(name, walk):
    """No instance overflows on the oracle or runs into the step cap; every honest replica delivers the probed key,
    so a stale F_DEL cell read as current would show as missing deliveries."""
    case = W.by_name()[name]
    hon = {d for d in range(case.n) if d not in case.byz}
    for tag, specs in _batches(case, walk).items():
        for i, (exp, dec, _n) in W.oracle_results(W.Batch(case, walk, tag, specs)).items():
            sp = specs[i]
            if case.consensus:
                assert exp["status"] == "done" and all(len(dec.get(d, ())) >= sp["round_cap"] for d in hon), (sp["name"], exp["status"])
                if case.byz:          # the Byzantine replica's key of phase index S_BIG is delivered everywhere
                    assert {e[1] for e in exp["events"]["deliver"] if (e[2], e[3]) == (case.byz[0], W.S_BIG)} == hon
                continue
            assert exp["status"] == "quiescent", (sp["name"], exp["status"])
            got = {e[1] for e in exp["events"]["deliver"] if (e[2], e[3]) == tuple(sp["probe"])}
            assert got == hon, (sp["name"], sorted(hon - got))
            if case.msgs and walk != "full_clear":        # connection peers: the Byzantine replicas ECHO and READY the key, one of them twice
                raw = [(a["src"], a["type"]) for a in sp["actions"] if a["kind"] == "byz" and a["type"] != S.SEND]
                assert len(raw) > len(set(raw)) == 2 * len(case.byz)


@pytest.mark.parametrize("name,walk", [(n, w) for n, w in PARAMS if w in ("wrap", "wrap_at")])
def test_wrap_schedule_returns_to_a_written_tag(name, walk):
    case = W.by_name()[name]
    epochs = [specs for _tag, _off, specs in case.walk(walk)]
    assert len(epochs) == 8192 // W.K_WRAP + 8 and 8192 % W.K_WRAP == 0 and 8192 % W.K_ODD != 0
    Q = case.key_window
    # what the host booked before it counted records: + 2 per epoch (the probed key's phase index is below Q), far
    # from the full clear for the whole walk -- nothing came to the rescue
    assert case.probe_s // Q <= 1
    parent = [W.parent_gen_used(case.probe_s, Q)] * len(epochs)
    assert sum(parent) < W.GEN_FULL_CLEAR and W.host_walk(parent)[1] == []
    # the kernel's rule: instance 0 writes cells under one tag again after 8192 / K epochs; its siblings never do
    assert W.first_reuse(epochs, 0, Q) == 8192 // W.K_WRAP
    assert all(W.first_reuse(epochs, i, Q) is None for i in range(1, case.count))
    assert len({case.K(i) for i in range(case.count)}) >= 2
    # the odd epochs leave the probed slot's cells alone: its KEYs only, the delivered key sits in the next slot
    odd = epochs[1]
    assert all((sp["probe"][1] - case.probe_s) % Q == 1 for sp in odd) and all(sp["probe"][1] == case.probe_s for sp in epochs[0])
    # the host's count with the records in it: a full clear in time, every time
    excess = [W.excess_records(W.alloc_records(specs), False, Q) for specs in epochs]
    assert excess[0] == W.K_WRAP and excess[1] == W.K_WRAP - 1
    used = [W.gen_used(max(sp["probe"][1] for sp in specs), Q, x) for specs, x in zip(epochs, excess)]
    assert W.K_WRAP < min(used) and max(used) < W.GEN_HARD
    bases, clears = W.host_walk(used, [W.gen_used(0, Q, x) for x in excess])
    assert clears and all(W.first_reuse(epochs, i, Q, clears) is None for i in range(case.count))
    assert all(b + u < W.GEN_HARD for b, u in zip(bases, used))


def test_one_epoch_of_8192_keys_is_beyond_the_tags():
    """K = 8192 would bring the tag back within one epoch: the engine refuses it (test_gpu_gen_tags)."""
    assert W.gen_used(0, 4, 8192) >= W.GEN_HARD > W.gen_used(0, 4, W.K_WRAP)


@pytest.mark.parametrize("name", [c.name for c in CASES if "full_clear" in c.walks])
def test_full_clear_schedule_crosses_where_the_table_says(name):
    case = W.by_name()[name]
    epochs = case.walk("full_clear")
    Q = case.key_window
    used = [W.gen_used(W.S_BIG, Q, W.excess_records(W.alloc_records(specs), False, Q)) for _t, _o, specs in epochs]
    # a plain SEND is its key's one record; the restricted one comes as KEY + SEND, one record more
    assert used[0] == W.S_BIG // Q + 2 and used[1] == used[0] + 1
    bases, clears = W.host_walk(used)
    assert clears == [6], (bases, clears)
    assert bases[5] + used[5] >= W.GEN_FULL_CLEAR > bases[5] and bases[6] == 0 and bases[7] == used[6]
    assert len(epochs) >= 9          # the epoch before the clear, the clearing one and two after it
    # an engine that never cleared: from this epoch on S_BIG lies beyond s_limit (BRC_OVERFLOW: the walk fails)
    never, _ = W.host_walk(used, None, 1 << 30)
    over = [e for e, b in enumerate(never) if b + 3 < W.GEN_HARD and W.s_limit(b, Q) <= W.S_BIG or b + 3 >= W.GEN_HARD]
    assert over and over[0] < len(epochs), never
    # the two batches differ: values, and a restricted SEND in the odd one
    a, b = epochs[0][2], epochs[1][2]
    assert any(x["kind"] == "byz" and x["type"] == S.SEND and x["dst"] != (1 << case.n) - 1 for x in b[0]["actions"])
    assert {x.get("value", 0) for sp in a for x in sp["actions"]} != {x.get("value", 0) for sp in b for x in sp["actions"]}


def test_s_limit_numbers_follow_the_formula():
    case = W.by_name()["p8"]
    (_ta, _oa, first), (_tb, _ob, second), _third = case.walk("s_limit")
    Q = case.key_window
    assert Q == 2                     # the smallest key window brc_create takes
    base = W.gen_used(W.S_BIG, Q)
    assert base == W.S_BIG // Q + 2 and base < W.GEN_FULL_CLEAR       # no full clear before the second epoch
    lim = W.s_limit(base, Q)
    assert lim == (W.GEN_MASK - 3 - base) * Q < W.S_14BIT
    ss = [sp["probe"][1] for sp in second]
    assert ss[0] == lim - 1 and ss[1] == lim and all(s < Q * 8 for s in ss[2:])
    # the second epoch's own count: a full clear follows, the third epoch runs on a clean engine
    assert base + W.gen_used(lim - 1, Q) >= W.GEN_FULL_CLEAR


@pytest.mark.parametrize("name", [c.name for c in CASES if "consensus" in c.walks])
def test_consensus_walk_crosses_the_full_clear_once(name):
    case = W.by_name()[name]
    epochs = case.walk("consensus")
    specs = epochs[0][2]
    used = case.consensus_used(specs)
    bases, clears = W.host_walk([used] * len(epochs))
    assert len(clears) == 1 and 4 <= clears[0] < len(epochs) - 2 and len(epochs) <= 200, (used, clears, len(epochs))
    assert case.smax(specs) >= 2 * case.key_window          # the phase indices wrap the window many times over
    # an engine that never cleared is out of tags before the walk ends
    never, _ = W.host_walk([used] * len(epochs), None, 1 << 30)
    assert never[-1] + used >= W.GEN_HARD
    assert case.inst[1] == (16 if name == "c16-ref" else 8)


def test_slowset4_batches_put_slow_replicas_beside_each_other():
    """The n = 4 slow-set batches of test_gpu_gen_tags: every instance does real work on the oracle, and within the
    full wave item neighbouring instances have different slow replicas (a neighbour's slow lane read as a sender
    of this instance changes the arrivals)."""
    from oracle import oracle
    from oracle.schedule import Schedule
    for kind, specs in W.slowset4_specs().items():
        assert len(specs) == 19 and all(sp["n"] == 4 and sp["delay_model"] == W.SLOW for sp in specs)
        sch = Schedule(4, 1, specs[0]["seed"], W.SLOW, specs[0]["dmax"], 1)
        slow = [tuple(d for d in range(4) if sch.is_slow(sp["g"], d)) for sp in specs]
        assert all(len(x) == 1 for x in slow)
        assert len(set(slow[:16])) >= 3, (kind, slow)
        for sp in specs:
            exp = oracle.run(sp, light=True)
            assert exp["status"] in ("done", "quiescent") and exp["counts"]["deliver"] >= 3, (sp["name"], exp)
