"""SPEC modes: the C oracle's restatement (oracle/brc_oracle.c) against the independent pure-Python
model (tests/spec_model.py) on random small workloads -- honest runs, coin rounds, Byzantine
silence and equivocation, staggered starts, every delay model and key window.  The reference
cannot run these modes, so this agreement is what pins their parity."""
import random

import pytest

from oracle import oracle
from tests import golden_io, spec_model
from tests.golden import specs as S


def _check(sp):
    exp = spec_model.run(sp)
    got = oracle.run(sp)
    for k in ("status", "t_stop", "msgs_sent", "arrivals"):
        assert got[k] == exp[k], "%s %s: oracle %r model %r" % (sp["name"], k, got[k], exp[k])
    a, b = golden_io.canonical_events(got["events"]), golden_io.canonical_events(exp["events"])
    for k in ("deliver", "decide", "send"):
        assert a[k] == b[k], "%s: %s events differ" % (sp["name"], k)
    return got


def _random_specs(seed, count, variants=False):
    """variants: Byzantine runs draw nv from {2, 4} and a split of specs.variant_actions (every variant of an origin in
    use); the draws of the existing chunks are unchanged without it."""
    rng = random.Random(seed)
    out = []
    for i in range(count):
        n = rng.choice([4, 5, 6, 7, 8, 10, 13])
        f = rng.randint(0, (n - 1) // 3)
        model = rng.randint(0, 3)
        dmax = rng.randint(1, 6) if model else 1
        window = rng.choice([2, 4, 8])
        g = rng.getrandbits(20)
        if rng.random() < 0.25:
            sends = [(rng.randint(0, 5), o, q) for o in range(n) for q in range(rng.randint(0, 2))]
            sp = S.spec_brb_spec(n, f, rng.getrandbits(40), model, dmax, g, sends, window=window)
        else:
            byz = rng.sample(range(n), rng.randint(0, f))
            extra = []
            nv = 2
            if variants and f and not byz:
                byz = rng.sample(range(n), rng.randint(1, f))
            if variants and byz:
                nv = rng.choice([2, 4])
                if len(byz) <= n - nv:
                    extra = S.variant_actions(n, byz, nv, rng.choice(["even", "skewed"]))
                    window = 2 if nv == 4 else rng.choice([2, 4])       # the engine's limit: Q * NV <= 8 under SPEC
            elif byz and rng.random() < 0.5:
                extra = S.equivocation_actions(n, byz)
            starts = None if rng.random() < 0.6 else [rng.choice([0, 0, rng.randint(1, 8)]) for _ in range(n)]
            sp = S.spec_cons_spec(n, f, rng.getrandbits(40), model, dmax, g, round_cap=rng.randint(1, 4),
                                  window=window, coin_seed=rng.getrandbits(40), byzantine=byz,
                                  nv=nv if extra else 1, extra=extra, starts=starts, step_cap=3000)
        sp["name"] = "specfuzz/%d" % i
        out.append(sp)
    return out


@pytest.mark.parametrize("chunk", range(4))
def test_oracle_spec_matches_model(chunk):
    for sp in _random_specs(1000 + chunk, 40):
        _check(sp)


@pytest.mark.parametrize("chunk", range(2))
def test_oracle_spec_matches_model_with_every_variant(chunk):
    """Two and four key variants per origin (specs.variant_actions, both splits): the `seen` host masks of
    spec_deliver are indexed by the host kp // nv."""
    specs = _random_specs(2000 + chunk, 60, variants=True)
    assert sum(sp["nv"] == 4 for sp in specs) >= 5 and sum(sp["nv"] == 2 for sp in specs) >= 5
    for sp in specs:
        _check(sp)


def _fault_bound_specs(seed, count):
    """f from the whole range 0 .. n - 1 and committees down to n = 1 (the draws above stop at (n - 1) // 3 and n = 4):
    the four thresholds where n - f is 1 or 2, where 2 f + 1 exceeds n, and with n + f of both parities.  SPEC above
    its fault bound may flip coins for ever, so the step cap is low; a stop there is compared like any other."""
    rng = random.Random(seed)
    out = []
    for i in range(count):
        n = rng.choice([1, 2, 3, 1, 2, 3, 4, 5, 7, 10])
        f = rng.randint(0, n - 1)
        model = rng.randint(0, 3)
        dmax = rng.randint(1, 5) if model else 1
        window = rng.choice([2, 4, 8])
        g = rng.getrandbits(20)
        byz = rng.sample(range(n), rng.randint(0, min(f, n - 1, 2))) if rng.random() < 0.4 else []
        kind = rng.random()
        if kind < 0.25:
            sends = [(rng.randint(0, 5), o, q) for o in range(n) if o not in byz for q in range(rng.randint(0, 2))]
            sp = S.spec_brb_spec(n, f, rng.getrandbits(40), model, dmax, g, sends, window=window, byzantine=byz)
        elif kind < 0.4:
            sends = [(rng.randint(0, 5), o, q) for o in range(n) if o not in byz for q in range(rng.randint(0, 2))]
            sp = S.beb_spec(n, rng.getrandbits(40), model, dmax, g, sends, byzantine=byz)
            sp["f"] = f                                   # (the slow set's size; best-effort broadcast has no quorum)
        else:
            sp = S.spec_cons_spec(n, f, rng.getrandbits(40), model, dmax, g, round_cap=rng.randint(1, 3), window=window,
                                  coin_seed=rng.getrandbits(40), byzantine=byz, step_cap=150)
        sp["name"] = "specfault/%d" % i
        out.append(sp)
    return out


@pytest.mark.parametrize("chunk", range(3))
def test_oracle_spec_matches_model_over_the_whole_fault_range(chunk):
    specs = _fault_bound_specs(3000 + chunk, 60)
    assert sum(sp["n"] <= 3 for sp in specs) >= 20 and sum(sp["f"] > (sp["n"] - 1) // 3 for sp in specs) >= 15
    assert any(sp["f"] == sp["n"] - 1 and sp["n"] > 1 for sp in specs) and any(sp["f"] == 0 for sp in specs)
    ended = 0
    for sp in specs:
        r = _check(sp)
        ended += any(e[2] == 1 and e[4] >= 1 for e in r["events"]["send"])
    assert ended >= 10, ended                             # phase ends happen: the draws are not all stalls


def test_spec_coin_rounds_happen():
    """With an even split the phase-2 tallies stay at or below f, so the common coin decides the
    next estimate; every honest replica still decides, and all decide the same value."""
    seen_coin = False
    for g in range(20):
        sp = S.spec_cons_spec(7, 2, 0xC0, 2, 3, g, round_cap=1, window=4, coin_seed=99,
                              proposals=[1, 2, 1, 2, 1, 2, 1])
        sp["name"] = "coin/%d" % g
        r = _check(sp)
        assert r["status"] == "done"
        dec = r["events"]["decide"]
        assert len({d[3] for d in dec}) == 1, "agreement"
        seen_coin |= max(d[2] for d in dec) > 1
    assert seen_coin, "no instance needed a coin round"


def test_oracle_beb_matches_model():
    """Best-effort broadcast: the C oracle's beb_on_message against the model."""
    rng = random.Random(44)
    for i in range(60):
        n = rng.choice([3, 4, 7, 10, 16])
        model = rng.randint(0, 3)
        dmax = rng.randint(1, 6) if model else 1
        sends = [(rng.randint(0, 6), o, q) for o in range(n) for q in range(rng.randint(0, 2))]
        byz = rng.sample(range(n), rng.randint(0, n // 3))
        sp = S.beb_spec(n, rng.getrandbits(40), model, dmax, rng.getrandbits(20),
                        [x for x in sends if x[1] not in byz], byzantine=byz)
        sp["name"] = "beb/%d" % i
        r = _check(sp)
        honest = n - len(byz)
        assert len(r["events"]["deliver"]) == honest * len([x for x in sends if x[1] not in byz])
