"""Edge cases of the lean kernels' key-pair loop (NPAD = 64, sender peers, n = 64, f = 21; brc_step.h
process_pair and the LCHUNK-deep key pipeline around it): key lists whose lengths sit on the
pipeline's edges, a restricted-destination SEND in either seat of a pair, pairs whose two keys carry
different message types, and sends that mark ring rows for both delay classes and both types at once.
Each case runs under the constant-delay model (one delay class) and the slow-set model (two), on the
reference, SPEC and BEB instantiations, which share the loop.  Everything is bit-exact against the C oracle."""
import pytest

from oracle import oracle
from tests import golden_io
from tests.golden import specs as S

pytestmark = pytest.mark.gpu

N, F = 64, 21
BYZ = list(range(58, 64))
ALL64 = (1 << 64) - 1
LCHUNK = 8                     # brc_internal.h BRC_LCHUNK: key slots in flight on the lean kernels
# (delay model, dmax, dconst): one delay class (every link 3 steps) and two (slow set)
MODELS = {"const": (0, 8, 3), "slowset": (2, 8, 1)}


@pytest.fixture(scope="module")
def runner():
    from tests import engine_runner
    return engine_runner


def _check(got, specs):
    for sp, r in zip(specs, got):
        exp = oracle.run(sp)
        assert exp["status"] in ("done", "quiescent"), "%s: oracle status %s" % (sp["name"], exp["status"])
        exp["events"] = golden_io.canonical_events(exp["events"])
        for k in ("status", "t_stop", "msgs_sent", "arrivals", "cell_steps"):
            assert r[k] == exp[k], "%s %s: %r vs oracle %r" % (sp["name"], k, r[k], exp[k])
        for k in ("deliver", "decide", "send"):
            assert r["events"][k] == exp["events"][k], "%s: %s events differ" % (sp["name"], k)


def _spec(mode, model, g, sends, extra=(), seed=0x9A125):
    dm, dmax, dconst = MODELS[model]
    sp = S.brb_spec(N, F, seed, dm, dmax, g, sends, dconst=dconst, byzantine=BYZ, extra=extra, step_cap=400)
    if mode == "spec":
        sp.update(mode="spec_brb", window=4, coin_seed=0)
    elif mode == "beb":
        sp.update(mode="beb")
    sp["name"] = "pairs-%s-%s/%d" % (mode, model, g)
    return sp


def _restricted(kp, t, dst, src=None):
    """A Byzantine origin's SEND that reaches only the replicas of ``dst``."""
    return [dict(t=t, kind="byz_key", kp=kp, s=0, value=1),
            dict(t=t, kind="byz", src=kp if src is None else src, type=S.SEND, kp=kp, s=0, dst=dst)]


def edge_specs(mode, model):
    """Key-list lengths 1, 2, LCHUNK - 1, LCHUNK, LCHUNK + 1 and 2 LCHUNK + 1 (under one delay class
    every step of such a run carries exactly that many keys: the odd tail pair beside the padding
    entry, the refill that falls out of range, the entry's wait counts), and a restricted SEND among
    ordinary keys whose count puts it in each seat of a pair; the last one also carries a SEND that
    only reaches Byzantine replicas (no honest lane takes it: nobody sends, no ring mark)."""
    few = sum(1 << d for d in range(0, 10))
    only_byz = sum(1 << d for d in BYZ)
    out = []
    for g, nk in enumerate((1, 2, LCHUNK - 1, LCHUNK, LCHUNK + 1, 2 * LCHUNK + 1)):
        out.append(_spec(mode, model, g, [(0, o, 0) for o in range(nk)]))
    out.append(_spec(mode, model, 6, [(0, 0, 0)], extra=_restricted(60, 0, few)))
    out.append(_spec(mode, model, 7, [(0, 0, 0), (0, 1, 0)],
                     extra=_restricted(60, 0, few) + _restricted(61, 0, only_byz)))
    return out


def type_specs(mode, model):
    """Pairs whose keys carry different type sets in one step, built from Byzantine keys whose
    messages are injected at chosen steps (every link of the constant model takes 3 steps):
    g 0: an honest key's SEND beside a key receiving ECHO + READY;
    g 1: an honest key's READYs (its SEND went out six steps earlier) beside a key receiving SEND,
         ECHO and READY at once;
    g 2: both of the above in one run, with further honest keys started one step apart, so ECHO and READY
         sends of two keys fall into one step (ring marks of both types, and of both delay classes
         under the slow-set model)."""
    def er(kp, t, types):
        acts = [dict(t=t, kind="byz_key", kp=kp, s=0, value=1)]
        for src, ty in zip((61, 62, 63), types):
            acts.append(dict(t=t, kind="byz", src=kp if ty == S.SEND else src, type=ty, kp=kp, s=0, dst=ALL64))
        return acts
    a = _spec(mode, model, 0, [(5, 0, 0)], extra=er(60, 5, (S.ECHO, S.READY)))
    b = _spec(mode, model, 1, [(0, 0, 0)], extra=er(59, 6, (S.SEND, S.ECHO, S.READY)))
    c = _spec(mode, model, 2, [(0, 0, 0), (5, 1, 0)] + [(t, 2 + t, 0) for t in range(1, 8)],
              extra=er(60, 5, (S.ECHO, S.READY)) + er(59, 6, (S.SEND, S.ECHO, S.READY)))
    return [a, b, c]


@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("mode", ["reference", "spec", "beb"])
def test_key_list_edges_and_restricted_send(runner, mode, model):
    specs = edge_specs(mode, model)
    _check(runner.run_specs(specs), specs)


@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("mode", ["reference", "spec"])
def test_pairs_with_different_type_sets(runner, mode, model):
    specs = type_specs(mode, model)
    _check(runner.run_specs(specs), specs)
