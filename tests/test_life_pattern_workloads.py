"""Preconditions of tests/test_gpu_life_pattern.py, on the C oracle alone (no GPU): every batch of
tests/life_pattern_workloads.py is what the table says (Byzantine replicas of both parities, delay classes and waves; a
mask per instance; instances that decide and instances that stall), the small-f committees deliver equivocated keys --
one variant at f = 1, both at f = 0 -- and no batch needs more than its key window.  Plus the binding's side of the
interface: the flag bit, the ABI version, the Python mirror of the LDS carve."""
import pytest

from tests import life_pattern_workloads as LP
from tests import wide_window_workloads as W

NAMES = [b.name for b in LP.batches()]
ORACLE_SECONDS = 90.0                        # every oracle run of the module together, wall clock
_TOOK = []


def _results(batch):
    if not _TOOK:
        _TOOK.append(LP.oracle_all())
    return LP.oracle_results(batch)


@pytest.mark.parametrize("name", NAMES)
def test_batch_preconditions(name):
    b = LP.by_name()[name]
    specs = b.specs
    sp0 = specs[0]
    n = sp0["n"]
    assert len(specs) == LP.COUNT == 8
    assert 64 < n <= 256 and sp0.get("peer_mode", "sender") == "sender" and sp0["nv"] == b.nv and b.nv in (2, 4)
    assert sp0["mode"] in ("consensus", "beb_consensus")
    assert sp0["delay_model"] in (LP.CONST, LP.SLOW) and sp0["dmax"] <= 8
    assert b.q * b.nv <= (32 if b.wide_windows else 8)
    npad = 128 if n <= 128 else 256
    assert LP.lds_bytes_life_wide(npad, b.q, b.nv, False, True) <= 160 * 1024
    for sp in specs:
        # the Byzantine actions are exactly the engine's pattern for the instance's mask; everything else proposes at 0
        from tests.golden import specs as S
        byz = sp["byzantine"]
        assert byz == sorted(byz) and all(0 <= x < n for x in byz)
        assert [a for a in sp["actions"] if a["kind"] != "propose"] == S.equivocation_actions(n, byz, nv=b.nv)
        assert all(a["t"] == 0 for a in sp["actions"] if a["kind"] == "propose")
        assert sorted(a["node"] for a in sp["actions"] if a["kind"] == "propose") == [d for d in range(n) if d not in byz]
    if not b.load_masks:
        assert all(sp["byzantine"] == sp0["byzantine"] for sp in specs) and sp0["byzantine"]
    res = _results(b)
    status = [exp["status"] for (exp, _dec, _n) in res.values()]
    need = [W.needs(exp, sp0["dmax"]) for (exp, _dec, _n) in res.values()]
    print(name, status, [exp["t_stop"] for (exp, _dec, _n) in res.values()], need)
    assert all(s in ("done", "quiescent") for s in status), status          # no instance left running, none at the cap
    assert all(exp["t_stop"] < sp0["step_cap"] for (exp, _dec, _n) in res.values())
    assert max(need) <= b.q, need                                           # no overflow (the send log's window)
    assert all(exp["t_stop"] >= 1 for sp, (exp, _dec, _n) in zip(specs, res.values()) if sp["byzantine"])


def test_masks_batch_covers_parities_classes_and_extremes():
    b = LP.by_name()["lp-128-ref-masks"]
    assert b.load_masks and len({tuple(sp["byzantine"]) for sp in b.specs}) >= 6
    assert b.specs[0]["byzantine"] == [] and len(b.specs[1]["byzantine"]) == b.specs[1]["f"] == 23
    for sp in b.specs[2:]:
        slow = set(LP.slow_set(70, 23, sp["seed"], sp["delay_model"], sp["dmax"], sp["g"]))
        kinds = {(x in slow, x & 1) for x in sp["byzantine"]}
        assert kinds == {(False, 0), (False, 1), (True, 0), (True, 1)}, (sp["name"], sp["byzantine"], kinds)
    assert all(min(LP.class_sizes4(sp)) > 0 for sp in b.specs)             # four non-empty honest classes
    res = _results(b)
    decided = [all(d in dec for d in range(70) if d not in sp["byzantine"]) for sp, (_e, dec, _n) in zip(b.specs, res.values())]
    assert any(decided) and not all(decided), decided                      # f equivocators leave n - f deliveries: a stall
    assert not decided[1]


def test_both_waves_and_both_kernels_widths():
    by = LP.by_name()
    byz = by["lp-256-ref-c3"].specs[0]["byzantine"]
    assert {x // 64 for x in byz} == {0, 1, 2} and {x & 1 for x in byz} == {0, 1}
    assert by["lp-256-ref-c3"].specs[0]["delay_model"] == LP.CONST and by["lp-256-ref-c3"].specs[0]["dconst"] == 3
    sp = by["lp-256-ref-loaded"].specs[0]
    assert sp["n"] == 256 and {x // 64 for x in sp["byzantine"]} == {0, 1, 2, 3} and by["lp-256-ref-loaded"].proposals == "loaded"
    assert {a["value"] for s in by["lp-256-ref-loaded"].specs for a in s["actions"] if a["kind"] == "propose"} == {1, 2, 3}
    assert by["lp-128-beb-d4"].specs[0]["mode"] == "beb_consensus" and by["lp-128-beb-d4"].specs[0]["n"] == 100
    q16 = by["lp-128-ref-q16"]
    assert q16.q * q16.nv == 16 and q16.wide_windows and q16.specs[0]["round_cap"] == 4
    nv4 = by["lp-128-ref-nv4"]
    assert (nv4.q, nv4.nv) == (2, 4)
    # an instance that decides in most batches
    for name in ("lp-256-ref-c3", "lp-256-ref-loaded", "lp-128-beb-d4", "lp-128-ref-q16", "lp-128-ref-nv4"):
        res = _results(by[name])
        assert any(exp["status"] == "done" for (exp, _dec, _n) in res.values()), name


def test_small_f_committees_deliver_equivocated_keys():
    """n = 65: at f = 1 with an odd Byzantine replica the even half plus the origin's own ECHO is the quorum (34), so
    variant 0 can deliver, at receivers that got the SEND and at receivers that did not; both variants of one origin
    deliver at one replica only at f = 0 with an even Byzantine replica (33 + 33)."""
    by = LP.by_name()
    got = {}
    for name in LP.SMALL_F:
        b = by[name]
        assert b.specs[0]["n"] == 65 and len(b.specs[0]["byzantine"]) == 1
        got[name] = [LP.equivocated_deliveries(sp, exp) for sp, (exp, _dec, _n) in zip(b.specs, _results(b).values())]
        print(name, got[name])
    assert by["lp-128-f1-slow"].specs[0]["f"] == 1 and by["lp-128-f1-slow"].specs[0]["byzantine"][0] & 1
    assert by["lp-128-f0-slow"].specs[0]["f"] == 0 and not by["lp-128-f0-slow"].specs[0]["byzantine"][0] & 1
    f1 = got["lp-128-f1-const"] + got["lp-128-f1-slow"]
    assert any(c > 0 for (c, _b) in f1), f1                                 # an honest replica delivers an equivocated key
    assert not any(bb for (_c, bb) in f1)                                   # ... never both variants at f >= 1
    # ... at replicas of the out-class too: 64 honest replicas, 33 of them even
    assert any(c > 33 for (c, _b) in f1), f1
    f0 = got["lp-128-f0-const"] + got["lp-128-f0-slow"]
    assert any(bb > 0 for (_c, bb) in f0), f0                               # one replica delivers both variants


def test_oracle_time_budget():
    _results(LP.batches()[0])
    print("oracle runs of the module: %.1f s" % _TOOK[0])
    assert _TOOK[0] < ORACLE_SECONDS, _TOOK[0]


def test_flag_abi_and_carve():
    import inspect

    from byzantinerandomizedconsensus_amd import _lib as L
    from byzantinerandomizedconsensus_amd.engine import Engine
    from tests import wide_life_workloads as WL
    assert L.FLAG_LIFE_PATTERN == LP.FLAG == 32 and L.FLAG_WIDE_LIFE == LP.FLAG_LIFE == 16 and L.ABI_VERSION >= 12
    assert inspect.signature(Engine.__init__).parameters["life_pattern"].default is False
    # the carve without the pattern term is the one tests/test_gpu_wide_life.py pins
    for npad in (128, 256):
        for q, nv in ((8, 1), (4, 2), (2, 4), (8, 2), (16, 2), (32, 1)):
            base = WL.lds_bytes_life_wide(npad, q, nv, False)
            assert LP.lds_bytes_life_wide(npad, q, nv, False) == base
            nkw = npad * q * nv // 64
            assert LP.lds_bytes_life_wide(npad, q, nv, False, True) == base + 16 * nkw + 64 + 4 * npad
    assert LP.lds_bytes_life_wide(256, 32, 1, False) == 92736
    assert LP.lds_bytes_life_wide(128, 4, 2, False, True) == 16512
    assert LP.lds_bytes_life_wide(256, 16, 2, False, True) == 91776 <= 160 * 1024


def test_class_api_does_not_set_the_flag():
    import inspect

    from byzantinerandomizedconsensus_amd import network
    assert "life_pattern" not in inspect.getsource(network)
