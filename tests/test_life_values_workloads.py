"""Preconditions of tests/test_gpu_life_values.py, on the C oracle alone (no GPU): every batch of
tests/life_values_workloads.py decides ids >= 4, depends on the third bit of its value ids, ends done inside its key
window and runs on the oracle in seconds; the eight-id batch fills a replica's value table.  Plus the host's side of the
interface: the LDS carve with the value plane (the C formula itself, compiled here), brc_create's refusals, which need
no device, the flag bit and the ABI version."""
import concurrent.futures
import ctypes
import os
import subprocess

import pytest

from oracle import oracle
from tests import golden_io
from tests import life_values_workloads as LV
from tests import wide_values_workloads as V
from tests import wide_window_workloads as W
from tests.golden import specs as S

from byzantinerandomizedconsensus_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [b.name for b in LV.batches()]
ORACLE_NAMES = [b.name for b in LV.batches() if b.oracle]
# n = 65, f = 0 with an equivocator cannot decide, whatever is proposed: a phase ends after n - f + 1 = 66 deliveries.
# Phase 1 has exactly 66 keys (64 honest proposals and both pattern keys, which deliver everywhere: 32 honest ECHOs of
# a parity plus the origin's own are the quorum of 33), so nothing is left over; phase 2 has the 64 honest keys only.
# With b equivocators phase 2 sees n - b + (b - 1) = n - 1 deliveries, for every b >= 1.  The batch is kept for what it
# alone has -- pattern keys that deliver, so a window holds ids 1 and 2 beside ids above 3 -- and is held to that
# (test_f0_pattern_batch_fills_phase_one_and_stalls) instead of to "done", "decides an id >= 4" and the fold check, whose
# observable (a decision) it cannot produce.
STALLS = ("lv-128-pat-f0",)
DECIDING = [n for n in ORACLE_NAMES if n not in STALLS]
RUN_SECONDS = 10.0


def test_table_covers_the_shapes():
    by = LV.by_name()
    got = {(b.specs[0]["n"], b.specs[0]["mode"], b.specs[0]["delay_model"], b.specs[0]["dmax"], b.specs[0]["round_cap"],
            b.q, b.nv, b.wide_windows, b.pattern, b.load_masks) for b in LV.batches()}
    assert got == {(65, "consensus", LV.SLOW, 8, 1, 8, 1, False, False, False),
                   (70, "consensus", LV.SLOW, 8, 1, 8, 1, False, False, False),
                   (128, "consensus", LV.SLOW, 4, 1, 8, 1, False, False, False),
                   (130, "consensus", LV.CONST, 3, 1, 8, 1, False, False, False),
                   (128, "beb_consensus", LV.SLOW, 8, 1, 8, 1, False, False, False),
                   (70, "consensus", LV.SLOW, 4, 3, 8, 1, False, False, False),
                   (70, "consensus", LV.SLOW, 8, 5, 16, 1, True, False, False),
                   (70, "consensus", LV.SLOW, 8, 1, 8, 1, False, False, True),
                   (70, "consensus", LV.SLOW, 8, 1, 4, 2, False, True, False),
                   (65, "consensus", LV.SLOW, 4, 1, 4, 2, False, True, False),
                   (256, "consensus", LV.SLOW, 8, 1, 8, 1, False, False, False)}
    for b in LV.batches():
        specs, sp0 = b.specs, b.specs[0]
        n = sp0["n"]
        assert len(specs) == (2 if n == 256 else LV.COUNT) and [sp["g"] for sp in specs] == [777 + i for i in range(len(specs))]
        assert all(sp["values"] == S.VALUES8 and 5 <= sp["f"] <= 10 or b.name == "lv-128-pat-f0" for sp in specs)
        assert b.q * b.nv <= (32 if b.wide_windows else 8) and sp0["dmax"] <= 8
        assert b.oracle == (n <= 130)
        for sp in specs:
            byz = sp["byzantine"]
            extra = [a for a in sp["actions"] if a["kind"] != "propose"]
            assert extra == (S.equivocation_actions(n, byz, nv=b.nv) if b.pattern else [])        # nothing to inject
            props = [a for a in sp["actions"] if a["kind"] == "propose"]
            assert all(a["t"] == 0 for a in props) and sorted(a["node"] for a in props) == [d for d in range(n) if d not in byz]
            assert max(a["value"] for a in props) >= 4
        if not b.load_masks:
            assert all(sp["byzantine"] == sp0["byzantine"] for sp in specs)
    assert by["lv-128-n65-maj"].specs[0]["byzantine"] == [5, 33]               # replica 64, the second wave's one, is honest
    assert len({tuple(sp["byzantine"]) for sp in by["lv-128-masks"].specs}) == 3
    # the pattern batches: honest majorities of id 5 or more next to the pattern's ids 1 and 2
    for name in ("lv-128-pat-n70", "lv-128-pat-f0"):
        for sp in by[name].specs:
            props = [a["value"] for a in sp["actions"] if a["kind"] == "propose"]
            assert max(props.count(v) for v in (5, 6, 7)) * 2 > sp["n"] + sp["f"]
            assert {a["value"] for a in sp["actions"] if a["kind"] == "byz_key"} == {1, 2}
    assert by["lv-128-pat-f0"].specs[0]["f"] == 0 and by["lv-128-pat-f0"].specs[0]["byzantine"] == [32]
    assert {LV.EIGHT, LV.CAP3, LV.RESET, LV.OTHER, LV.BIG, LV.NO_ORACLE} | set(LV.BINARY) | set(LV.SIBLING.values()) <= set(NAMES)
    assert by[LV.SIBLING[LV.NO_ORACLE]].specs[0]["n"] == 130 and by[LV.NO_ORACLE].specs[0]["n"] == 256


@pytest.mark.parametrize("name", DECIDING)
def test_batch_decides_high_ids_inside_its_window(name):
    b = LV.by_name()[name]
    res = LV.oracle_results(b)
    secs = LV.oracle_seconds(b)
    print(name, [exp["status"] for (exp, _d, _n) in res.values()], [exp["t_stop"] for (exp, _d, _n) in res.values()],
          ["%.1f s" % s for s in secs])
    assert max(secs) < RUN_SECONDS, secs
    # done, and no overflow: the send log needs no more than the key window
    assert all(exp["status"] == "done" for (exp, _d, _n) in res.values())
    assert all(exp["t_stop"] < b.specs[0]["step_cap"] for (exp, _d, _n) in res.values())
    need = [W.needs(exp, b.specs[0]["dmax"]) for (exp, _d, _n) in res.values()]
    assert max(need) <= b.q, need
    # at least two of three instances have an honest replica decide an id >= 4
    high = sum(any(v >= 4 for ds in dec.values() for (_r, _t, v) in ds) for (_e, dec, _n) in res.values())
    assert high >= 2, (name, high)
    if b.specs[0]["round_cap"] > 1:
        # ... in a later round as well: the decided id went back through the send queue and the slot value
        late = sum(any(v >= 4 and r >= 2 for ds in dec.values() for (r, _t, v) in ds) for (_e, dec, _n) in res.values())
        assert late >= 2, (name, late)


@pytest.mark.parametrize("name", DECIDING)
def test_the_third_bit_matters(name):
    """Run with every value id folded to two bits, the oracle's result changes for at least two of three instances."""
    b = LV.by_name()[name]
    res = LV.oracle_results(b)
    with concurrent.futures.ThreadPoolExecutor(len(b.specs)) as ex:
        lows = list(ex.map(lambda sp: I_run(LV.fold(sp)), b.specs))
    changed = 0
    for i, low in enumerate(lows):
        exp = res[i][0]
        changed += any(low[k] != exp[k] for k in LV.CKEYS) or low["events"] != exp["events"]
    assert changed >= 2, (name, changed)


def test_f0_pattern_batch_fills_phase_one_and_stalls():
    """Every honest replica delivers the 64 honest phase-0 keys and both keys of the equivocator -- ids 1 and 2 beside a
    majority of an id above 4 and a tail of every other id -- ends phase 1 at the 66th delivery, SENDs its phase-1 key and
    stalls there: QUIESCENT, inside the window, in under 10 s."""
    (name,) = STALLS
    b = LV.by_name()[name]
    res = LV.oracle_results(b)
    assert max(LV.oracle_seconds(b)) < RUN_SECONDS
    for sp, (exp, dec, _n) in zip(b.specs, res.values()):
        n, nv, (byz,) = sp["n"], sp["nv"], sp["byzantine"]
        hon = [d for d in range(n) if d != byz]
        assert exp["status"] == "quiescent" and not dec and W.needs(exp, sp["dmax"]) <= b.q
        got = {}
        for _t, node, kp, s in exp["events"]["deliver"]:
            got.setdefault(node, []).append((kp, s))
        for d in hon:
            assert sorted(got[d][:66]) == sorted([(o * nv, 0) for o in hon] + [(byz * nv, 0), (byz * nv + 1, 0)]), d
            assert sorted(got[d][66:]) == [(o * nv, 1) for o in hon], d
        sent = sorted(src for _t, src, typ, kp, s in exp["events"]["send"] if typ == S.SEND and s == 1)
        assert sent == hon
        assert {a["value"] for a in sp["actions"] if a["kind"] == "propose"} == set(range(8))


def I_run(sp):
    low = oracle.run(sp)
    low["events"] = golden_io.canonical_events(low["events"])
    return low


def test_eight_id_batch_fills_a_value_table():
    """Some honest replica inserts eight ids in one window, id 0 among them (the window replayed from the DELIVER order,
    as tests/test_wide_values_workloads.py does)."""
    b = LV.by_name()[LV.EIGHT]
    for i, sp in enumerate(b.specs):
        assert {a["value"] for a in sp["actions"] if a["kind"] == "propose"} == set(range(8))
        exp = oracle.run(sp)
        decides, widest, _above = V.replay(sp, exp)
        want = sorted([t, d, r, S.VALUES8.index(v)] for t, d, r, v in exp["events"]["decide"])
        assert sorted(decides) == want, i                  # the replay is the oracle's consensus
        assert widest == 8, (i, widest)


CARVE = r"""
#include <stdio.h>
#include <initializer_list>
#include "byzantinerandomizedconsensus_amd/csrc/brc_layout.h"
int main() {
    for (int npad : {128, 256})
        for (unsigned q : {2u, 4u, 8u, 16u, 32u})
            for (unsigned nv : {1u, 2u, 4u})
                for (int pat = 0; pat < 2; ++pat) {
                    const unsigned NK = npad * q * nv, nkw = NK / 64;
                    printf("%d %u %u %d %u %u %u\n", npad, q, nv, pat, brc::lds_bytes_life_wide(npad, NK, nkw, false, q, pat),
                           brc::lds_bytes_life_wide(npad, NK, nkw, false, q, pat, false),
                           brc::lds_bytes_life_wide(npad, NK, nkw, false, q, pat, true));
                }
    return 0;
}
"""


def test_carve_with_the_value_plane(tmp_path):
    """csrc/brc_layout.h lds_bytes_life_wide itself: with v8 the old value + NK for every accepted (NPAD, window,
    pattern); without it the old value (the mirrors tests/test_gpu_wide_life.py and tests/test_life_pattern_workloads.py
    pin)."""
    from tests import life_pattern_workloads as LP
    from tests import wide_life_workloads as WL
    src, exe = str(tmp_path / "carve.cpp"), str(tmp_path / "carve")
    open(src, "w").write(CARVE)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", ROOT, src, "-o", exe])
    rows = [tuple(int(x) for x in line.split()) for line in subprocess.check_output([exe]).decode().splitlines()]
    seen = 0
    for npad, q, nv, pat, dflt, off, on in rows:
        if q * nv > 32 or (pat and nv == 1):
            continue
        seen += 1
        old = LP.lds_bytes_life_wide(npad, q, nv, False, bool(pat))
        assert dflt == off == old == LV.lds_bytes_life_wide(npad, q, nv, False, bool(pat)), (npad, q, nv, pat)
        if not pat:
            assert old == WL.lds_bytes_life_wide(npad, q, nv, False)
        assert on == old + npad * q * nv == LV.lds_bytes_life_wide(npad, q, nv, False, bool(pat), True), (npad, q, nv, pat)
        assert on <= 160 * 1024
    assert seen >= 30
    assert LV.lds_bytes_life_wide(256, 32, 1, False) == 92736
    # the largest carve: NPAD 256 with 8,192 key slots
    assert max(on for npad, q, nv, pat, _d, _o, on in rows if q * nv <= 32 and not (pat and nv == 1)) == \
        LV.lds_bytes_life_wide(256, 32, 1, False, False, True) == 92736 + 8192
    assert LV.lds_bytes_life_wide(256, 16, 2, False, True, True) == 91776 + 8192


def _create(**kw):
    """(rc, reason) of brc_create; an engine that was created (a device is present) is destroyed."""
    lib = L.load()
    base = dict(n=70, f=5, instances=1, protocol=L.PROTO_CONSENSUS, seed=1, delay_model=L.DELAY_SLOWSET, delay_max=8,
                delay_const=1, round_cap=1, step_cap=400, key_window=8, variants=1, proposals=L.PROPOSALS_PHILOX,
                mode=L.MODE_REFERENCE)
    base.update(kw)
    h = ctypes.c_void_p()
    rc = lib.brc_create(ctypes.byref(L.Config(**base)), ctypes.byref(h))
    why = (lib.brc_last_error(None) or b"").decode()
    if rc == L.OK:
        lib.brc_destroy(h)
    else:
        assert not h.value
    return rc, why


def test_flag_values_and_abi():
    import inspect

    from byzantinerandomizedconsensus_amd.engine import Engine
    assert L.FLAG_LIFE_VALUES == LV.FLAG == 128 and L.FLAG_WIDE_LIFE == LV.FLAG_LIFE == 16
    assert L.FLAG_LIFE_PATTERN == LV.FLAG_PATTERN == 32
    assert L.ABI_VERSION == 13 and L.load().brc_abi_version() == 13
    assert inspect.signature(Engine.__init__).parameters["life_values"].default is False


def test_create_refusals_need_no_device():
    life, val = L.FLAG_WIDE_LIFE, L.FLAG_LIFE_VALUES

    def refused(words, **kw):
        rc, why = _create(**kw)
        assert rc == L.E_INVALID and all(w in why for w in words), (kw, rc, why)

    refused(("BRC_FLAG_LIFE_VALUES", "needs BRC_FLAG_WIDE_LIFE"), flags=val)
    refused(("BRC_FLAG_LIFE_VALUES", "needs BRC_FLAG_WIDE_LIFE"), flags=val | L.FLAG_WIDE_VALUES)
    refused(("BRC_FLAG_LIFE_VALUES", "n > 64"), flags=life | val, n=64)
    refused(("BRC_FLAG_LIFE_VALUES", "n > 64"), flags=life | val, n=33)
    refused(("BRC_FLAG_LIFE_VALUES", "sender peers"), flags=life | val, peer_mode=L.PEER_CONNECTION)
    refused(("BRC_FLAG_LIFE_VALUES", "BRC_MODE_SPEC"), flags=life | val, mode=L.MODE_SPEC)
    # with the step kernel's record / 3-bit flags: refused as BRC_FLAG_WIDE_LIFE refuses them
    old = "BRC_FLAG_WIDE_LIFE: not with BRC_FLAG_WIDE_RECORDS / BRC_FLAG_WIDE_VALUES (flags), which select the step kernel's " \
          "record and 3-bit forms"
    for extra in (L.FLAG_WIDE_RECORDS, L.FLAG_WIDE_VALUES):
        assert _create(flags=life | val | extra) == (L.E_INVALID, old)
        assert _create(flags=life | extra) == (L.E_INVALID, old)
    # bit 64 stays unknown
    for flags in (64, 64 | life, 64 | life | val):
        assert _create(flags=flags) == (L.E_INVALID, "invalid configuration (see include/brc.h field ranges)")
    # everything BRC_FLAG_WIDE_LIFE requires still holds under the new flag
    refused(("BRC_FLAG_WIDE_LIFE", "delay_model"), flags=life | val, delay_model=L.DELAY_UNIFORM, delay_max=4)
    refused(("BRC_FLAG_WIDE_LIFE", "event_capacity"), flags=life | val, event_capacity=64)
    refused(("field ranges",), flags=life | val, key_window=16)
    # what the flag takes (no BRC_E_INVALID: BRC_OK with a device, BRC_E_HIP without)
    for kw in (dict(), dict(mode=L.MODE_BEB), dict(n=256, f=10), dict(delay_model=L.DELAY_CONST, delay_const=3),
               dict(flags=life | val | L.FLAG_WIDE_WINDOWS, key_window=16),
               dict(flags=life | val | L.FLAG_WIDE_WINDOWS, n=130, key_window=32),
               dict(flags=life | val | L.FLAG_LIFE_PATTERN, byz_pattern=L.BYZ_EQUIVOCATE, variants=2, key_window=4),
               dict(flags=life | val | L.FLAG_LIFE_PATTERN | L.FLAG_WIDE_WINDOWS, n=256, byz_pattern=L.BYZ_EQUIVOCATE, variants=2,
                    key_window=16)):
        rc, why = _create(**dict(dict(flags=life | val), **kw))
        assert rc != L.E_INVALID, (kw, why)


def test_class_api_does_not_set_the_flag():
    import inspect

    from byzantinerandomizedconsensus_amd import network
    assert "life_values" not in inspect.getsource(network) and "LIFE_VALUES" not in inspect.getsource(network)
