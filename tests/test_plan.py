"""The engine planner (csrc/brc_plan.h: brc_create's whole decision, free of HIP) over a fixed grid of configurations.

tests/plan_dump.cpp is built with the host C++ compiler against brc_plan.h alone -- that it compiles is the proof that
the planner needs no HIP header -- under the address and undefined-behaviour sanitizers, and run once.  Its dump is held
to: every refusal reason of the planner and every kernel family occur; the plans' invariants; and, for every
configuration planned without a device-memory figure, the answer of the library's brc_create (which loads and refuses on
a GPU-less host, tests/test_abi.py), so the planner under test is the one that ships."""
import ctypes
import os
import re
import subprocess

import pytest

from byzantinerandomizedconsensus_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_H = os.path.join(ROOT, "byzantinerandomizedconsensus_amd", "csrc", "brc_plan.h")
LDS_MAX = 160 * 1024
INT_FIELDS = ("n", "f", "protocol", "peer_mode", "instances", "delay_model", "delay_max", "delay_const", "step_cap",
              "key_window", "variants", "proposals", "byz_pattern", "event_capacity", "mode", "flags")


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """[(config fields, BRC_KERNEL or None, device memory or None, rc, reason or None, plan fields or None)]"""
    exe = str(tmp_path_factory.mktemp("plan") / "plan_dump")
    # the sanitizer runtimes linked statically: the program runs as it is, whatever else the loader brings in
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tests", "plan_dump.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=False)
    assert run.returncode == 0, run.stderr.decode()[-4000:]
    lines = run.stdout.decode().splitlines()
    assert len(lines) % 2 == 0
    out = []
    for cl, rl in zip(lines[0::2], lines[1::2]):
        assert cl.startswith("C ") and rl[:2] in ("R ", "P "), (cl, rl)
        kv = dict(t.split("=", 1) for t in cl[2:].split(" "))
        cfg = {k: int(kv[k]) for k in INT_FIELDS}
        env = None if kv["env"] == "-" else kv["env"]
        mem = None if kv["mem"] == "unknown" else int(kv["mem"])
        if rl.startswith("R "):
            m = re.fullmatch(r"R rc=(-?\d+) why=(.*)", rl)
            out.append((cfg, env, mem, int(m.group(1)), m.group(2), None))
        else:
            out.append((cfg, env, mem, L.OK, None, {k: int(v) for k, v in (t.split("=") for t in rl[2:].split(" "))}))
    return out


def planner_reason_literals():
    """The string literals of brc_plan.h, adjacent ones joined as the compiler joins them, comments dropped."""
    src = re.sub(r"//[^\n]*", "", open(PLAN_H).read())
    joined = re.findall(r'"(?:[^"\\\n]|\\.)*"(?:\s*"(?:[^"\\\n]|\\.)*")*', src)
    return ["".join(re.findall(r'"((?:[^"\\\n]|\\.)*)"', j)) for j in joined]


# brc_create's refusal "BRC_FLAG_WIDE_LIFE: key_window * variants = ... exceeds the wide key-lifetime kernel's LDS" guards
# a carve no accepted field range reaches: at NPAD = 256 and key_window * variants = 32, the largest the range check
# lets through, lds_bytes_life_wide is 16 * 128 + 32,768 + 6 * 8,192 + 576 + 32 * 256 (+ 3,136 in the pattern form)
# = 95,872 B of 163,840 (include/brc.h: "a carve above 160 KB would be refused").  It stays in the planner, in its
# place in the order of the checks; the grid cannot produce it, and the test holds that it does not.
UNREACHABLE = ("BRC_FLAG_WIDE_LIFE: key_window * variants = ", " exceeds the wide key-lifetime kernel's LDS (lds ")


def test_every_refusal_reason_is_produced(cases):
    reasons = {why for _, _, _, rc, why, _ in cases if rc != L.OK}
    assert all(rc == L.E_INVALID for _, _, _, rc, _, _ in cases if rc != L.OK)
    # the planner's texts: every literal but the BRC_KERNEL values, the closing fragments of the two reasons that
    # carry a number, and the four lifetime-only texts of brc_inject / brc_run (life_only_why: no brc_create refusal)
    texts = [t for t in planner_reason_literals() if len(t) > 16 and not t.startswith("this engine runs on")]
    # (30 reasons, and the two fragments of the reason that names f, which the planner states at both of its f >= n checks)
    assert len(texts) == 34 and len(set(texts)) == 32, texts
    for t in texts:
        hit = any(t in r for r in reasons)
        assert hit != (t in UNREACHABLE), t
    assert len([t for t in planner_reason_literals() if t.startswith("this engine runs on")]) == 4


def families(c, p):
    qnv = c["key_window"] * c["variants"]
    step, life, wide = p["step_ok"], p["life_cfg"], p["wide"]
    return {
        "npad4": step and p["npad"] == 4, "npad8": step and p["npad"] == 8, "npad16": step and p["npad"] == 16,
        "npad32": step and p["npad"] == 32,
        "lean64-regmask": step and p["compact"] and p["regmask"], "lean64-ldsmask": step and p["compact"] and not p["regmask"],
        "general64": step and p["general"] and p["kmode"] == 4, "connection64": step and p["npad"] == 64 and p["kmode"] == 3,
        "wide-wv4": step and p["wide_wv4"], "wide-3waves": step and wide and not p["wide_wv4"] and not p["wide_rec"],
        "wide-records": step and p["wide_rec"] and not p["wide_val"], "wide-values": step and p["wide_val"],
        "wide-windows": step and wide and qnv > 8,
        "life-two-class": life and not wide and not p["life_pl"], "life-per-link": life and p["life_pl"] and p["life_rw"] == 32,
        "life-dm16": life and p["life_pl"] and p["life_rw"] == 64, "life-qbig": life and not wide and c["key_window"] >= 64,
        "life-hbm-meta": life and not wide and p["has_lmeta"],
        "wide-life": life and wide and not p["life_pat"], "wide-life-pattern": life and wide and p["life_pat"],
        "life-only-by-window": not step and p["compact"] and qnv > 32,
        "life-only-by-memory": not step and p["compact"] and qnv <= 32,
        "life-only-by-connection-lds": not step and not wide and p["kmode"] == 3,
    }


def test_every_kernel_family_is_selected(cases):
    seen = set()
    names = None
    for c, _, _, rc, _, p in cases:
        if rc == L.OK:
            fam = families(c, p)
            names = set(fam)
            seen |= {k for k, v in fam.items() if v}
    assert seen == names, sorted(names - seen)


FAULT_BOUND_NS = (1, 2, 3, 4, 33, 64, 65, 256)


def test_fault_bound_ends(cases):
    """f = n and f = n + 1 are refused with a reason that names f and both numbers; f = 0 and f = n - 1 are planned on
    every kernel family tests/fault_bound_workloads.py uses at that committee size (plan_dump.cpp, part 5)."""
    narrow = {"npad4"}
    mid = {"lean64-regmask", "general64", "connection64", "life-two-class", "life-dm16"}     # (per-link delays up to 12)
    wide = {"wide-wv4", "wide-records", "wide-life", "wide-life-pattern"}
    for n in FAULT_BOUND_NS:
        for f in (n, n + 1):
            rows = [(c, rc, why) for c, _, _, rc, why, _ in cases if c["n"] == n and c["f"] == f]
            assert len(rows) >= 5, (n, f)
            for c, rc, why in rows:
                # (the pattern flag's own conditions are checked first and name their field)
                if rc == L.E_INVALID and why.startswith("BRC_FLAG_LIFE_PATTERN"):
                    continue
                assert rc == L.E_INVALID and why == "the fault bound f = %d must be below n = %d (f: 0 .. n - 1)" % (f, n), (c, why)
        for f in (0, n - 1):
            seen, modes, protocols = set(), set(), set()
            for c, _, _, rc, why, p in cases:
                if c["n"] == n and c["f"] == f and rc == L.OK:
                    seen |= {k for k, v in families(c, p).items() if v}
                    modes.add((c["mode"], c["peer_mode"], bool(p["life_cfg"])))
                    protocols.add(c["protocol"])
            want = narrow if n <= 32 else mid if n <= 64 else wide
            assert seen >= want, (n, f, sorted(want - seen))
            ref, spec, beb = L.MODE_REFERENCE, L.MODE_SPEC, L.MODE_BEB
            assert modes >= {(m, L.PEER_SENDER, False) for m in (ref, spec, beb)}, (n, f, modes)
            if n <= 64:
                assert (ref, L.PEER_CONNECTION, False) in modes, (n, f)
            if n > 32:
                assert modes >= {(m, L.PEER_SENDER, True) for m in (ref, spec, beb)}, (n, f, modes)
            assert n > 32 or protocols == {L.PROTO_BRB, L.PROTO_CONSENSUS}, (n, f)
    # no configuration with f >= n is planned anywhere in the grid
    assert not [c for c, _, _, rc, _, _ in cases if rc == L.OK and c["f"] >= c["n"]]


def test_plan_invariants(cases):
    for c, env, mem, rc, _, p in cases:
        if rc != L.OK:
            continue
        at = (c, env, mem)
        inst, q = c["instances"], c["key_window"]
        # LDS: what a launch can ask for fits a workgroup's 160 KB
        assert (p["step_ok"] and p["lds_bytes"] <= LDS_MAX) or (not p["step_ok"] and p["life_lds"] <= LDS_MAX), at
        assert not p["life_cfg"] or p["life_lds"] <= LDS_MAX, at
        assert p["step_ok"] or p["life_cfg"], at                       # an engine no kernel serves is refused
        # geometry
        assert p["npad"] >= c["n"] and (p["npad"] == 4 or p["npad"] < 2 * c["n"]), at
        assert p["wide"] == (c["n"] > 64) and p["ipw"] == (1 if p["wide"] else 64 // p["npad"]), at
        assert p["lpi"] == max(64, p["npad"]) and p["bw"] == max(1, p["npad"] // 64), at
        assert p["NK"] == p["npad"] * c["variants"] * q and p["nkw"] == (p["NK"] + 63) // 64, at
        assert p["nitems"] == (inst + p["ipw"] - 1) // p["ipw"], at
        assert not (p["compact"] and p["general"]) and (not p["regmask"] or p["compact"]), at
        assert not p["wide_val"] or p["wide_rec"], at
        assert not p["wide_rec"] or (p["wide"] and not p["wide_wv4"]), at
        assert p["nval"] == (8 if p["wide_val"] or not (p["compact"] or p["wide"]) else 4), at
        assert p["kmode"] == (3 if c["peer_mode"] == L.PEER_CONNECTION else 4 if p["general"] else c["mode"]), at
        # the buffer predicates and sizes agree with one another
        assert p["cells_up_front"] == (not p["life_cfg"]), at
        assert p["cells_n"] == p["nitems"] * p["rows"] * p["lpi"], at
        assert p["cells_bytes"] == p["cells_n"] * (4 if p["compact"] else 8), at
        assert p["keys"] == (inst * p["NK"] if p["step_ok"] else 1), at
        assert (p["meta_bytes"], p["mgen_bytes"], p["kdst_bytes"]) == (8 * p["keys"], 4 * p["keys"], 8 * p["keys"] * p["bw"]), at
        assert (p["act_bytes"] > 8) == bool(p["step_ok"]), at
        assert p["step_state_bytes"] >= p["cells_bytes"] + 20 * inst * p["NK"], at
        assert p["item_u32_bytes"] == 4 * p["nitems"] and p["items_bytes"] == 16 * p["nitems"], at
        assert p["inst_bytes"] == 16 * inst and p["istats_bytes"] == 32 * inst and p["byz_bytes"] == 8 * p["bw"] * inst, at
        assert p["cons_rec_bytes"] == 8 * p["nitems"] * p["lpi"] and p["hmask_bytes"] == p["nitems"] * p["cons_bytes"], at
        # an xsn table exactly where extra-SEND / restricted records can exist: the non-lean narrow kernels, and the
        # wide kernels with the record path
        assert p["has_xsn"] == (p["wide_rec"] or not (p["compact"] or p["wide"])), at
        rec = 8 * 5 if p["wide_rec"] else 24
        assert (p["xsend_bytes"], p["xsn_bytes"]) == ((p["nitems"] * 16 * rec, 4 * p["nitems"]) if p["has_xsn"] else (8, 8)), at
        assert p["has_dring"] == (p["life_cfg"] and p["life_pl"]), at
        assert p["dring_bytes"] == (p["nitems"] * p["life_rw"] * p["nkw"] * 512 if p["has_dring"] else 8), at
        assert p["has_lmeta"] == (p["life_cfg"] and not p["life_pl"] and q >= 32), at
        assert p["lmeta_bytes"] == (8 * p["nitems"] * p["NK"] if p["has_lmeta"] else 8), at
        assert p["has_dbits"] == (p["compact"] and c["mode"] == L.MODE_SPEC and p["step_ok"]), at
        assert p["dbits_bytes"] == (p["nitems"] * p["nkw"] * 512 if p["has_dbits"] else 8), at
        assert not (p["has_dring"] and p["has_lmeta"]), at
        # the memory test: a lean engine within the step kernel's windows is lifetime-only exactly when its step
        # state exceeds 90 % of a known device memory
        if p["compact"] and c["key_window"] * c["variants"] <= 32:
            assert p["step_ok"] == (mem is None or p["step_state_bytes"] <= mem // 10 * 9), at


def test_memory_threshold_is_exact(cases):
    """Around need == total / 10 * 9 of the lean configurations: one byte of device memory decides."""
    by_cfg = {}
    for c, env, mem, rc, why, p in cases:
        if mem is not None:
            by_cfg.setdefault((tuple(sorted(c.items())), env), []).append((mem, rc, why, p))
    assert by_cfg
    for (_, env), rows in by_cfg.items():
        need = {p["step_state_bytes"] for _, rc, _, p in rows if rc == L.OK}
        fits = [(mem, rc, p) for mem, rc, _, p in rows if rc == L.OK and p["step_ok"]]
        assert fits and len(need) == 1
        at = need.pop() // 9 * 10
        assert sorted(m for m, _, _ in fits) == [at, at + 1, at + 10, 2 ** 64 - 1]
        for mem, rc, why, p in rows:
            if mem in (0, at - 1):
                assert (rc == L.OK and not p["step_ok"] and p["life_cfg"]) or (rc == L.E_INVALID and "do not fit" in why), (env, mem)


def test_library_agrees_with_planner(cases, monkeypatch):
    """brc_create of the built library, per grid configuration without a device-memory figure: the same refusal, byte
    for byte, or no BRC_E_INVALID (BRC_OK with a device -- whose memory the small batches of the grid never approach --
    and BRC_E_HIP without)."""
    lib = L.load()
    checked = 0
    for c, env, mem, rc, why, _ in cases:
        if mem is not None:
            continue
        if env is None:
            monkeypatch.delenv("BRC_KERNEL", raising=False)
        else:
            monkeypatch.setenv("BRC_KERNEL", env)
        h = ctypes.c_void_p()
        got = lib.brc_create(ctypes.byref(L.Config(round_cap=1, seed=1, **c)), ctypes.byref(h))
        if rc != L.OK:
            assert got == L.E_INVALID and not h.value, (c, env, got)
            assert lib.brc_last_error(None) == why.encode(), (c, env)
        else:
            assert got != L.E_INVALID, (c, env, lib.brc_last_error(None))
            if got == L.OK:
                lib.brc_destroy(h)
        checked += 1
    assert checked > 1000
