"""brc_inject's decisions (csrc/brc_inject.h: the staging function and the book of injections, free of HIP) on scripted
batches with synthetic device state.

tests/inject_dump.cpp is built with the host C++ compiler against brc_inject.h alone -- that it compiles is the proof that
the header needs no HIP header -- under the address and undefined-behaviour sanitizers, and run as a program of its own on
the scripts of tests/inject_workloads.py.  Its dump is held to: every refusal text of the header; the all-or-nothing
rule; the links a Byzantine replica's ECHO / READY has left, at n = 7 and n = 130; the record tables (merge, no merge,
16 / 17, pruning) decoded from their packed words; repeated SENDs; and the generation book against the restatement and
the record schedules of tests/gen_tag_workloads.py.  tests/test_gpu_inject_texts.py holds the library to the same texts."""
import re

import pytest

from byzantinerandomizedconsensus_amd import _lib as L
from tests import gen_tag_workloads as W
from tests import inject_workloads as J

S, K, M, P = L.INJ_SEND, L.INJ_KEY, L.INJ_MSG, L.INJ_PROPOSE
rec, batch, full = J.rec, J.batch, J.full


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return J.build_dump(tmp_path_factory.mktemp("inject"))


def dump(exe, scenarios):
    """scenarios: [(name, engine, command lines)] -> {name: ops}"""
    lines = []
    for name, cfg, cmds in scenarios:
        lines += [J.engine_line(name, cfg)] + list(cmds)
    out = J.run_dump(exe, lines)
    assert all(out[name]["E"].get("rc") == 0 for name, _, _ in scenarios), out
    return {name: out[name]["ops"] for name, _, _ in scenarios}


def header_literals():
    """The string literals of brc_inject.h, adjacent ones joined as the compiler joins them, comments dropped."""
    src = re.sub(r"//[^\n]*", "", open(J.INJECT_H).read())
    joined = re.findall(r'"(?:[^"\\\n]|\\.)*"(?:\s*"(?:[^"\\\n]|\\.)*")*', src)
    return ["".join(re.findall(r'"((?:[^"\\\n]|\\.)*)"', j)) for j in joined]


def keys_script(cfg, k, node=6):
    return ["quiet 1"] + batch([rec(1 + j, K, node, kp=node) for j in range(k)]) + ["run 0 0"]


# no literal of the header is unreachable (tests/test_plan.py has one, and lists it by name)
UNREACHABLE = ()


def test_every_refusal_text_is_produced(exe):
    out = J.run_dump(exe, J.refusal_script())
    whys = []
    for name, _cfg, _state, recs, rc, text in J.REFUSALS:
        op, = out["refuse/" + name]["ops"]
        assert op["rc"] == rc and op["why"].startswith(text), (name, op)
        whys.append(op["why"])
        # the device state is read once, at the first record past its static checks: not at all when the first record
        # fails them, and never for an empty batch
        assert op["fetches"] == (1 if name in ("time-before", "life-done", "stopped") or len(recs) > 1 else 0), (name, op)
    got = dump(exe, [("budget", "p7-q2", keys_script("p7-q2", 8188)), ("empty", "p7", ["inject"])])
    whys.append(got["budget"][-1]["why"])
    assert got["empty"][0]["rc"] == 0 and got["empty"][0]["fetches"] == 0 and got["empty"][0]["staged"] == 0
    texts = [t for t in header_literals() if len(t) > 16]
    assert len(texts) == 20 and len(set(texts)) == 20, texts
    for t in texts:
        assert any(t in w for w in whys) != (t in UNREACHABLE), t


def valid_batch(cfg):
    c = J.ENGINES[cfg]
    n, b = c["n"], c["n"] - 1
    out = [rec(0, S, 0, n=n), rec(1, K, b, kp=b), rec(2, M, b, type=L.ECHO, n=n)]
    if not (cfg.startswith("lean") or cfg.startswith("w70") or cfg.startswith("c7")):
        out += [rec(3, M, b, type=L.READY, dst=5), rec(3, M, b, type=L.READY, n=n), rec(4, S, 1, n=n), rec(5, S, 1, dst=3)]
    return out


def test_a_refused_batch_leaves_nothing_behind(exe):
    """After each refused batch the same valid batch gives the dump it gives on a book that never saw the refused one."""
    scen = []
    for name, cfg, state, recs, _rc, _text in J.REFUSALS:
        if name in ("pattern", "life-only"):        # the engine takes no batch at all
            continue
        undo = ["item 0 0 0", "inst 0 0", "lifedone 0"] if state else []
        scen.append(("after/" + name, cfg, state + batch(recs) + undo + batch(valid_batch(cfg))))
        scen.append(("clean/" + name, cfg, batch(valid_batch(cfg))))
    # ... and a refusal by the 17th record, after records that changed links, SENDs and tables of their own
    for cfg in ("p7", "wr130"):
        bad = valid_batch(cfg) + J.extra_sends(17, 9)
        scen.append(("after/17/" + cfg, cfg, batch(bad) + batch(valid_batch(cfg))))
        scen.append(("clean/17/" + cfg, cfg, batch(valid_batch(cfg))))
    got = dump(exe, scen)
    for name, _, _ in scen:
        if name.startswith("after/"):
            refused, ok = got[name]
            assert refused["rc"] != 0 and ok["rc"] == 0 and ok["staged"] >= 3, (name, refused, ok)
            assert ok == got["clean/" + name[6:]][0], name


@pytest.mark.parametrize("cfg", ("p7", "wr130", "gen40", "wr70-cons"))
def test_links_of_a_byzantine_echo(exe, cfg):
    """A subset ECHO, then a broadcast of the same (node, type, key): a record over exactly the complement; a third: a
    record over no link; `restricted` bit 1 on the first only.  At n = 130 the subset uses the second and third
    destination words.  In one batch and over three calls alike."""
    n, wide = J.ENGINES[cfg]["n"], J.ENGINES[cfg]["n"] > 64
    b = n - 1
    sub = 0b10 | (1 << (n - 2)) | ((1 << 70) if n > 70 else 0)
    seq = [rec(1, M, b, kp=b, type=L.ECHO, dst=sub), rec(2, M, b, kp=b, type=L.ECHO, n=n), rec(3, M, b, kp=b, type=L.ECHO, n=n)]
    other = [rec(1, M, b, kp=b, type=L.READY, n=n), rec(2, M, b, kp=b, type=L.READY, dst=sub)]    # broadcast first
    got = dump(exe, [("one", cfg, batch(seq)), ("three", cfg, [ln for x in seq for ln in batch([x])]),
                     ("cell", cfg, batch(other))])
    one = got["one"][0]
    js = one["J"]
    assert [j["dst"] for j in js] == [sub, full(n) & ~sub, 0] and [j["restricted"] for j in js] == [3, 1, 1], js
    if n == 130:
        assert (sub >> 64) & (2 ** 64 - 1) and sub >> 128
    assert [j for op in got["three"] for j in op["J"]] == js
    tab, = one["T"]
    recs = J.decode_table(tab, wide)
    assert [(r["t"], r["type"], r["dst"]) for r in recs] == [(1, L.ECHO, sub), (2, L.ECHO, full(n) & ~sub)]   # none for the third
    assert all(r["node"] == b for r in recs) if wide else all(r["smask"] == 1 << b and r["seg"] == 0 for r in recs)
    assert J.decode_table(got["three"][-2]["T"][0], wide) == recs and got["three"][-1]["T"] == []
    assert one["K"]["links"] == 1 and got["three"][-1]["K"] == one["K"]
    # a broadcast with no record before it keeps the cell path and books its links: the subset after it has none left
    c0, c1 = got["cell"][0]["J"]
    assert (c0["restricted"], c0["dst"], c1["restricted"], c1["dst"]) == (0, full(n), 1, 0) and got["cell"][0]["T"] == []


def test_record_tables(exe):
    n7, n130 = 7, 130
    two = lambda n, **kw: [rec(1, M, n - 2, kp=3, type=L.ECHO, dst=5, **kw), rec(1, M, n - 1, kp=3, type=L.ECHO, dst=5, **kw)]
    first = lambda n: [rec(0, S, 0, n=n)]
    xs = lambda n, k, t0=1, j0=0: J.extra_sends(k, t0, j0)
    scen = [("merge7", "p7", batch(two(n7))), ("merge130", "wr130", batch(two(n130))),
            ("seg7", "p7", batch(two(n7) + two(n7, instance=1))),
            ("b16-7", "p7", batch(first(n7) + xs(n7, 16)) + batch(xs(n7, 1, 40, 16))),
            ("b16-130", "wr130", batch(first(n130) + xs(n130, 16)) + batch(xs(n130, 1, 40, 16))),
            ("empty7", "p7", batch(first(n7) + [rec(1, S, 1, dst=0)])), ("empty70", "wr70", batch(first(70) + [rec(1, S, 1, dst=0)]))]
    # pruning at t + delay_max < item.t (delay_max = 4): a record at t = 1 leaves when the item stands at 6, stays at 5,
    # and stays on an item that is not initialised
    for tag, item in (("at6", "item 0 6 1"), ("at5", "item 0 5 1"), ("uninit", "item 0 6 0")):
        for cfg, n in (("p7", n7), ("wr130", n130)):
            scen.append(("prune-%s-%s" % (tag, cfg), cfg, batch(first(n) + xs(n, 1)) + [item] + batch(xs(n, 1, 6, 1)) + batch([rec(7, K, 1)])))
    got = dump(exe, scen)
    m, = J.decode_table(got["merge7"][0]["T"][0], False)
    assert m == dict(slot=3 * 4, t=1, seg=0, type=L.ECHO, smask=0b1100000, dst=5)
    w = J.decode_table(got["merge130"][0]["T"][0], True)
    assert [(r["node"], r["dst"], r["type"], r["slot"]) for r in w] == [(128, 5, L.ECHO, 12), (129, 5, L.ECHO, 12)]
    assert [r["seg"] for r in J.decode_table(got["seg7"][0]["T"][0], False)] == [0, 1]      # one item, two instances
    for name, wide, where in (("b16-7", False, "item"), ("b16-130", True, "instance")):
        ok, over = got[name]
        assert ok["rc"] == 0 and ok["T"][0]["count"] == 16 and ok["K"]["recs"] == 16
        assert all(r["type"] == 0 for r in J.decode_table(ok["T"][0], wide))
        assert over["rc"] == L.E_UNSUPPORTED and over["why"].endswith("records in flight in one " + where)
    # an extra SEND with no link: recorded on the narrow kernels, not on the wide ones (staged on both)
    assert got["empty7"][0]["T"][0]["count"] == 1 and got["empty7"][0]["J"][1]["type"] == 2
    assert got["empty70"][0]["T"] == [] and got["empty70"][0]["J"][1]["type"] == 2
    for cfg, wide in (("p7", False), ("wr130", True)):
        for tag, ts in (("at6", [6]), ("at5", [1, 6]), ("uninit", [1, 6])):
            ops = got["prune-%s-%s" % (tag, cfg)]
            assert [r["t"] for r in J.decode_table(ops[1]["T"][0], wide)] == ts, (cfg, tag)
            assert ops[1]["K"]["recs"] == len(ts)
            assert ops[2]["rc"] == 0 and ops[2]["T"] == []       # a batch that adds no record rewrites no table


def test_repeated_sends(exe):
    """`type` of a staged SEND: 0 the key's first, 2 a key SENT before by another node, 3 this node's repeat.  (1 cannot
    occur: a node's repeat is of a key SENT before, and the kernels that take no second SEND refuse it.)"""
    for cfg in ("p7", "c7", "wr130"):
        n = J.ENGINES[cfg]["n"]
        seq = [rec(0, S, 0, n=n), rec(1, S, 1, dst=0b0110), rec(2, S, 1, dst=0b1100), rec(3, S, 1, dst=0b1100), rec(3, S, 2, n=n, s=1)]
        got = dump(exe, [("a", cfg, batch(seq) + ["inst 0 %d" % L.DONE] + batch(seq[3:4]))])["a"]
        js = got[0]["J"]
        if cfg == "c7":       # connection peers carry every copy: nothing dropped, nothing unstaged
            assert [(j["type"], j["dst"]) for j in js] == [(0, full(n)), (2, 0b0110), (3, 0b1100), (3, 0b1100), (0, full(n))]
        else:                 # sender peers: the node's used links are dropped; with none left the repeat is not staged
            assert [(j["type"], j["dst"]) for j in js] == [(0, full(n)), (2, 0b0110), (3, 0b1000), (0, full(n))]
        assert got[0]["K"]["sends"] == 5                       # ... yet counted
        assert all(j["restricted"] == (j["dst"] != full(n)) for j in js)
        # a stopped instance still refuses it
        assert got[1]["rc"] == L.E_STATE and got[1]["why"] == "instance already stopped"
    # a quiescent instance is re-opened, once per staged record; a dropped repeat re-opens nothing
    got = dump(exe, [("q", "p7", ["inst 1 %d" % L.QUIESCENT] + batch([rec(0, S, 0, n=7, instance=1), rec(0, S, 0, n=7, instance=1)])
                      + batch([rec(1, K, 1, instance=1)]))])["q"]
    assert got[0]["O"] == [1] and got[0]["staged"] == 1 and got[1]["O"] == []


# ---- generations -------------------------------------------------------------------------------------------------
def case_engine(case):
    fam = case.family
    return J._cfg(case.n, case.byz, peer=L.PEER_CONNECTION if fam.startswith("conn") else L.PEER_SENDER,
                  flags=L.FLAG_GENERAL_KEYS if fam == "general64" else 0, q=case.key_window,
                  mode=L.MODE_SPEC if fam == "spec" else L.MODE_BEB if fam == "beb" else L.MODE_REFERENCE, instances=case.count)


def case_records(specs, n):
    """The KEY / SEND injections of a batch (tests/gen_tag_workloads.py alloc_records, with their times)."""
    out = []
    for i, sp in enumerate(specs):
        for a in sp["actions"]:
            if a["kind"] == "byz_key":
                out.append(rec(a["t"], K, a["kp"], kp=a["kp"], s=a["s"], instance=i))
            elif a["kind"] == "brb_send":
                out.append(rec(a["t"], S, a["node"], kp=a["kp"], s=a["s"], instance=i, n=n))
            elif a["kind"] == "byz" and a["type"] == W.S.SEND:
                out.append(rec(a["t"], S, a["src"], kp=a["kp"], s=a["s"], instance=i, dst=a["dst"]))
    return out


GEN_WALKS = [(c.name, w) for c in W.cases() for w in c.walks if w != "consensus"]


def test_generation_book_follows_the_restatement(exe):
    """Every record schedule of tests/gen_tag_workloads.py but the consensus walks (whose phase indices come from the
    kernel): per epoch the book's gen_base, gen_used, clear decision and s_limit equal host_walk / gen_used / s_limit /
    excess_records, across the full clears."""
    scen, want = [], {}
    for name, walk in GEN_WALKS:
        case = W.by_name()[name]
        epochs = case.walk(walk)
        Q = case.key_window
        lines, smaxs, excess, scripts = ["quiet 1"], [], [], {}
        for tag, _off, specs in epochs:
            if tag not in scripts:
                recs = case_records(specs, case.n)
                assert len(recs) == len(W.alloc_records(specs))
                scripts[tag] = (batch(recs), max(sp["probe"][1] for sp in specs), W.excess_records(W.alloc_records(specs), False, Q))
            b, smax, x = scripts[tag]
            lines += b + ["run 0 %d" % smax, "reset"]
            smaxs.append(smax)
            excess.append(x)
        scen.append((name + "/" + walk, case_engine(case), lines))
        used = [W.gen_used(s, Q, x) for s, x in zip(smaxs, excess)]
        bases, clears = W.host_walk(used, [W.gen_used(0, Q, x) for x in excess])
        want[name + "/" + walk] = (Q, used, excess, bases, clears)
    got = dump(exe, scen)
    crossed = 0
    for key, (Q, used, excess, bases, clears) in want.items():
        ops = got[key]
        assert len(ops) == 3 * len(used)
        cleared = set()
        for e in range(len(used)):
            inj, run, rst = ops[3 * e:3 * e + 3]
            assert inj["rc"] == 0 and inj["K"]["gen_extra"] == excess[e] and inj["K"]["gen_used"] == W.gen_used(0, Q, excess[e]), (key, e)
            assert run["rc"] == 0 and run["K"]["gen_base"] == bases[e] and run["K"]["gen_used"] == used[e] == run["K"]["gen_cur"], (key, e, run)
            assert run["s_limit"] == W.s_limit(bases[e], Q, excess[e]), (key, e)
            if run["clear"]:
                cleared.add(e)
            if rst["full"]:
                cleared.add(e + 1)
            assert rst["K"]["gen_extra"] == 0 and rst["K"]["gen_smax"] == 0 and rst["K"]["sends"] == 0 and rst["K"]["recs"] == 0
        assert cleared - {len(used)} == set(clears), (key, cleared, clears)
        crossed += bool(clears)
    assert crossed >= 10


def test_generation_budget_edges(exe):
    got = dump(exe, [
        ("brb-8187", "p7-q2", keys_script("p7-q2", 8187)), ("brb-8188", "p7-q2", keys_script("p7-q2", 8188)),
        ("cons-8186", "p7-cons", keys_script("p7-cons", 8186)), ("cons-8187", "p7-cons", keys_script("p7-cons", 8187)),
        # under the consensus protocol every KEY and every first SEND counts; an extra SEND does not
        ("cons-count", "p7-cons", batch([rec(0, K, 6, kp=6), rec(1, S, 6, kp=6, n=7), rec(2, S, 5, kp=6, n=7), rec(3, S, 0, kp=6, s=4, n=7)])),
        ("brb-count", "p7", batch([rec(0, K, 6, kp=6), rec(1, S, 6, kp=6, n=7), rec(2, S, 5, kp=6, n=7), rec(3, S, 0, kp=6, s=4, n=7)])),
        # PROPOSE records of one replica are passes; Philox proposals are one more
        ("passes", "p7-cons", batch([rec(0, P, 0), rec(5, P, 0), rec(5, P, 1)]) + ["run 0 9"]),
        # the lean and the wide kernels keep no tags; nor does a run of the lifetime kernel
        ("lean", "lean40", batch([rec(j, K, 39, kp=39) for j in range(5)]) + ["run 0 7"]),
        ("wide", "wr70", batch([rec(j, K, 69, kp=69) for j in range(5)]) + ["run 0 7"]),
        ("life", "p7-cons", ["run 1 7"]),
    ])
    # the first refused KEY count of one key on a fresh engine: the 8188th under BRB (tests/test_gpu_gen_tags.py), the
    # 8187th record of one slot under the consensus protocol
    text = ("slot generation budget exhausted: call brc_reset (the records injected in this epoch can allocate one key slot "
            "more often than the %d generation tags left)" % (W.GEN_HARD - 1))
    assert W.GEN_HARD - 1 == 8188
    for ok, bad in (("brb-8187", "brb-8188"), ("cons-8186", "cons-8187")):
        assert got[ok][-1]["rc"] == 0 and got[ok][-1]["clear"] == 0, got[ok][-1]
        assert got[bad][-1]["rc"] == L.E_STATE and got[bad][-1]["why"] == text, got[bad][-1]
    assert got["brb-8187"][0]["K"]["gen_used"] == 8188 == W.gen_used(0, 2, W.excess_records([(0, 6, 0, "k")] * 8187, False, 2))
    assert got["cons-8186"][0]["K"]["gen_used"] == 8188 == W.gen_used(0, 4, W.excess_records([(0, 6, 0, "k")] * 8186, True, 4))
    recs = [(0, 6, 0, "k"), (0, 6, 0, "s"), (0, 6, 4, "s")]            # the extra SEND (the third record) is no allocation
    assert got["cons-count"][0]["K"]["gen_extra"] == W.excess_records(recs, True, 4) == 3
    assert got["brb-count"][0]["K"]["gen_extra"] == W.excess_records(recs, False, 4) == 1
    assert [j["type"] for j in got["cons-count"][0]["J"]] == [0, 0, 2, 0]
    run = got["passes"][1]
    assert run["K"]["gen_props"] == 2 and run["K"]["gen_used"] == W.gen_used(9, 4, 0, passes=3)
    assert run["s_limit"] == W.s_limit(0, 4, 0, passes=3)
    for name in ("lean", "wide", "life"):
        run = got[name][-1]
        assert run["rc"] == 0 and run["s_limit"] == W.S_14BIT and run["K"]["gen_cur"] == 0 and run["K"]["gen_extra"] == 0, (name, run)
