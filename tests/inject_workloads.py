"""Workload table of tests/test_inject.py (CPU) and tests/test_gpu_inject_texts.py: the engines, the brc_inject batches
and the script that tests/inject_dump.cpp runs them from, its build and the parser of its dump.

An engine is a brc_config (ENGINES); a scenario is an engine under a name of its own with a list of script commands.
REFUSALS: one batch per refusal text of csrc/brc_inject.h, with the synthetic device state it needs (none for most)."""
import os
import subprocess

from byzantinerandomizedconsensus_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INJECT_H = os.path.join(ROOT, "byzantinerandomizedconsensus_amd", "csrc", "brc_inject.h")
XSEND_MAX, WREC_W, XS_TYPE_SH, WREC_NODE_SH = 16, 5, 48, 56          # csrc/brc_layout.h
STEP_CAP = 9000                                                     # inject_dump.cpp's engines


def _cfg(n, byz, peer=L.PEER_SENDER, flags=0, cons=False, mode=L.MODE_REFERENCE, q=4, nv=1, pattern=L.BYZ_NONE, instances=3):
    return dict(n=n, f=(n - 1) // 3, protocol=L.PROTO_CONSENSUS if cons else L.PROTO_BRB, mode=mode, peer_mode=peer,
                delay_model=L.DELAY_SLOWSET, delay_max=4, key_window=q, variants=nv,
                proposals=L.PROPOSALS_PHILOX if cons else L.PROPOSALS_NONE, byz_pattern=pattern, flags=flags,
                instances=instances, byz=sum(1 << b for b in byz))


# the kernel families that take injections differently, a broadcast and a consensus engine of each; the Byzantine
# replicas are the last two, so at n = 130 they sit in the third mask word
ENGINES = {}
for _name, _kw in (("p7", dict(n=7, byz=(5, 6))), ("c7", dict(n=7, byz=(5, 6), peer=L.PEER_CONNECTION)),
                   ("lean40", dict(n=40, byz=(38, 39))), ("gen40", dict(n=40, byz=(38, 39), flags=L.FLAG_GENERAL_KEYS)),
                   ("w70", dict(n=70, byz=(68, 69))), ("wr70", dict(n=70, byz=(68, 69), flags=L.FLAG_WIDE_RECORDS)),
                   ("wr130", dict(n=130, byz=(128, 129), flags=L.FLAG_WIDE_RECORDS))):
    ENGINES[_name] = _cfg(**_kw)
    ENGINES[_name + "-cons"] = _cfg(cons=True, **_kw)
ENGINES["wl70"] = _cfg(70, (68, 69), flags=L.FLAG_WIDE_LIFE, cons=True)        # lifetime-only
ENGINES["p7-spec"] = _cfg(7, (5, 6), cons=True, mode=L.MODE_SPEC)
ENGINES["p7-pattern"] = _cfg(7, (5, 6), nv=2, pattern=L.BYZ_EQUIVOCATE)
ENGINES["p7-q2"] = _cfg(7, (6,), q=2)                                          # tests/gen_tag_workloads.py p8


S, K, M, P, D = L.INJ_SEND, L.INJ_KEY, L.INJ_MSG, L.INJ_PROPOSE, L.INJ_DELIVER


def full(n):
    return (1 << n) - 1


def rec(t, kind, node, kp=0, s=0, value=1, type=0, dst=None, instance=0, n=None):
    """One brc_injection as a dict (dst: an int of up to 256 bits; None: every replica of an n-replica instance, or
    none where n is not given)."""
    return dict(t=t, kind=kind, type=type, instance=instance, node=node, kp=kp, s=s, value=value,
                dst=(full(n) if n else 0) if dst is None else dst)


def extra_sends(k, t0=1, j0=0, instance=0):
    """k SENDs of key (0, 0) after its first, each a record of its own: nodes 2 .. 6 in turn, every node over one fresh
    link a time (no link used twice, so none is dropped), at steps of their own (no merge)."""
    return [rec(t0 + j - j0, S, 2 + j % 5, dst=1 << (j // 5), instance=instance) for j in range(j0, j0 + k)]


def rec_line(x):
    d = x["dst"]
    return "r %d %d %d %d %d %d %d %d %s" % (x["t"], x["kind"], x["type"], x["instance"], x["node"], x["kp"], x["s"], x["value"],
                                            " ".join(hex((d >> (64 * w)) & (2 ** 64 - 1)) for w in range(4)))


def batch(recs):
    return [rec_line(x) for x in recs] + ["inject"]


def engine_line(scenario, cfg):
    c = ENGINES[cfg] if isinstance(cfg, str) else cfg
    b = c["byz"]
    return "engine %s %d %d %d %d %d %d %d %d %d %d %d %d %d %s %s" % (
        scenario, c["n"], c["f"], c["protocol"], c["mode"], c["peer_mode"], c["delay_model"], c["delay_max"], c["key_window"],
        c["variants"], c["proposals"], c["byz_pattern"], c["flags"], c["instances"], c.get("env") or "-",
        " ".join(hex((b >> (64 * w)) & (2 ** 64 - 1)) for w in range(4)))


def lib_config(cfg, **over):
    c = dict(ENGINES[cfg] if isinstance(cfg, str) else cfg)
    b = c.pop("byz")
    c.pop("env", None)
    c.update(over)
    return L.Config(seed=1, delay_const=1, round_cap=1, step_cap=STEP_CAP, byzantine_mask=b & (2 ** 64 - 1),
                    byzantine_mask_hi=(ctypes_u64x3(b)), **c)


def ctypes_u64x3(b):
    import ctypes
    return (ctypes.c_uint64 * 3)(*[(b >> (64 * w)) & (2 ** 64 - 1) for w in (1, 2, 3)])


def lib_injections(recs):
    import ctypes
    arr = (L.Injection * max(1, len(recs)))()
    for a, x in zip(arr, recs):
        a.t, a.kind, a.type, a.instance, a.node, a.kp, a.s, a.value = (x[k] for k in ("t", "kind", "type", "instance", "node",
                                                                                     "kp", "s", "value"))
        a.dst_mask = x["dst"] & (2 ** 64 - 1)
        for w in range(3):
            a.dst_mask_hi[w] = (x["dst"] >> (64 * (w + 1))) & (2 ** 64 - 1)
    return arr


# ---- one batch per refusal text ----------------------------------------------------------------------------------
_ok7 = rec(0, S, 0, n=7)             # a valid record ahead of the refused one: it must leave nothing behind
# (name, engine, synthetic-state commands, records, rc, text or its start); state "run": tests/test_gpu_inject_texts.py
# gets there with a three-step run instead
REFUSALS = [
    ("pattern", "p7-pattern", [], [], L.E_STATE, "explicit injections cannot be combined with byz_pattern"),
    ("life-only", "wl70", [], [rec(0, P, 0)], L.E_UNSUPPORTED, "this engine runs on the wide key-lifetime kernel only"),
    ("instance-range", "p7", [], [_ok7, rec(0, S, 0, n=7, instance=3)], L.E_INVALID, "injection out of range"),
    ("node-range", "p7", [], [rec(0, S, 7, n=7)], L.E_INVALID, "injection out of range"),
    ("t-range", "p7", [], [rec(STEP_CAP + 1, S, 0, n=7)], L.E_INVALID, "injection out of range"),
    ("value-range", "lean40", [], [rec(0, S, 0, n=40, value=4)], L.E_INVALID, "value id / phase index out of range"),
    ("value-negative", "p7", [], [rec(0, S, 0, n=7, value=-1)], L.E_INVALID, "value id / phase index out of range"),
    ("s-range", "p7", [], [rec(0, S, 0, n=7, s=0xFFFE)], L.E_INVALID, "value id / phase index out of range"),
    ("propose-brb", "p7", [], [_ok7, rec(0, P, 0)], L.E_INVALID, "PROPOSE needs the consensus protocol"),
    ("deliver-brb", "p7", [], [rec(0, D, 0)], L.E_INVALID, "DELIVER needs the consensus protocol"),
    ("deliver-spec", "p7-spec", [], [rec(0, D, 0)], L.E_UNSUPPORTED, "DELIVER: SPEC consensus counts phase-indexed keys"),
    ("deliver-host", "p7-cons", [], [rec(0, D, 0, kp=7)], L.E_INVALID, "DELIVER host out of range"),
    ("kp-range", "p7", [], [rec(0, K, 0, kp=7)], L.E_INVALID, "kp out of range"),
    ("msg-type", "p7", [], [rec(0, M, 6, type=L.SEND, n=7)], L.E_INVALID, "MSG type must be ECHO or READY"),
    ("subset-connection", "c7", [], [rec(0, M, 6, type=L.ECHO, dst=3)], L.E_UNSUPPORTED,
     "an ECHO / READY to a subset of the peers: not with connection peers"),
    ("subset-wide", "w70", [], [rec(0, M, 69, type=L.ECHO, dst=3)], L.E_UNSUPPORTED,
     "an ECHO / READY to a subset of the peers: not on the wide kernels (n > 64)"),
    ("subset-lean", "lean40", [], [rec(0, M, 39, type=L.READY, dst=3)], L.E_UNSUPPORTED,
     "an ECHO / READY to a subset of the peers: not on the lean kernels"),
    ("subset-honest", "p7", [], [_ok7, rec(1, M, 6, type=L.ECHO, dst=3), rec(1, M, 0, type=L.ECHO, dst=3)], L.E_UNSUPPORTED,
     "an ECHO / READY to a subset of the peers needs a Byzantine sender"),
    ("subset-honest-wide", "wr130", [], [rec(1, M, 0, type=L.ECHO, dst=3)], L.E_UNSUPPORTED,
     "an ECHO / READY to a subset of the peers needs a Byzantine sender"),
    ("send-twice-lean", "lean40", [], [rec(0, S, 0, n=40), rec(1, S, 1, n=40)], L.E_UNSUPPORTED,
     "a key can be SENT only once on this kernel"),
    ("send-twice-wide", "w70", [], [rec(0, S, 0, n=70), rec(1, S, 0, n=70)], L.E_UNSUPPORTED,
     "a key can be SENT only once on this kernel"),
    ("kind", "p7", [], [_ok7, rec(0, 6, 0)], L.E_INVALID, "unknown injection kind"),
    ("kind-zero", "wr70", [], [rec(0, 0, 0)], L.E_INVALID, "unknown injection kind"),
    ("time-before", "p7", ["item 0 3 1"], [_ok7], L.E_STATE, "injection time is before the instance's current step"),
    ("life-done", "lean40-cons", ["lifedone 1", "inst 0 %d" % L.QUIESCENT], [rec(0, P, 0)], L.E_STATE,
     "instance finished by the key-lifetime kernel (no step state to resume): brc_reset first"),
    ("stopped", "p7", ["item 0 3 1", "inst 0 %d" % L.BADINJ], [rec(STEP_CAP, S, 0, n=7)], L.E_STATE, "instance already stopped"),
    ("table-item", "p7", [], [rec(0, S, 0, n=7)] + extra_sends(17), L.E_UNSUPPORTED,
     "more than 16 extra-SEND / restricted ECHO / READY records in flight in one item"),
    ("table-instance", "wr130", [], [rec(0, S, 0, n=130)] + extra_sends(17), L.E_UNSUPPORTED,
     "more than 16 extra-SEND / restricted ECHO / READY records in flight in one instance"),
]
RUN_STATE = ("time-before", "stopped")      # the GPU test reaches these two with a run; "life-done" stays synthetic


def refusal_script():
    out = []
    for name, cfg, state, recs, _rc, _text in REFUSALS:
        out += [engine_line("refuse/" + name, cfg)] + state + batch(recs)
    return out


# ---- the dump program --------------------------------------------------------------------------------------------
def build_dump(tmpdir):
    exe = os.path.join(str(tmpdir), "inject_dump")
    # the sanitizer runtimes linked statically: the program runs as it is, whatever else the loader brings in
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tests", "inject_dump.cpp"), "-o", exe])
    return exe


def _kv(text):
    return dict(t.split("=", 1) for t in text.split(" "))


def run_dump(exe, lines):
    """{scenario: {"E": plan fields or refusal, "ops": [inject / run / reset results in script order]}}"""
    run = subprocess.run([exe], input=("\n".join(lines) + "\n").encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         check=False)
    assert run.returncode == 0, run.stderr.decode()[-4000:]
    out, cur, op = {}, None, None
    for ln in run.stdout.decode().splitlines():
        tag, _, body = ln.partition(" ")
        if tag == "E":
            name, _, body = body.partition(" ")
            assert name not in out, name
            rc, _, tail = body.partition(" ")
            cur = out[name] = {"E": dict(rc=int(rc[3:]), why=tail[4:]) if tail.startswith("why=") else
                               {k: int(v) for k, v in _kv(body).items()}, "ops": []}
        elif tag in ("I", "G"):
            if " why=" in body:
                head, _, why = body.partition(" why=")
                op = dict({k: int(v) for k, v in _kv(head).items()}, op=tag, why=why)
            else:
                op = dict({k: int(v) for k, v in _kv(body).items()}, op=tag, J=[], T=[], O=[], why=None)
            cur["ops"].append(op)
        elif tag == "Z":
            op = dict({k: int(v) for k, v in _kv(body).items()}, op=tag)
            cur["ops"].append(op)
        elif tag == "J":
            j = _kv(body)
            dst = [int(w, 16) for w in j.pop("dst").split(",")]
            op["J"].append(dict({k: int(v) for k, v in j.items()}, dst=sum(w << (64 * i) for i, w in enumerate(dst))))
        elif tag == "T":
            t = _kv(body)
            op["T"].append(dict(item=int(t["item"]), count=int(t["count"]), words=[int(w, 16) for w in t["words"].split(",")]))
        elif tag == "O":
            op["O"] = [int(v) for v in body.split()]
        elif tag == "K":
            op["K"] = {k: int(v) for k, v in _kv(body).items()}
        else:
            raise AssertionError(ln)
    return out


def decode_table(t, wide):
    """The packed words of one table back into records, through XS_TYPE_SH, WREC_NODE_SH and WREC_W; the words past
    the count must be zero."""
    W = WREC_W if wide else 3
    assert len(t["words"]) == W * XSEND_MAX and t["count"] <= XSEND_MAX
    assert not any(t["words"][W * t["count"]:])
    out = []
    for j in range(t["count"]):
        w = t["words"][W * j:W * (j + 1)]
        r = dict(slot=w[0] & 0xFFFF, t=(w[0] >> 16) & 0xFFFFFF, type=(w[0] >> XS_TYPE_SH) & 0xFF)
        if wide:
            r.update(type=(w[0] >> XS_TYPE_SH) & 0xFF, node=w[0] >> WREC_NODE_SH, dst=sum(x << (64 * i) for i, x in enumerate(w[1:])))
            assert (w[0] >> 40) & 0xFF == 0
        else:
            r.update(seg=(w[0] >> 40) & 0xFF, type=w[0] >> XS_TYPE_SH, smask=w[1], dst=w[2])
        out.append(r)
    return out
