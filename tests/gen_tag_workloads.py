"""Workload table of tests/test_gpu_gen_tags.py (GPU) and tests/test_gen_tag_workloads.py (its preconditions, on
the oracle alone): many epochs (brc_reset / brc_reset_at to the next) on ONE engine of every non-lean narrow step
kernel, the ones whose cells carry a 13-bit allocation generation and are never swept (csrc/brc_step.h; DESIGN.md
section 3, "Key slots").  A cell whose tag differs from its slot's generation is stale in every field; a reset keeps
the generations, so exactness rests on the host's count of them (csrc/brc_engine.hip gen_used).

A case: name, family (FAMILIES: one per tagged kernel family), a small batch (consecutive global ids from 777, at
most 8 instances), and the walks it takes part in.  A walk is a list of epochs, each a batch of harness specs:

  wrap        every epoch: K[i] byz_key records of ONE Byzantine key (kp, s) at steps 1 .. K[i]; in the even epochs
              then that key's SEND to every peer at step K[i] + 1 (declared by then: the SEND allocates nothing, the
              cells are written under the tag the KEYs left), in the odd epochs the SEND of the key (kp, s + 1) in
              the slot beside it.  (With the SEND in every epoch each epoch rewrites the cells the one before left,
              and no stale cell lives long enough to meet its tag again: that walk passed before the host counted
              the KEYs.)  Instance 0 has K = K_WRAP, which divides 8192; its siblings in the wave
              item have K' = K_ODD (no divisor) or the one KEY that declares the key at the SEND's step, so they
              sit at other tags.  8192 / K + 8 epochs.
  wrap_at     the same, re-keyed: reset_at(777 + count) and reset_at(777) alternate, so stale cells belong to
              other global ids.
  full_clear  BRB, one SEND at phase index S_BIG per instance: the host books S_BIG / Q + 2 generations per epoch
              and brc_reset clears fully once GEN_FULL_CLEAR is crossed.  Two batches alternate (other values, a
              restricted SEND in the odd ones: GEN_RESTRICTED and kdst across the clear).
  s_limit     key window 2, the smallest the engine has: after an epoch at S_BIG the next one's s_limit is below
              the 14-bit bound; a SEND at s_limit - 1 runs, one at s_limit stops its instance with BRC_OVERFLOW.
  consensus   the in-kernel allocations (send_key_now): one consensus batch over and over until gen_base has
              crossed GEN_FULL_CLEAR, and on to where an engine that never cleared would run out of tags.

K_WRAP.  Nothing in brc_inject or upload_injections bounds the number of records.  A slot takes one allocating
record per step (a second one finds t < t_quiet = t + 1: BRC_OVERFLOW) and t <= step_cap <= STEP_LIMIT = 60000; the
bound that bites is the tag itself: brc_run refuses an epoch whose records could advance one slot by GEN_MASK - 2 or
more (BRC_E_STATE; 8192 KEYs of one key would bring the tag back inside one epoch).  4096 is the largest divisor
of 8192 below that.
"""
from tests import interleaved_workloads as I
from tests.golden import specs as S

OFFSET = I.OFFSET
REF, SPEC, BEB, CONN, XREF = I.REF, I.SPEC, I.BEB, I.CONN, I.XREF
CONST, UNIF, SLOW = I.CONST, I.UNIF, I.SLOW

# csrc/brc_internal.h, csrc/brc_engine.hip
GEN_BITS = 13
GEN_MASK = (1 << GEN_BITS) - 1
GEN_FULL_CLEAR = 6000
GEN_HARD = GEN_MASK - 2
S_14BIT = 0x3FFE
STEP_LIMIT = 60000

K_WRAP = 4096                 # module docstring
K_ODD = 100                   # no divisor of 8192
S_BIG = 4000
FAMILIES = ("packed4", "packed8", "packed16", "packed32", "general64", "conn64", "conn8", "spec", "beb")
WALKS = ("wrap", "wrap_at", "full_clear", "s_limit", "consensus")


# ---- the host's book-keeping, restated (csrc/brc_engine.hip gen_used, brc_run, brc_reset) -------------------------
def excess_records(records, consensus, Q):
    """records: the (instance, kp, s, kind) of an epoch's KEY and SEND injections.  Per key slot the records that
    can allocate it beyond one per key; under the consensus protocol every record counts (the kernel may allocate
    the key itself).  The largest count over the slots."""
    per_key, per_slot = {}, {}
    for (inst, kp, s, _kind) in records:
        c = per_key[(inst, kp, s)] = per_key.get((inst, kp, s), 0) + 1
        if c > 1 or consensus:
            per_slot[(inst, kp, s % Q)] = per_slot.get((inst, kp, s % Q), 0) + 1
    return max(per_slot.values(), default=0)


def gen_used(smax, Q, excess=0, passes=1):
    """Generations one epoch can have advanced a slot by, plus one to spare: passes * (smax / Q + 1) + excess + 1."""
    return passes * (smax // Q + 1) + excess + 1


def parent_gen_used(smax, Q):
    """What the host booked before it counted injected records: max phase index / Q + 2."""
    return smax // Q + 2


def s_limit(gen_base, Q, excess=0, passes=1):
    """brc_run's P.s_limit: phase indices from here on are BRC_OVERFLOW."""
    return min(S_14BIT, (GEN_HARD - 1 - gen_base - excess) // passes * Q)


def host_walk(used, staged=None, full_clear=GEN_FULL_CLEAR):
    """used[e]: gen_used of epoch e; staged[e]: the same before its first brc_run, from the staged records alone
    (no phase index seen yet; 2 without records).  (gen_base at the start of every epoch, the epochs whose
    brc_reset or first brc_run cleared fully)."""
    base, bases, clears = 0, [], []
    for e in range(len(used)):
        if e > 0:
            if base + used[e - 1] >= full_clear:
                base = 0
                clears.append(e)
            else:
                base += used[e - 1]
            # the first brc_run of the epoch, nothing run yet
            if base > 0 and base + (staged[e] if staged else 2) >= full_clear:
                base = 0
                clears.append(e)
        bases.append(base)
    return bases, clears


# ---- the kernel's allocation rule, restated (csrc/brc_step.h send_rec) --------------------------------------------
def slot_epoch(actions, tag, cells, mask=GEN_MASK):
    """One instance, one epoch, the records of ONE key slot in time order: a KEY always allocates (gen + 1); a
    SEND allocates unless its key is declared and not yet sent, and the key's deliveries then write the slot's
    cells under the tag.  The slot starts the epoch free, at `tag` (a reset keeps it); cells: the tag its cells
    carry from an earlier allocation (None: fresh).  Returns (tag, cells, whether a SEND found the cells of an
    earlier allocation under its own tag: stale cells that read as current)."""
    key, sent, hazard, since = None, False, False, 1
    for a in sorted(actions, key=lambda a: a["t"]):
        k = (a["kp"], a["s"])
        if a["kind"] == "byz_key":
            tag, key, sent, since = (tag + 1) & mask, k, False, since + 1
        elif a["kind"] == "byz" and a["type"] == S.SEND or a["kind"] == "brb_send":
            if not (key == k and not sent):
                tag, since = (tag + 1) & mask, since + 1
            hazard = hazard or (since > 0 and cells == tag)
            key, sent, cells, since = k, True, tag, 0
    return tag, cells, hazard


def first_reuse(epochs, i, Q, clears=(), mask=GEN_MASK):
    """Instance i over the walk: the first epoch in which some slot's SEND finds cells an earlier epoch (since the
    last full clear) left under the very tag the slot has come back to.  None: never."""
    state = {}
    for e, specs in enumerate(epochs):
        if e in clears:
            state = {}
        for slot, acts in slot_records(specs[i], Q).items():
            tag, cells = state.get(slot, (0, None))
            tag, cells, hazard = slot_epoch(acts, tag, cells, mask)
            state[slot] = (tag, cells)
            if hazard:
                return e
    return None


def slot_records(sp, Q):
    """{(kp, s % Q): the KEY / SEND records of that key slot}"""
    out = {}
    for a in sp["actions"]:
        if a["kind"] in ("byz_key", "brb_send") or a["kind"] == "byz" and a["type"] == S.SEND:
            out.setdefault((a["kp"], a["s"] % Q), []).append(a)
    return out


def alloc_records(specs):
    """(instance, kp, s, kind) of every KEY / SEND injection of a batch (engine_runner._injections' records)."""
    out = []
    for i, sp in enumerate(specs):
        for a in sp["actions"]:
            if a["kind"] in ("byz_key", "brb_send") or a["kind"] == "byz" and a["type"] == S.SEND:
                out.append((i, a["kp"], a["s"], a["kind"]))
    return out


# ---- cases --------------------------------------------------------------------------------------------------------
class Case:
    """make(g, i, actions) -> spec of global id g, local id i, with the given extra actions; probe(i) -> the (kp, s)
    every honest replica of instance i must deliver; byz: the Byzantine replicas."""

    def __init__(self, name, family, inst, n, byz, make, count, key_window, walks, consensus=False, probe_s=0,
                 msgs=False):
        self.name, self.family, self.inst, self.n, self.byz = name, family, inst, n, list(byz)
        self.make, self.count, self.key_window, self.walks, self.consensus = make, count, key_window, walks, consensus
        self.probe_s, self.msgs = probe_s, msgs
        self._walks = {}

    def open_kw(self):
        return dict(key_window=self.key_window)

    def K(self, i):
        return K_WRAP if i == 0 else K_ODD if i % 2 else 0

    def _spec(self, walk, tag, g, i, actions, probe, cap):
        return dict(self.make(g, i, actions), name="%s/%s/%s/%d" % (self.name, walk, tag, i), step_cap=cap, probe=probe)

    def _wrap_batch(self, off, tag, walk, odd=False):
        """odd: the K KEYs go to the probed slot as in the even epochs, but the key SENT and delivered is the next
        phase index, in the slot beside it -- the probed slot's cells stay as the epoch before left them."""
        b = self.byz[0]
        allm = (1 << self.n) - 1
        specs = []
        for i in range(self.count):
            K, key = self.K(i), (b, self.probe_s)
            acts = [dict(t=1 + j, kind="byz_key", kp=b, s=key[1], value=1) for j in range(K)]
            if K == 0:          # no run of KEYs: the key is declared at the SEND's own step
                acts = [dict(t=1, kind="byz_key", kp=b, s=key[1], value=1)]
            if odd:
                key = (b, self.probe_s + 1)
                acts.append(dict(t=K + 1, kind="byz_key", kp=b, s=key[1], value=2))
            acts.append(dict(t=K + 1, kind="byz", src=b, type=S.SEND, kp=b, s=key[1], dst=allm))
            if self.msgs:       # connection peers: the Byzantine replicas' ECHO / READY fill the send-count rings
                acts += I.byz_msgs(K + 2, self.byz, [key], self.n) + I.byz_msgs(K + 3, self.byz[:1], [key], self.n)
            specs.append(self._spec(walk, tag, off + i, i, acts, key, K_WRAP + 400))
        return specs

    def walk(self, walk):
        """[(batch tag, global id offset, specs)] per epoch."""
        if walk not in self._walks:
            self._walks[walk] = getattr(self, "_" + walk)()
        return self._walks[walk]

    def _wrap(self):
        a, b = self._wrap_batch(OFFSET, "a", "wrap"), self._wrap_batch(OFFSET, "b", "wrap", odd=True)
        return [("a", OFFSET, a) if e % 2 == 0 else ("b", OFFSET, b) for e in range(8192 // K_WRAP + 8)]

    def _wrap_at(self):
        a, b = self._wrap_batch(OFFSET, "a", "wrap_at"), self._wrap_batch(OFFSET + self.count, "b", "wrap_at", odd=True)
        return [("a", OFFSET, a) if e % 2 == 0 else ("b", OFFSET + self.count, b) for e in range(8192 // K_WRAP + 8)]

    def _full_clear(self):
        o, b = 0, self.byz[0]
        allm = (1 << self.n) - 1
        A = [self._spec("full_clear", "a", OFFSET + i, i,
                        [dict(t=i % 3, kind="brb_send", node=o, kp=o, s=S_BIG, payload="TEST 1.%d" % S_BIG)], (o, S_BIG), 600)
             for i in range(self.count)]
        # the odd epochs: a Byzantine origin's key, other value ids; in instance 0 it is SENT to every replica but
        # honest replica 1, and the origin's own ECHO makes up the quorum, so replica 1 delivers it as well
        B = [self._spec("full_clear", "b", OFFSET + i, i,
                        I.restricted_send(1 + i % 2, b, S_BIG, allm & ~2 if i == 0 else allm, value=2 + i % 2) +
                        [dict(t=2 + i % 2, kind="byz", src=b, type=S.ECHO, kp=b, s=S_BIG, dst=allm)],
                        (b, S_BIG), 600) for i in range(self.count)]
        return [("a", OFFSET, A) if e % 2 == 0 else ("b", OFFSET, B) for e in range(10)]

    def _s_limit(self):
        o, Q = 0, self.key_window

        def batch(tag, ss):
            return [self._spec("s_limit", tag, OFFSET + i, i,
                               [dict(t=1 + i, kind="brb_send", node=o, kp=o, s=s, payload="TEST 1.%d" % s)], (o, s), 600)
                    for i, s in enumerate(ss)]
        first = batch("a", [S_BIG] * self.count)
        lim = s_limit(gen_used(S_BIG, Q), Q)
        assert lim < S_14BIT
        # instance 1 stands at the limit, its siblings below it
        second = batch("b", [lim - 1, lim] + [5 + i for i in range(self.count - 2)])
        return [("a", OFFSET, first), ("b", OFFSET, second), ("a", OFFSET, first)]

    def _consensus(self):
        specs = [self._spec("consensus", "a", OFFSET + i, i, (), None, 4000) for i in range(self.count)]
        used = self.consensus_used(specs)
        # past the full clear, and on to where the tags of an engine that never cleared would be spent
        return [("a", OFFSET, specs)] * ((GEN_HARD + used - 1) // used + 2)

    def smax(self, specs):
        """The largest phase index any replica SENDs on the oracle, or a record carries."""
        from oracle import oracle
        own = max(e[4] for sp in specs for e in oracle.run(sp, kinds=("send",))["events"]["send"] if e[2] == S.SEND)
        return max([own] + [s for (_i, _kp, s, _k) in alloc_records(specs)])

    def consensus_used(self, specs):
        """gen_used of one epoch of the consensus walk (one PROPOSE per replica: one pass)."""
        return gen_used(self.smax(specs), self.key_window, excess_records(alloc_records(specs), True, self.key_window))


class Batch:
    """What tests.test_gpu_interleaved.oracle_mismatches and interleaved_workloads.oracle_results ask of a case."""

    def __init__(self, case, walk, tag, specs):
        self.name = "gen/%s/%s/%s" % (case.name, walk, tag)
        self.specs, self.byz, self.consensus = specs, case.byz, case.consensus


def _build():
    out = []

    def add(*a, **kw):
        out.append(Case(*a, **kw))

    # (the reference protocol under slow-set delays: uniform ones stall it -- an ECHO ahead of the SEND; tuned on the
    # oracle as in step_noevent_workloads.TUNED)
    def brb(n, f, seed, byz, mode=None, dmax=3, model=SLOW, rdmax=4, **kw):
        def make(g, i, actions):
            if mode == "spec":
                sp = S.spec_brb_spec(n, f, seed, UNIF, dmax, g, [], byzantine=byz, extra=actions, window=4)
            elif mode == "beb":
                sp = S.beb_spec(n, seed, UNIF, dmax, g, [], byzantine=byz, extra=actions)
            else:
                sp = S.brb_spec(n, f, seed, model, rdmax, g, [], byzantine=byz, extra=actions, **kw)
            return sp
        return make

    def general(make):
        return lambda g, i, actions: dict(make(g, i, actions), general_keys=True)

    # NPAD 4, 16 instances per wave item: the five share one item and one key list
    # (slow-set delays at n = 4: these batches showed the NPAD 4 kernel counting the NEXT instance's slow replicas
    # among an instance's senders -- arrivals 25 against the oracle's 21 on a fresh engine; slowset4_specs below)
    add("p4", "packed4", ("step", 4, 4, REF, 0), 4, [3], brb(4, 1, 0x6E7A0004, [3]), 5, 4,
        ("wrap", "wrap_at", "full_clear"))
    add("p8", "packed8", ("step", 8, 4, REF, 0), 7, [6], brb(7, 2, 0x6E7A0008, [6]), 3, 2, ("wrap", "s_limit"))
    # (uniform delays, so that the re-keyed batch differs; seed tuned on the oracle: every replica delivers)
    add("p16", "packed16", ("step", 16, 4, REF, 0), 13, [12], brb(13, 4, 0x6E7A1710, [12], model=UNIF, rdmax=3), 3, 4,
        ("wrap", "wrap_at", "full_clear"))
    add("p32", "packed32", ("step", 32, 4, REF, 0), 25, [24], brb(25, 8, 0x6E7A0020, [24]), 2, 4, ("wrap",))
    add("n40-xref", "general64", ("step", 64, 4, XREF, 0), 40, [39], general(brb(40, 13, 0x6E7A0040, [39])), 2, 4,
        ("wrap", "full_clear"))
    # connection peers: 5 words per cell, the ECHO / READY send-count rings go stale with the cell word
    add("n40-conn", "conn64", ("step", 64, 4, CONN, 0), 40, [38, 39],
        brb(40, 13, 0x6E7A0041, [38, 39], peer_mode="connection"), 2, 4, ("wrap", "wrap_at", "full_clear"), msgs=True)
    add("n6-conn", "conn8", ("step", 8, 4, CONN, 0), 6, [5], brb(6, 1, 0x6E7A0006, [5], peer_mode="connection"), 3, 4,
        ("wrap",), msgs=True)
    # SPEC broadcast, Q = 4: the probed key's phase index 6 wraps the window (slot 6 % 4)
    add("p8-spec", "spec", ("step", 8, 4, SPEC, 0), 7, [6], brb(7, 2, 0x6E7A0108, [6], mode="spec"), 3, 4,
        ("wrap", "full_clear"), probe_s=6)
    add("p8-beb", "beb", ("step", 8, 4, BEB, 0), 7, [6], brb(7, 0, 0x6E7A0208, [6], mode="beb"), 3, 4, ("wrap",))

    # the consensus pass's own allocations.  The reference protocol keeps more phase indices of one origin in flight
    # with every round (13 by round 8, specs.scenario_groups), so no key window lets its own phase indices book 30
    # generations an epoch: two rounds at Q = 8, and Byzantine replica 9's key of phase index S_BIG, which every
    # replica delivers and counts, books S_BIG / Q of them.  SPEC buffers exactly its window: 80 rounds at Q = 4
    def ref16(g, i, actions):
        key = I.restricted_send(1, 9, S_BIG, (1 << 10) - 1, value=1 + g % 2)
        return S.cons_spec(10, 3, 0x6E7A0310, SLOW, 4, g, round_cap=2, byzantine=[9], extra=key + list(actions), step_cap=4000)
    add("c16-ref", "packed16", ("step", 16, 4, REF, 0), 10, [9], ref16, 4, 8, ("consensus",), consensus=True)

    def spec8(g, i, actions):
        return S.spec_cons_spec(7, 2, 0x6E7A0308, UNIF, 2, g, round_cap=80, window=4, extra=actions, step_cap=4000)
    add("c8-spec", "spec", ("step", 8, 4, SPEC, 0), 7, [], spec8, 8, 4, ("consensus",), consensus=True)
    assert len({c.name for c in out}) == len(out)
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


def by_name():
    return {c.name: c for c in cases()}


def walk_params():
    return [(c.name, w) for c in cases() for w in c.walks]


oracle_results = I.oracle_results


def slowset4_specs():
    """n = 4 under slow-set delays, 19 instances (a full wave item of 16 and a tail of three): which replica is slow
    differs per instance (schedule.h slow_offset), so the instances of an item see different neighbours.  BRB with
    every replica SENDing, reference consensus, SPEC consensus; f = 1 slow replica, D = 4 and D = 3."""
    out = {}
    out["brb"] = [dict(S.brb_spec(4, 1, 0x6E7A0404, SLOW, 4, OFFSET + i, [(i % 2, o, 0) for o in range(4)]),
                       name="slowset4/brb/%d" % i, step_cap=600) for i in range(19)]
    out["cons"] = [dict(S.cons_spec(4, 1, 0x6E7A0414, SLOW, 3, OFFSET + i, round_cap=2), name="slowset4/cons/%d" % i,
                        step_cap=600) for i in range(19)]
    out["spec"] = [dict(S.spec_cons_spec(4, 1, 0x6E7A0424, SLOW, 4, OFFSET + i, round_cap=2, window=4),
                        name="slowset4/spec/%d" % i, step_cap=600) for i in range(19)]
    return out
