"""Preconditions of tests/test_gpu_key_domain.py, checked without a GPU on the C oracle alone: every batch of
tests/key_domain_workloads.py does real work (some instance ends done with every honest replica decided, none
overflows), and the high word it places matters -- the oracle's result on each low-word twin (the batch a kernel
computes that loses the word) differs from its result on the batch, under carry on an instance past the boundary.  So
the GPU test's comparison with the oracle fails for a kernel that drops seed >> 32, coin_seed >> 32 or g >> 32, loses the
carry of inst_offset + inst, or shares one g_hi among the instances of a wave item.  The oracle's own draw is pinned for
64-bit seeds and 40-bit ids by tests/test_schedule.py.

Also here, host side: shard.shard_range tiles ranges beyond 2^32 and 2^63 exactly, and the brc_config struct carries
64-bit seeds and offsets unchanged.

The whole file takes about 70 s on 8 cores (the oracle runs of the n = 129 and n = 130 batches are most of it)."""
import pytest

from tests import key_domain_workloads as K
from tests import step_noevent_workloads as T

BATCHES = K.batches()


def test_table_has_every_family_in_every_placement():
    fams = K.families()
    assert [f.name for f in fams] == list(K.INTENDED) and len(fams) == 15
    assert [(b.family.name, b.placement) for b in BATCHES] == [(f.name, p) for f in fams for p in K.PLACEMENTS]
    packed = [f for f in fams if f.npad < 64]
    assert [f.npad for f in packed] == [4, 8, 16, 32] and sorted(f.mode for f in packed) == [K.REF, K.SPEC, K.BEB, K.CONN]
    assert sum(f.n == f.npad for f in packed) == 2 and sum(f.n < f.npad for f in packed) == 2
    for f in fams:
        assert f.npad // 2 < f.n <= f.npad, f.name
        assert f.count == (3 * (64 // f.npad) + 1 if f.npad < 64 else 5 if f.npad == 64 else 3), f.name
        assert f.round_cap == (2 if f.n <= 64 else 1), f.name
        assert 0 < f.c < f.count and (f.npad >= 64 or f.c % (64 // f.npad)), (f.name, f.c)
    assert {f.kind for f in fams} == {"step", "life", "wide_life", "pattern"}
    assert set(K.PER_KERNEL_FILE.values()) <= {f.name for f in fams}
    assert set(K.COIN_DIFFERS) == {f.name for f in fams if f.mode == K.SPEC}
    assert {T.pick_npad(f.n) for f in fams if f.mode == K.SPEC} == {8, 64, 128, 256}


def test_placements_put_the_high_bits_where_they_say():
    for hi in (K.HI, K.CHI, K.TOP_HI, K.TOP_CHI):
        assert hi & 1 and hi >> 16 and hi & 0xFFFF and hi < 2 ** 32
    assert K.TOP_HI >> 31 and K.TOP_CHI >> 31
    for b in BATCHES:
        f, sp = b.family, b.specs
        assert [s["g"] for s in sp] == list(range(sp[0]["g"], sp[0]["g"] + f.count)), b.label
        assert all(0 <= s["g"] < 2 ** 64 for s in sp), b.label
        assert b.run["proposals"] == ("loaded" if b.placement == "seed-hi" and f.mode == K.SPEC else "philox"), b.label
        seed, g0 = sp[0]["seed"], sp[0]["g"]
        assert seed & K.M32 == f.lo < 2 ** 32
        if b.placement == "seed-hi":
            assert seed >> 32 == K.HI and g0 == K.OFFSET == 777
            if f.mode == K.SPEC:
                assert sp[0]["coin_seed"] == K.CLO | K.CHI << 32
        elif b.placement == "g-hi":
            assert seed < 2 ** 32 and g0 == 3 * 2 ** 32 + 777
        elif b.placement == "carry":
            assert seed < 2 ** 32 and g0 == 2 ** 32 - f.c
            assert [s["g"] >> 32 for s in sp] == [0] * f.c + [1] * (f.count - f.c)
            assert b.past_boundary() == list(range(f.c, f.count))
        else:
            assert g0 == 2 ** 64 - 100 and sp[-1]["g"] < 2 ** 64 and seed >> 63 == 1 and g0 >> 63 == 1
            if f.mode == K.SPEC:
                assert sp[0]["coin_seed"] >> 63 == 1
        # the twins: the same batch with one high word gone
        for what, twin in b.twins:
            for s, t in zip(sp, twin.specs):
                gone = {k for k in s if k != "name" and s[k] != t[k]}
                if what.startswith("seed"):
                    assert {"seed"} <= gone <= {"seed", "actions"} and t["seed"] == s["seed"] & K.M32, (b.label, what)
                elif what.startswith("coin"):
                    assert gone == {"coin_seed"} and t["coin_seed"] == s["coin_seed"] & K.M32, (b.label, what)
                else:
                    # Philox proposals follow the id: the propose actions differ with it
                    assert gone <= {"g", "actions"} and t["g"] == s["g"] & K.M32, (b.label, what)
        assert [w for w, _ in b.twins] == (["seed & 0xFFFFFFFF"] + ["coin_seed & 0xFFFFFFFF"] * (f.mode == K.SPEC)
                                           if b.placement == "seed-hi" else ["g & 0xFFFFFFFF"]), b.label


def test_every_step_family_lands_on_the_instantiation_it_names():
    """brc_create's rules as step_noevent_workloads.instantiation restates them; the lifetime families are held to
    their kernel by last_kernel() in the GPU test."""
    for b in BATCHES:
        want = K.INTENDED[b.family.name]
        if b.family.kind == "step":
            assert T.instantiation(b.specs[0], b.key_window) == want, b.label
        else:
            assert want == "life", b.label
    forms = {K.INTENDED[f.name][1:] for f in K.families() if f.kind == "step" and f.npad == 64}
    assert forms == {(64, 8, K.REF, 0), (64, 8, K.BEB, 2), (64, 8, K.XREF, 0)}          # lean, register masks, general
    wide = {K.INTENDED[f.name] for f in K.families() if f.kind == "step" and f.npad > 64}
    assert {w[1] for w in wide} == {128, 256} and {w[4] for w in wide} == {0, 4} and any(w[3] == K.SPEC for w in wide)
    # the lifetime kernel's forms: two-class (constant / slow-set) and per-link (uniform / geometric)
    life = [f for f in K.families() if f.kind == "life"]
    assert sorted((f.model in (K.UNIF, K.GEO), f.mode) for f in life) == [(False, K.REF), (False, K.SPEC), (True, K.CONN)]


@pytest.mark.parametrize("label", [b.label for b in BATCHES])
def test_batch_preconditions(label):
    b = K.by_label()[label]
    f = b.family
    hon = [d for d in range(f.n) if d not in f.byz]
    res = T.oracle_results(b)
    assert sorted(res) == list(range(f.count)), (label, "every instance is compared")
    assert not any(exp["status"] == "overflow" for exp, _d, _n in res.values()), label
    worked = [i for i, (exp, dec, _n) in res.items() if exp["status"] == "done" and all(d in dec for d in hon)]
    assert worked, (label, "no instance ends done with every honest replica decided")
    for what, twin in b.twins:
        diff = K.differing(b, twin)
        print(label, what, "differs on", len(diff), "of", f.count, "done and decided:", len(worked))
        assert diff, (label, what, "the oracle computes the twin's result: the high word does not show")
        if b.placement == "carry":
            # before the boundary batch and twin are one spec; the instances past it are the ones that can differ
            assert set(diff) <= set(b.past_boundary()) and diff, (label, diff)
        if what.startswith("coin"):
            assert diff == K.COIN_DIFFERS[f.name], (label, diff)
            # a coin round happened there: the replicas decide after round 1
            assert all(min(r for rows in res[i][1].values() for (r, _t, _v) in rows) > 1 for i in diff), label


def test_shard_range_tiles_ranges_beyond_32_and_63_bits():
    from byzantinerandomizedconsensus_amd import shard
    for total in (2 ** 40 + 3, 2 ** 63 + 5):
        world, nxt, counts = 8, 0, []
        for rank in range(world):
            first, count = shard.shard_range(total, world, rank)
            assert type(first) is int and type(count) is int
            assert first == nxt, (total, rank)
            nxt = first + count
            counts.append(count)
        assert nxt == total == sum(counts) and max(counts) - min(counts) <= 1, (total, counts)
        assert counts == sorted(counts, reverse=True)           # the first total % world ranks take the extra one


def test_config_struct_carries_64_bit_seeds_and_offsets():
    """The ctypes brc_config (the fields Engine fills): no GPU and no library."""
    import ctypes

    from byzantinerandomizedconsensus_amd import _lib as L
    x, seed, coin = 2 ** 64 - 100, 0x4B1D0403 | K.TOP_HI << 32, K.CLO | K.TOP_CHI << 32
    cfg = L.Config(n=4, f=1, instances=3, instance_offset=x, seed=seed, coin_seed=coin)
    assert (cfg.instance_offset, cfg.seed, cfg.coin_seed) == (x, seed, coin)
    raw = ctypes.string_at(ctypes.byref(cfg), ctypes.sizeof(cfg))
    for field, value in (("instance_offset", x), ("seed", seed), ("coin_seed", coin)):
        off = getattr(L.Config, field).offset
        assert getattr(L.Config, field).size == 8 and off % 8 == 0
        assert int.from_bytes(raw[off:off + 8], "little") == value, field
    cfg.instance_offset = 3 * 2 ** 32 + 777
    assert cfg.instance_offset == 3 * 2 ** 32 + 777
