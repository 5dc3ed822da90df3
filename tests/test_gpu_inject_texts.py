"""GPU: the library's brc_inject against the dump of csrc/brc_inject.h (tests/inject_dump.cpp): for every refusing batch
of tests/inject_workloads.py the same engine is created, the same batch is sent, and the return code and
brc_last_error(h) must equal the dump's, byte for byte -- so the header under test is the one that ships.  One instance
per engine.  A kernel is launched for two cases only, where the dump has synthetic state: a three-step run at n = 7
leaves its instance stopped at a step past 0 (time before the current step, instance already stopped)."""
import ctypes

import pytest

from byzantinerandomizedconsensus_amd import _lib as L
from tests import inject_workloads as J

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    return J.run_dump(J.build_dump(tmp_path_factory.mktemp("inject")), J.refusal_script())


def create(lib, cfg):
    h = ctypes.c_void_p()
    rc = lib.brc_create(ctypes.byref(J.lib_config(cfg, instances=1)), ctypes.byref(h))
    assert rc == L.OK, lib.brc_last_error(None)
    return h


def inject(lib, h, recs):
    return lib.brc_inject(h, J.lib_injections(recs), len(recs))


def test_library_refuses_with_the_dumped_texts(dumped):
    lib = L.load()
    checked = 0
    for name, cfg, state, recs, _rc, _text in J.REFUSALS:
        if state or any(x["instance"] for x in recs):       # synthetic state; the instance-range case needs its batch of 3
            continue
        want, = dumped["refuse/" + name]["ops"]
        h = create(lib, cfg)
        try:
            assert inject(lib, h, recs) == want["rc"] != L.OK, name
            assert lib.brc_last_error(h) == want["why"].encode(), name
        finally:
            lib.brc_destroy(h)
        checked += 1
    assert checked >= 22


def test_library_refuses_after_a_run_with_the_dumped_texts(dumped):
    lib = L.load()
    by = {r[0]: r for r in J.REFUSALS}
    h = create(lib, "p7")
    try:
        # a SEND that runs, and at step 2 an ECHO of a key nobody declared: BRC_BADINJ stops the instance there
        work = [J.rec(0, J.S, 0, n=7), J.rec(2, J.M, 6, kp=3, type=L.ECHO, n=7)]
        assert inject(lib, h, work) == L.OK, lib.brc_last_error(h)
        left = ctypes.c_uint32()
        assert lib.brc_run(h, 3, ctypes.byref(left)) == L.OK, lib.brc_last_error(h)
        res = L.InstanceResult()
        assert lib.brc_read_instances(h, 0, 1, ctypes.byref(res)) == L.OK
        assert res.status == L.BADINJ and 1 <= res.t_now <= 3, (res.status, res.t_now)
        for name in J.RUN_STATE:
            want, = dumped["refuse/" + name]["ops"]
            assert inject(lib, h, by[name][3]) == want["rc"] == L.E_STATE, name
            assert lib.brc_last_error(h) == want["why"].encode(), name
    finally:
        lib.brc_destroy(h)
