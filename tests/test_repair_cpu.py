"""CPU tier: the repair batch's host arithmetic and argument contract
(include/isal_hip.h "repair batch"), no GPU.

isal_hip_decode_matrix is checked against ecutil.decode_matrix (the oracle's
restatement of erasure_code_perf.c:134-168), never against the engine itself.
No pattern below may be skipped as undecodable: gf_gen_rs_matrix has no
singular pattern at k=4 m=6 (1-2 erasures) or k=10 m=14 (1-4 erasures), and
gf_gen_cauchy1_matrix none at all; the one singular case is tested as such.
"""
import ctypes
import itertools
import random

import numpy as np

import ecutil

EINVAL, ESINGULAR = -1, -5
SINGULAR_RS_20_28 = (0, 13, 17, 18, 21, 23)


def _check_patterns(engine, oracle, a, k, patterns, seed):
    rng = random.Random(seed)
    n = 0
    for pat in patterns:
        errs = list(pat)
        rng.shuffle(errs)
        want_ret, want_c, want_surv = ecutil.decode_matrix(a, k, errs, oracle)
        assert want_ret == 0, f"the checker calls {errs} singular"
        ret, c, surv = engine.decode_matrix(a, k, errs)
        assert ret == 0, (errs, ret)
        assert surv == want_surv, (errs, surv, want_surv)
        # row i belongs to errs[i], in the caller's (shuffled) order
        assert np.array_equal(c, want_c), (errs, c.reshape(len(errs), k), want_c.reshape(len(errs), k))
        n += 1
    return n


def test_decode_matrix_every_pattern_rs_4_6(engine, oracle):
    k, m = 4, 6
    a = oracle.gf_gen_rs_matrix(m, k)
    pats = [p for n in (1, 2) for p in itertools.combinations(range(m), n)]
    assert _check_patterns(engine, oracle, a, k, pats, 1) == 6 + 15


def test_decode_matrix_every_pattern_rs_10_14_three_erasures(engine, oracle):
    k, m = 10, 14
    a = oracle.gf_gen_rs_matrix(m, k)
    assert _check_patterns(engine, oracle, a, k, itertools.combinations(range(m), 3), 2) == 364


def test_decode_matrix_seeded_patterns_cauchy_20_28_eight_erasures(engine, oracle):
    k, m = 20, 28
    a = oracle.gf_gen_cauchy1_matrix(m, k)
    rng = random.Random(2028)
    pats = [tuple(sorted(rng.sample(range(m), 8))) for _ in range(200)]
    assert _check_patterns(engine, oracle, a, k, pats, 3) == 200


def test_decode_matrix_reports_the_singular_pattern(engine, oracle):
    k, m = 20, 28
    a = oracle.gf_gen_rs_matrix(m, k)
    assert ecutil.decode_matrix(a, k, list(SINGULAR_RS_20_28), oracle)[0] != 0
    assert engine.decode_matrix(a, k, SINGULAR_RS_20_28)[0] == ESINGULAR
    assert engine.ESINGULAR == ESINGULAR
    # its neighbour (one index moved) decodes: the code is about the pattern
    assert engine.decode_matrix(a, k, (1, 13, 17, 18, 21, 23))[0] == 0


def test_decode_matrix_rejects_bad_arguments(engine, oracle):
    k, m = 4, 6
    a = oracle.gf_gen_rs_matrix(m, k)
    assert engine.decode_matrix(a, k, [])[0] == EINVAL
    assert engine.decode_matrix(a, k, [0, 1, 2])[0] == EINVAL  # more than m - k
    assert engine.decode_matrix(a, k, [1, 1])[0] == EINVAL
    assert engine.decode_matrix(a, k, [6])[0] == EINVAL


class _Fake:
    """Shard pointer tables over addresses that are never dereferenced: the
    checks under test run before any GPU use."""

    def __init__(self, m, nstripes):
        self.m, self.n = m, nstripes
        u8p = ctypes.POINTER(ctypes.c_ubyte)
        self.arr = (u8p * (m * nstripes))()
        for i in range(m * nstripes):
            self.arr[i] = ctypes.cast(ctypes.c_void_p(0x10000 + 4096 * i), u8p)

    def set(self, s, i, address):
        self.arr[s * self.m + i] = ctypes.cast(ctypes.c_void_p(address), ctypes.POINTER(ctypes.c_ubyte))
        return self


def _create(engine, a, len_, k, m, nerrs, nstripes, errs, shards, out=True):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    e = np.array(errs, dtype=np.uint8) if errs is not None else None
    h, bad = ctypes.c_void_p(), ctypes.c_int(-7)
    u8p = ctypes.POINTER(ctypes.c_ubyte)
    rc = engine.lib().isal_hip_repair_create(
        ctypes.byref(h) if out else None, len_, k, m, ctypes.cast(ctypes.c_void_p(a.ctypes.data), u8p), nerrs,
        nstripes, ctypes.cast(ctypes.c_void_p(e.ctypes.data), u8p) if e is not None else None,
        shards.arr if shards is not None else None, ctypes.byref(bad))
    assert not h.value, "a failed create returned an object"
    return rc, bad.value


def test_repair_create_rejects_bad_arguments_without_gpu(engine, oracle):
    """Every check that needs no GPU runs before the first HIP call, so the
    codes are the same on a host without one."""
    k, m, S = 4, 6, 3
    a = oracle.gf_gen_rs_matrix(m, k)
    good = [0, 1, 2, 5, 4, 3]  # nerrs = 2
    assert _create(engine, a, 4096, k, m, 0, S, [], _Fake(m, S)) == (EINVAL, -1)  # nerrs = 0
    assert _create(engine, a, 4096, k, m, 3, S, [0, 1, 2] * S, _Fake(m, S)) == (EINVAL, -1)  # nerrs > m - k
    assert _create(engine, a, 4096, k, m, 2, S, [0, 1, 3, 3, 4, 5], _Fake(m, S)) == (EINVAL, 1)  # duplicate
    assert _create(engine, a, 4096, k, m, 2, S, [0, 1, 2, 5, 4, 6], _Fake(m, S)) == (EINVAL, 2)  # index >= m
    assert _create(engine, a, 4096, k, m, 2, S, good, _Fake(m, S).set(2, 3, 0)) == (EINVAL, 2)  # NULL shard
    assert _create(engine, a, 4096, k, m, 2, S, good, _Fake(m, S).set(1, 0, 0x20008)) == (EINVAL, 1)  # % 16 != 0
    assert _create(engine, a, 4096, k, m, 2, S, good, _Fake(m, S), out=False)[0] == EINVAL  # NULL out
    assert _create(engine, a, -1, k, m, 2, S, good, _Fake(m, S))[0] == EINVAL
    assert _create(engine, a, 4096, k, m, 2, 0, good, _Fake(m, S))[0] == EINVAL
    assert _create(engine, a, 4096, k, m, 2, S, None, _Fake(m, S))[0] == EINVAL
    assert _create(engine, a, 4096, k, m, 2, S, good, None)[0] == EINVAL
    L = engine.lib()
    assert L.isal_hip_repair_run(None, None) == EINVAL
    assert L.isal_hip_repair_npatterns(None) == EINVAL
    assert L.isal_hip_repair_destroy(None) == 0


def test_repair_create_names_the_first_singular_stripe_without_gpu(engine, oracle):
    k, m, S, nerrs = 20, 28, 8, 6
    a = oracle.gf_gen_rs_matrix(m, k)
    rng = random.Random(5)
    errs = []
    for s in range(S):
        pat = list(SINGULAR_RS_20_28) if s in (5, 7) else [1, 13, 17, 18, 21, 23 + (s % 4)]
        assert (ecutil.decode_matrix(a, k, pat, oracle)[0] != 0) == (s in (5, 7))
        rng.shuffle(pat)
        errs += pat
    assert _create(engine, a, 8192, k, m, nerrs, S, errs, _Fake(m, S)) == (ESINGULAR, 5)
