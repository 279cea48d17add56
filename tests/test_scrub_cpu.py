"""CPU tier: the scrub batch's host arithmetic and argument contract
(include/isal_hip.h "scrub batch"), no GPU.

Expected answers come from the small model below, written with the oracle's
gf_mul / gf_inv; it implements the header's per-column rule and never calls
the library. tests/test_scrub_gpu.py feeds the same model with the oracle's
parity. Every refusal of isal_hip_scrub_create below is decided before the
first HIP call; the pointers are addresses that are never dereferenced.
"""
import ctypes
import random
from functools import lru_cache

import numpy as np
import pytest

EINVAL, ESINGULAR = -1, -5
CLEAN, MULTI = 0xFFFFFFFF, 0xFFFFFFFE
U8P = ctypes.POINTER(ctypes.c_ubyte)


# ---- the model ---------------------------------------------------------------

@lru_cache(maxsize=1)
def _gf(oracle):
    """(256 x 256 product table, inverse table) from the oracle."""
    mul = np.array([[oracle.gf_mul(a, b) for b in range(256)] for a in range(256)], np.uint8)
    inv = np.array([0] + [oracle.gf_inv(a) for a in range(1, 256)], np.uint8)
    return mul, inv


def model_locate(oracle, coef, k, rows, e):
    """The header's rule for one byte column's syndrome e (rows values):
    CLEAN, the shard it names, or MULTI. coef: rows x k, row-major."""
    mul, inv = _gf(oracle)
    e = [int(x) for x in e]
    if not any(e):
        return CLEAN
    for j in range(k):
        col = [int(coef[l * k + j]) for l in range(rows)]
        p = next((l for l in range(rows) if col[l]), None)
        if p is None:
            continue
        d = int(mul[e[p], inv[col[p]]])
        if d and all(int(mul[col[l], d]) == e[l] for l in range(rows)):
            return j
    nz = [l for l in range(rows) if e[l]]
    return k + nz[0] if len(nz) == 1 else MULTI


def model_verdict(oracle, coef, k, rows, stored_parity, true_parity):
    """A stripe's verdict from its stored parity rows and the oracle's parity
    of its stored sources (lists of rows uint8 arrays): every mismatching
    column must name the same shard."""
    diff = [np.bitwise_xor(s, t) for s, t in zip(stored_parity, true_parity)]
    cols = np.nonzero(np.bitwise_or.reduce(diff))[0]
    named = {model_locate(oracle, coef, k, rows, [d[c] for d in diff]) for c in cols}
    if not named:
        return CLEAN
    return named.pop() if len(named) == 1 and MULTI not in named else MULTI


def matrix(oracle, kind, k, rows):
    """rows x k parity coefficients: rs, cauchy, or pq (rows {1..1}, {2^j})."""
    if kind == "rs":
        return oracle.gf_gen_rs_matrix(k + rows, k)[k * k:].copy()
    if kind == "cauchy":
        return oracle.gf_gen_cauchy1_matrix(k + rows, k)[k * k:].copy()
    assert kind == "pq" and rows == 2
    q, p = [], 1
    for _ in range(k):
        q.append(p)
        p = oracle.gf_mul(p, 2)
    return np.array([1] * k + q, np.uint8)


MATRICES = [("rs", 4, 2), ("rs", 10, 4), ("cauchy", 20, 8), ("pq", 6, 2)]


# ---- locate_syndrome ---------------------------------------------------------

@pytest.mark.parametrize("kind,k,rows", MATRICES)
def test_locate_syndrome_against_the_model(engine, oracle, kind, k, rows):
    coef = matrix(oracle, kind, k, rows)
    tbls = oracle.ec_init_tables(k, rows, coef)
    mul, _ = _gf(oracle)
    cases = [[0] * rows]
    for j in range(k):  # every multiple of every column of C
        cases += [[int(mul[int(coef[l * k + j]), d]) for l in range(rows)] for d in range(1, 256)]
    for l in range(rows):  # every single-row syndrome
        cases += [[v if r == l else 0 for r in range(rows)] for v in range(1, 256)]
    rng = random.Random(1000 * k + rows)
    cases += [[rng.randrange(256) for _ in range(rows)] for _ in range(2000)]
    seen = set()
    for e in cases:
        want = model_locate(oracle, coef, k, rows, e)
        got = engine.locate_syndrome(k, rows, tbls, np.array(e, np.uint8))
        assert got == want, (e, got, want)
        seen.add(want if want in (CLEAN, MULTI) else "data" if want < k else "parity")
    # the cases reach every kind of answer (rows = 2 random syndromes are mostly MULTI)
    assert seen == {CLEAN, MULTI, "data", "parity"}
    # the column multiples name their column, the single rows their row
    assert engine.locate_syndrome(k, rows, tbls, np.array(cases[1 + 255 * (k - 1)], np.uint8)) == k - 1
    assert engine.locate_syndrome(k, rows, tbls, np.array(cases[1 + 255 * k], np.uint8)) == k


def test_locate_syndrome_constants(engine):
    assert engine.SCRUB_CLEAN == CLEAN and engine.SCRUB_MULTI == MULTI
    assert engine.ESINGULAR == ESINGULAR


# ---- scrub_ambiguity ---------------------------------------------------------

@pytest.mark.parametrize("kind,k,rows", [("rs", 10, 4), ("cauchy", 20, 8), ("pq", 6, 2)])
def test_scrub_ambiguity_accepts_the_usual_matrices(engine, oracle, kind, k, rows):
    tbls = oracle.ec_init_tables(k, rows, matrix(oracle, kind, k, rows))
    assert engine.scrub_ambiguity(k, rows, tbls) is None


def _ambiguity(engine, oracle, k, rows, coef):
    return engine.scrub_ambiguity(k, rows, oracle.ec_init_tables(k, rows, np.array(coef, np.uint8)))


def test_scrub_ambiguity_names_the_first_offending_pair(engine, oracle):
    # 4 columns, 2 rows: column 3 = 2 * column 1
    assert oracle.gf_mul(2, 2) == 4
    assert _ambiguity(engine, oracle, 4, 2, [1, 1, 1, 2,
                                             1, 2, 3, 4]) == (1, 3)
    # a zero column is its own pair
    assert _ambiguity(engine, oracle, 3, 2, [1, 0, 1,
                                             2, 0, 3]) == (1, 1)
    # a multiple of a unit vector: the column and the parity row it imitates
    assert _ambiguity(engine, oracle, 3, 2, [1, 0, 1,
                                             2, 5, 3]) == (1, 3 + 1)
    assert _ambiguity(engine, oracle, 3, 3, [1, 7, 1,
                                             1, 0, 2,
                                             1, 0, 4]) == (1, 3 + 0)
    # lexicographic: (0, 2) comes before the zero column 1 and before (0, 3)
    assert _ambiguity(engine, oracle, 4, 2, [1, 0, 3, 1,
                                             2, 0, 6, 2]) == (0, 2)
    # nothing wrong: None
    assert _ambiguity(engine, oracle, 3, 2, [1, 1, 1,
                                             1, 2, 3]) is None


def test_scrub_ambiguity_rejects_arguments_outside_the_contract(engine):
    L = engine.lib()
    g = (ctypes.c_ubyte * (32 * 300))()
    pair = (ctypes.c_int * 2)(7, 7)
    assert L.isal_hip_scrub_ambiguity(0, 2, g, pair) == EINVAL and list(pair) == [-1, -1]
    assert L.isal_hip_scrub_ambiguity(4, 0, g, pair) == EINVAL
    assert L.isal_hip_scrub_ambiguity(253, 4, g, pair) == EINVAL
    assert L.isal_hip_scrub_ambiguity(4, 2, None, pair) == EINVAL
    # one row: every pair of sources is proportional; pair is optional
    g[1], g[33] = 1, 9
    assert L.isal_hip_scrub_ambiguity(2, 1, g, pair) == ESINGULAR and list(pair) == [0, 1]
    assert L.isal_hip_scrub_ambiguity(2, 1, g, None) == ESINGULAR


# ---- isal_hip_scrub_create's refusals ---------------------------------------

S = 4


def _ptrs(per_stripe, base, nstripes=S):
    arr = (U8P * (per_stripe * nstripes))()
    for i in range(per_stripe * nstripes):
        arr[i] = ctypes.cast(ctypes.c_void_p(base + 8192 * i), U8P)
    return arr


def _create(engine, oracle, len_=4096, k=10, rows=4, nstripes=S, coef=None, data="good", coding="good",
            gftbls="good", out=True, want_bad=True):
    if coef is None:
        coef = matrix(oracle, "rs", k, min(rows, 8)) if 2 <= rows <= 8 and k + rows <= 256 else np.ones(k * rows, np.uint8)
    g = oracle.ec_init_tables(k, rows, np.array(coef, np.uint8)) if gftbls == "good" else None
    n = max(nstripes, 1)
    data = _ptrs(k, 0x1000000, n) if isinstance(data, str) else data
    coding = _ptrs(rows, 0x9000000, n) if isinstance(coding, str) else coding
    h, bad = ctypes.c_void_p(0xdead), ctypes.c_int(-7)
    rc = engine.lib().isal_hip_scrub_create(
        ctypes.byref(h) if out else None, len_, k, rows,
        ctypes.cast(ctypes.c_void_p(g.ctypes.data), U8P) if g is not None else None, nstripes, data, coding,
        ctypes.byref(bad) if want_bad else None)
    if out and rc != 0:
        assert not h.value, "a failed create returned an object"
    elif out:
        assert h.value and engine.lib().isal_hip_scrub_destroy(h) == 0
    return rc, bad.value


def test_scrub_create_rejects_bad_counts_without_gpu(engine, oracle):
    assert _create(engine, oracle, rows=1) == (EINVAL, -1)  # one row cannot tell shards apart
    assert engine.max_rows_per_pass() == 8
    assert _create(engine, oracle, rows=9) == (EINVAL, -1)  # a syndrome must fit one pass
    assert _create(engine, oracle, k=253, rows=4) == (EINVAL, -1)  # k + rows = 257
    assert _create(engine, oracle, nstripes=0) == (EINVAL, -1)
    assert _create(engine, oracle, len_=-1) == (EINVAL, -1)
    assert _create(engine, oracle, k=0, coef=[1, 2, 3, 4]) == (EINVAL, -1)


def test_scrub_create_rejects_null_arguments_without_gpu(engine, oracle):
    assert _create(engine, oracle, out=False)[0] == EINVAL
    assert _create(engine, oracle, gftbls=None) == (EINVAL, -1)
    assert _create(engine, oracle, data=None) == (EINVAL, -1)
    assert _create(engine, oracle, coding=None) == (EINVAL, -1)


def test_scrub_create_names_the_first_stripe_with_a_bad_pointer(engine, oracle):
    k, rows = 10, 4
    for which, per in (("data", k), ("coding", rows)):
        t = _ptrs(per, 0x1000000 if which == "data" else 0x9000000)
        at = 2 * per + 1
        a = ctypes.cast(t[at], ctypes.c_void_p).value
        t[at] = ctypes.cast(ctypes.c_void_p(0), U8P)  # a NULL shard in stripe 2
        assert _create(engine, oracle, **{which: t}) == (EINVAL, 2), which
        t[at] = ctypes.cast(ctypes.c_void_p(a + 8), U8P)  # a shard at +8 in stripe 2
        assert _create(engine, oracle, **{which: t}) == (EINVAL, 2), which
        t[3 * per] = ctypes.cast(ctypes.c_void_p(0), U8P)  # a later offender does not change the answer
        assert _create(engine, oracle, **{which: t}) == (EINVAL, 2), which
        assert _create(engine, oracle, want_bad=False, **{which: t})[0] == EINVAL


def test_scrub_create_refuses_the_ambiguous_matrix(engine, oracle):
    assert _create(engine, oracle, k=4, rows=2, coef=[1, 1, 1, 2, 1, 2, 3, 4]) == (ESINGULAR, -1)
    assert _create(engine, oracle, k=3, rows=2, coef=[1, 0, 1, 2, 0, 3]) == (ESINGULAR, -1)
    # a bad pointer is reported before the matrix
    t = _ptrs(4, 0x1000000)
    t[4 * 1 + 3] = ctypes.cast(ctypes.c_void_p(0), U8P)
    assert _create(engine, oracle, k=4, rows=2, coef=[1, 1, 1, 2, 1, 2, 3, 4], data=t) == (EINVAL, 1)


def test_scrub_create_passes_the_checks_with_sound_arguments(engine, oracle):
    """Whatever a create with a sound argument set returns on this host (0 with
    a GPU, a HIP or pointer-kind code without), it is no refusal of the matrix
    and names no stripe."""
    for kind, k, rows in MATRICES:
        rc, bad = _create(engine, oracle, k=k, rows=rows, coef=matrix(oracle, kind, k, rows))
        assert rc != ESINGULAR and bad == -1, (kind, rc, bad)


def test_scrub_run_and_destroy_reject_null(engine):
    L = engine.lib()
    word = (ctypes.c_uint * 1)()
    assert L.isal_hip_scrub_run(None, word, None) == EINVAL
    assert L.isal_hip_scrub_run(None, None, None) == EINVAL
    assert L.isal_hip_scrub_destroy(None) == 0
