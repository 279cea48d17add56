"""CPU tier: the ragged scrub's argument contract (include/isal_hip.h "Ragged
scrub"), no GPU.

Every refusal of isal_hip_scrub_create_ragged is decided before the first HIP
call, in the header's order: counts and NULL arguments, then per stripe its
length and pointers, then the item count at the 4 KiB tile, then the matrix.
The pointers are addresses that are never dereferenced. The model and the
matrices are those of tests/test_scrub_cpu.py.
"""
import ctypes

import numpy as np
import pytest

from test_scrub_cpu import EINVAL, ESINGULAR, MATRICES, U8P, matrix

INTP = ctypes.POINTER(ctypes.c_int)
S = 4
AMBIGUOUS_4_2 = [1, 1, 1, 2, 1, 2, 3, 4]  # column 3 = 2 * column 1


def _ptrs(per_stripe, base, nstripes=S):
    arr = (U8P * (per_stripe * nstripes))()
    for i in range(per_stripe * nstripes):
        arr[i] = ctypes.cast(ctypes.c_void_p(base + 8192 * i), U8P)
    return arr


def _put(t, at, address):
    t[at] = ctypes.cast(ctypes.c_void_p(address), U8P)


def _at(t, at):
    return ctypes.cast(t[at], ctypes.c_void_p).value


def _create(engine, oracle, lens="good", k=10, rows=4, nstripes=S, coef=None, data="good", coding="good",
            gftbls="good", out=True, want_bad=True):
    if coef is None:
        coef = matrix(oracle, "rs", k, rows) if 2 <= rows <= 8 and 1 <= k and k + rows <= 256 else np.ones(
            max(k, 1) * rows, np.uint8)
    g = oracle.ec_init_tables(max(k, 1), rows, np.array(coef, np.uint8)) if gftbls == "good" else None
    n = max(nstripes, 1)
    if isinstance(lens, str):
        lens = [4096 + 21, 0, 5, 3 * 4096][:n] + [16] * max(0, n - 4)
    ln = (ctypes.c_int * n)(*lens) if lens is not None else None
    data = _ptrs(max(k, 1), 0x1000000, n) if isinstance(data, str) else data
    coding = _ptrs(rows, 0x9000000, n) if isinstance(coding, str) else coding
    h, bad = ctypes.c_void_p(0xdead), ctypes.c_int(-7)
    rc = engine.lib().isal_hip_scrub_create_ragged(
        ctypes.byref(h) if out else None, k, rows,
        ctypes.cast(ctypes.c_void_p(g.ctypes.data), U8P) if g is not None else None, nstripes, ln, data, coding,
        ctypes.byref(bad) if want_bad else None)
    if out and rc != 0:
        assert not h.value, "a failed create returned an object"
    elif out:
        assert h.value and engine.lib().isal_hip_scrub_destroy(h) == 0
    return rc, bad.value


def test_ragged_scrub_rejects_bad_counts_without_gpu(engine, oracle):
    assert _create(engine, oracle, rows=1) == (EINVAL, -1)  # one row cannot tell shards apart
    assert engine.max_rows_per_pass() == 8
    assert _create(engine, oracle, rows=9) == (EINVAL, -1)  # a syndrome must fit one pass
    assert _create(engine, oracle, k=253, rows=4) == (EINVAL, -1)  # k + rows = 257
    assert _create(engine, oracle, k=0, coef=[1, 2, 3, 4]) == (EINVAL, -1)
    assert _create(engine, oracle, nstripes=0) == (EINVAL, -1)
    assert _create(engine, oracle, nstripes=-3) == (EINVAL, -1)


def test_ragged_scrub_rejects_null_arguments_without_gpu(engine, oracle):
    assert _create(engine, oracle, out=False)[0] == EINVAL
    assert _create(engine, oracle, gftbls=None) == (EINVAL, -1)
    assert _create(engine, oracle, lens=None) == (EINVAL, -1)
    assert _create(engine, oracle, data=None) == (EINVAL, -1)
    assert _create(engine, oracle, coding=None) == (EINVAL, -1)


def test_ragged_scrub_counts_come_before_the_stripes(engine, oracle):
    """A bad count together with a bad length and a bad pointer names no stripe."""
    t = _ptrs(10, 0x1000000)
    _put(t, 0, 0)
    assert _create(engine, oracle, rows=9, lens=[-1, 0, 0, 0], data=t) == (EINVAL, -1)
    assert _create(engine, oracle, rows=1, lens=[-1, 0, 0, 0], data=t) == (EINVAL, -1)


def test_ragged_scrub_names_the_first_bad_stripe(engine, oracle):
    k, rows = 10, 4
    # a negative length
    assert _create(engine, oracle, lens=[4096, 5, -1, 7]) == (EINVAL, 2)
    assert _create(engine, oracle, lens=[4096, -5, -1, 7]) == (EINVAL, 1)
    assert _create(engine, oracle, lens=[4096, 5, -1, 7], want_bad=False)[0] == EINVAL
    for which, per in (("data", k), ("coding", rows)):
        t = _ptrs(per, 0x1000000 if which == "data" else 0x9000000)
        at = 2 * per + 1
        a = _at(t, at)
        _put(t, at, 0)  # a NULL shard in stripe 2
        assert _create(engine, oracle, **{which: t}) == (EINVAL, 2), which
        _put(t, at, a + 8)  # a shard at +8 in stripe 2
        assert _create(engine, oracle, **{which: t}) == (EINVAL, 2), which
        _put(t, 3 * per, 0)  # a later offender does not change the answer
        assert _create(engine, oracle, **{which: t}) == (EINVAL, 2), which
        # stripes of length 0 are checked too: stripe 1 of the default lengths
        _put(t, 1 * per, a + 4)
        assert _create(engine, oracle, **{which: t}) == (EINVAL, 1), which
        _put(t, 1 * per, 0)
        assert _create(engine, oracle, **{which: t}) == (EINVAL, 1), which
    # a negative length at stripe 2, an unaligned pointer at stripe 1: stripe 1
    t = _ptrs(k, 0x1000000)
    _put(t, 1 * k + 4, _at(t, 1 * k + 4) + 1)
    assert _create(engine, oracle, lens=[4096, 5, -1, 7], data=t) == (EINVAL, 1)
    # ... and the other way round: the length's stripe
    t = _ptrs(rows, 0x9000000)
    _put(t, 3 * rows, 0)
    assert _create(engine, oracle, lens=[4096, -2, 16, 7], coding=t) == (EINVAL, 1)


def test_ragged_scrub_refuses_the_ambiguous_matrix_last(engine, oracle):
    assert _create(engine, oracle, k=4, rows=2, coef=AMBIGUOUS_4_2) == (ESINGULAR, -1)
    assert _create(engine, oracle, k=3, rows=2, coef=[1, 0, 1, 2, 0, 3]) == (ESINGULAR, -1)  # a zero column
    assert _create(engine, oracle, k=4, rows=2, coef=AMBIGUOUS_4_2, lens=[0, 0, 0, 0]) == (ESINGULAR, -1)
    # a bad pointer and a bad length are reported before the matrix
    t = _ptrs(4, 0x1000000)
    _put(t, 4 * 1 + 3, 0)
    assert _create(engine, oracle, k=4, rows=2, coef=AMBIGUOUS_4_2, data=t) == (EINVAL, 1)
    assert _create(engine, oracle, k=4, rows=2, coef=AMBIGUOUS_4_2, lens=[1, 2, 3, -4]) == (EINVAL, 3)


def _big(engine, nstripes, coef):
    """k = 1, rows = 2, every stripe 2^31 - 1 bytes: 2^19 items each at the
    4 KiB tile. One pointer value repeated; (rc, bad, handle)."""
    n = 2**31 - 1
    u8 = ctypes.cast(ctypes.c_void_p(0x7000000), U8P)
    data = (U8P * nstripes)(*([u8] * nstripes))
    coding = (U8P * (2 * nstripes))(*([u8] * (2 * nstripes)))
    g = (ctypes.c_ubyte * 64)()
    g[1], g[33] = coef
    ln = (ctypes.c_int * nstripes)(*([n] * nstripes))
    assert engine.lib().isal_hip_ragged_items(nstripes, ln, 4096, None) == nstripes * 2**19
    h, bad = ctypes.c_void_p(), ctypes.c_int(-7)
    rc = engine.lib().isal_hip_scrub_create_ragged(ctypes.byref(h), 1, 2, ctypes.cast(g, U8P), nstripes, ln, data,
                                                   coding, ctypes.byref(bad))
    return rc, bad.value, h.value


def test_ragged_scrub_refuses_more_than_2_30_items_without_gpu(engine):
    """2048 stripes are exactly 2^30 items and pass the count check, 2049 are
    one launch too many. The refusal comes before any pointer is classified
    and before the matrix: with C = (3, 0), a multiple of parity row 0's unit
    column (ambiguous), 2048 stripes answer ESINGULAR, the check after the
    count, and 2049 EINVAL."""
    assert 2048 * 2**19 == 2**30
    rc, bad, h = _big(engine, 2049, (3, 7))
    assert (rc, bad, h) == (EINVAL, -1, None)
    assert _big(engine, 2049, (3, 0)) == (EINVAL, -1, None)
    assert _big(engine, 2048, (3, 0)) == (ESINGULAR, -1, None)
    # a sound matrix: past every refusal; what follows is the first HIP call
    # (no device) or the pointers' classification (the address is no device
    # memory), never an object, and never the matrix's code
    rc, bad, h = _big(engine, 2048, (3, 7))
    assert rc not in (0, ESINGULAR) and bad == -1 and h is None


def test_ragged_scrub_passes_the_checks_with_sound_arguments(engine, oracle):
    """Whatever a create with a sound argument set returns on this host (0 with
    a GPU, a HIP or pointer-kind code without), it is no refusal of the matrix
    and names no stripe; so with every length 0."""
    for kind, k, rows in MATRICES:
        coef = matrix(oracle, kind, k, rows)
        rc, bad = _create(engine, oracle, k=k, rows=rows, coef=coef)
        assert rc != ESINGULAR and bad == -1, (kind, rc, bad)
        rc, bad = _create(engine, oracle, k=k, rows=rows, coef=coef, lens=[0, 0, 0, 0])
        assert rc != ESINGULAR and bad == -1, (kind, rc, bad)


def test_ragged_scrub_python_wrapper_checks_its_lists(engine, oracle):
    tbls = oracle.ec_init_tables(4, 2, matrix(oracle, "rs", 4, 2))
    with pytest.raises(ValueError):
        engine.Scrub.ragged(4, 2, tbls, [16, 16], [0x1000] * 7, [0x1000] * 4)
    with pytest.raises(RuntimeError, match=r"stripe 1\)"):
        engine.Scrub.ragged(4, 2, tbls, [16, -1], [0x1000] * 8, [0x1000] * 4)
