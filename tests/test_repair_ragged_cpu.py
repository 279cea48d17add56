"""CPU tier: the ragged repair's argument contract (include/isal_hip.h
"Ragged repair"), no GPU.

Every refusal of isal_hip_repair_create_ragged runs before the first HIP call,
on pointer tables over fabricated addresses that are never dereferenced, so
each one is checked here with the stripe it must name.
"""
import ctypes
import random

import numpy as np

import ecutil

EINVAL, ENOMEM, ESINGULAR = -1, -3, -5
SINGULAR_RS_20_28 = (0, 13, 17, 18, 21, 23)  # test_repair_cpu.py's pattern
U8P = ctypes.POINTER(ctypes.c_ubyte)
INTP = ctypes.POINTER(ctypes.c_int)


class _Fake:
    """nstripes*m shard pointers over addresses that are never dereferenced."""

    def __init__(self, m, nstripes):
        self.m = m
        self.arr = (U8P * (m * nstripes))()
        for i in range(m * nstripes):
            self.arr[i] = ctypes.cast(ctypes.c_void_p(0x10000 + 4096 * i), U8P)

    def set(self, s, i, address):
        self.arr[s * self.m + i] = ctypes.cast(ctypes.c_void_p(address), U8P)
        return self


def _u8(x):
    x = np.ascontiguousarray(x, dtype=np.uint8)
    return x, ctypes.cast(ctypes.c_void_p(x.ctypes.data), U8P)


def _create(engine, a, k, m, nstripes, lens, max_errs, nerrs, errs, shards, out=True):
    """errs: the flat nstripes*max_errs table, exactly as the C caller passes it."""
    keep = [_u8(a) if a is not None else None, _u8(nerrs) if nerrs is not None else None,
            _u8(errs) if errs is not None else None]
    ap, np_, ep = [x[1] if x is not None else None for x in keep]
    ln = (ctypes.c_int * len(lens))(*lens) if lens is not None else None
    h, bad = ctypes.c_void_p(), ctypes.c_int(-7)
    rc = engine.lib().isal_hip_repair_create_ragged(
        ctypes.byref(h) if out else None, k, m, ap, nstripes, ctypes.cast(ln, INTP) if ln is not None else None,
        max_errs, np_, ep, shards.arr if shards is not None else None, ctypes.byref(bad))
    assert not h.value, "a failed create returned an object"
    return rc, bad.value


def test_engine_binds_the_ragged_repair(engine):
    assert hasattr(engine.lib(), "isal_hip_repair_create_ragged")
    assert callable(engine.Repair.ragged)


def test_ragged_repair_geometry_refusals_name_no_stripe(engine, oracle):
    k, m, S, E = 4, 6, 3, 2
    a = oracle.gf_gen_rs_matrix(m, k)
    lens, nerrs, errs = [4096, 0, 100], [2, 1, 0], [0, 1, 5, 0, 0, 0]

    def f():
        return _Fake(m, S)

    assert _create(engine, a, k, m, S, lens, E, nerrs, errs, f(), out=False)[0] == EINVAL  # NULL out
    assert _create(engine, None, k, m, S, lens, E, nerrs, errs, f()) == (EINVAL, -1)
    assert _create(engine, a, k, m, S, None, E, nerrs, errs, f()) == (EINVAL, -1)
    assert _create(engine, a, k, m, S, lens, E, None, errs, f()) == (EINVAL, -1)
    assert _create(engine, a, k, m, S, lens, E, nerrs, None, f()) == (EINVAL, -1)
    assert _create(engine, a, k, m, S, lens, E, nerrs, errs, None) == (EINVAL, -1)
    assert _create(engine, a, k, m, 0, lens, E, nerrs, errs, f()) == (EINVAL, -1)
    assert _create(engine, a, k, m, -2, lens, E, nerrs, errs, f()) == (EINVAL, -1)
    assert _create(engine, a, 0, m, S, lens, E, nerrs, errs, f()) == (EINVAL, -1)  # k < 1
    assert _create(engine, a, k, k, S, lens, E, nerrs, errs, f()) == (EINVAL, -1)  # m <= k
    assert _create(engine, a, k, 257, S, lens, E, nerrs, errs, _Fake(257, S)) == (EINVAL, -1)  # m > 256
    assert _create(engine, a, k, m, S, lens, 0, nerrs, errs, f()) == (EINVAL, -1)  # max_errs < 1
    assert _create(engine, a, k, m, S, lens, 3, [2, 1, 0], [0, 1, 0, 5, 0, 0, 0, 0, 0], f()) == (EINVAL, -1)  # > m - k


def test_ragged_repair_stripe_refusals_name_the_first_stripe(engine, oracle):
    k, m, S, E = 4, 6, 4, 2
    a = oracle.gf_gen_rs_matrix(m, k)
    lens = [4096, 0, 100, 7]
    nerrs = [2, 1, 0, 2]
    errs = [0, 5, 3, 0, 0, 0, 4, 1]

    def f():
        return _Fake(m, S)

    def with_(seq, at, v):
        out = list(seq)
        out[at] = v
        return out

    # nerrs[s] > max_errs
    assert _create(engine, a, k, m, S, lens, E, with_(nerrs, 2, 3), errs, f()) == (EINVAL, 2)
    assert _create(engine, a, k, m, S, lens, E, with_(nerrs, 1, 255), errs, f()) == (EINVAL, 1)
    # a negative length
    assert _create(engine, a, k, m, S, with_(lens, 3, -1), E, nerrs, errs, f()) == (EINVAL, 3)
    assert _create(engine, a, k, m, S, [4096, -5, -1, 7], E, nerrs, errs, f()) == (EINVAL, 1)
    # an index out of range, a duplicate; stripe 1 has length 0 and is still held to it
    assert _create(engine, a, k, m, S, lens, E, nerrs, with_(errs, 7, 6), f()) == (EINVAL, 3)
    assert _create(engine, a, k, m, S, lens, E, nerrs, with_(errs, 1, 0), f()) == (EINVAL, 0)
    assert _create(engine, a, k, m, S, lens, E, nerrs, with_(errs, 2, 6), f()) == (EINVAL, 1)
    # a NULL or misaligned shard; stripe 2 lost nothing and stripe 1 is empty
    assert _create(engine, a, k, m, S, lens, E, nerrs, errs, f().set(2, 3, 0)) == (EINVAL, 2)
    assert _create(engine, a, k, m, S, lens, E, nerrs, errs, f().set(1, 0, 0x20008)) == (EINVAL, 1)
    assert _create(engine, a, k, m, S, lens, E, nerrs, errs, f().set(3, 5, 0x20004)) == (EINVAL, 3)
    # the first offender wins
    assert _create(engine, a, k, m, S, with_(lens, 3, -1), E, with_(nerrs, 1, 3), errs, f().set(2, 0, 0)) == (EINVAL, 1)


def test_ragged_repair_ignores_the_tail_of_an_errs_row(engine, oracle):
    """A duplicate, or an index out of range, past nerrs[s] is no error: what
    answers then is the next check, the singular stripe 3."""
    k, m, S, E = 20, 28, 4, 6
    a = oracle.gf_gen_rs_matrix(m, k)
    lens = [4096, 17, 0, 4096]
    nerrs = [2, 1, 0, 6]
    errs = [3, 9, 3, 3, 9, 9,  # the tail repeats the row's own indices
            27, 27, 27, 200, 255, 27,  # ... and holds indices >= m
            5, 5, 5, 5, 5, 5] + list(SINGULAR_RS_20_28)
    assert _create(engine, a, k, m, S, lens, E, nerrs, errs, _Fake(m, S)) == (ESINGULAR, 3)
    # the same duplicate inside the counted part is refused
    assert _create(engine, a, k, m, S, lens, E, [3, 1, 0, 6], errs, _Fake(m, S)) == (EINVAL, 0)


def test_ragged_repair_names_the_first_singular_stripe(engine, oracle):
    k, m, S, E = 20, 28, 8, 7
    a = oracle.gf_gen_rs_matrix(m, k)
    rng = random.Random(5)
    nerrs, errs = [], []
    for s in range(S):
        if s in (5, 7):
            pat = list(SINGULAR_RS_20_28)
        else:
            pat = [1, 13, 17, 18, 21, 23 + (s % 4)][:(s % 6) + 1]
        assert (ecutil.decode_matrix(a, k, pat, oracle)[0] != 0) == (s in (5, 7))
        rng.shuffle(pat)
        nerrs.append(len(pat))
        errs += pat + [0] * (E - len(pat))
    # stripe 5 has length 0: its pattern is checked all the same
    lens = [8192, 1, 0, 4097, 16, 0, 5, 8192]
    assert _create(engine, a, k, m, S, lens, E, nerrs, errs, _Fake(m, S)) == (ESINGULAR, 5)


def test_ragged_repair_refuses_tables_past_the_limit(engine, oracle):
    """k = 16 of m = 256 with 240 and 239 erasures: 76800 and 76480 bytes of
    tables per pattern, so the 64 MiB of ISAL_HIP_REPAIR_MAX_TABLE_BYTES end
    before the 900 distinct patterns do. Neither count alone reaches the
    limit: the tables of all counts are summed."""
    k, m, S = 16, 256, 900
    E = m - k
    a = oracle.gf_gen_cauchy1_matrix(m, k)
    rng = random.Random(16)
    seen, nerrs, errs = set(), [], []
    for s in range(S):
        c = E - (s & 1)
        pat = tuple(sorted(rng.sample(range(m), c)))
        assert pat not in seen
        seen.add(pat)
        nerrs.append(c)
        errs += list(pat) + [0] * (E - c)
    per = [20 * k * E, 20 * k * (E - 1)]
    assert (S // 2) * per[0] < 64 << 20 and (S // 2) * per[1] < 64 << 20 < (S // 2) * (per[0] + per[1])
    assert _create(engine, a, k, m, S, [4096] * S, E, nerrs, errs, _Fake(m, S)) == (ENOMEM, -1)


def test_ragged_repair_refuses_more_than_2_30_items_in_one_class(engine, oracle):
    """As test_ragged_cpu.py: stripes of 2^31 - 1 bytes are 2^20 items each at
    the 2 KiB tile of a one-erasure class; 1025 of them are one launch too
    many. A three-erasure class runs on 4 KiB tiles only, 2^19 items per
    stripe, so it takes 2049. One pointer value repeated; the refusal comes
    before any pointer is classified."""
    k, m, n = 4, 8, 2**31 - 1
    a = oracle.gf_gen_cauchy1_matrix(m, k)
    u8 = ctypes.cast(ctypes.c_void_p(0x7000000), U8P)
    for count, S in ((1, 2**10 + 1), (3, 2**11 + 1)):
        tile = 2048 if count == 1 else 4096
        ln = (ctypes.c_int * S)(*([n] * S))
        assert engine.lib().isal_hip_ragged_items(S, ln, tile, None) > 2**30
        ptrs = (U8P * (S * m))(*([u8] * (S * m)))
        lens = [n] * S
        ne, keep_n = _u8([count] * S)
        er, keep_e = _u8([0, 5, 6] * S)
        aa, keep_a = _u8(a)
        h, bad = ctypes.c_void_p(), ctypes.c_int(-7)
        rc = engine.lib().isal_hip_repair_create_ragged(ctypes.byref(h), k, m, keep_a, S, (ctypes.c_int * S)(*lens), 3,
                                                        keep_n, keep_e, ptrs, ctypes.byref(bad))
        assert (rc, bad.value, h.value) == (EINVAL, -1, None), count
