"""CPU tier: the ragged batch's host arithmetic and argument contract
(include/isal_hip.h "ragged batch"), no GPU.

isal_hip_ragged_items is checked against a model of a few lines; every refusal
of isal_hip_ragged_create runs before the first HIP call, on pointer tables
over fabricated addresses that are never dereferenced.
"""
import ctypes

import numpy as np
import pytest

EINVAL = -1
U8P = ctypes.POINTER(ctypes.c_ubyte)
INTP = ctypes.POINTER(ctypes.c_int)


def model_items(lens, tile):
    """The tiles of stripe 0, then of stripe 1, ...: {stripe, tile index}."""
    return [(s, t) for s, n in enumerate(lens) for t in range((n + tile - 1) // tile)]


LENS = [
    [0, 5, 16, 4096, 4112, 8192 + 55, 1],  # zero first
    [5, 4096, 0, 9000, 1],  # zero in the middle
    [2048, 6000, 0],  # zero last
    [0, 0, 7, 0, 0],  # adjacent zeros
    [3 * 4096, 1],  # an exact multiple of the tile, then one byte
    [2 * 2048, 1],
    [1],
    [4095, 4096, 4097, 2047, 2048, 2049],
]


@pytest.mark.parametrize("tile", [2048, 4096])
@pytest.mark.parametrize("lens", LENS)
def test_ragged_items_match_the_model(engine, lens, tile):
    want = model_items(lens, tile)
    got = engine.ragged_items(lens, tile)
    assert got.shape == (len(want), 2) and got.dtype == np.uint32
    assert [tuple(int(x) for x in row) for row in got] == want
    # the count alone (items = NULL) is the same number
    ln = (ctypes.c_int * len(lens))(*lens)
    assert engine.lib().isal_hip_ragged_items(len(lens), ln, tile, None) == len(want)


def test_ragged_items_all_zero_and_bad_arguments(engine):
    L = engine.lib()
    assert engine.ragged_items([0, 0, 0], 4096).shape == (0, 2)
    assert L.isal_hip_ragged_items(3, (ctypes.c_int * 3)(0, 0, 0), 2048, None) == 0
    neg = (ctypes.c_int * 3)(4096, -1, 7)
    guard = (ctypes.c_uint * 8)(*([0xABCD] * 8))
    assert L.isal_hip_ragged_items(3, neg, 4096, guard) == -1
    assert list(guard) == [0xABCD] * 8, "a refused call wrote items"
    ok = (ctypes.c_int * 2)(1, 2)
    assert L.isal_hip_ragged_items(2, None, 4096, None) == -1
    assert L.isal_hip_ragged_items(0, ok, 4096, None) == -1
    assert L.isal_hip_ragged_items(-2, ok, 4096, None) == -1
    assert L.isal_hip_ragged_items(2, ok, 0, None) == -1
    assert L.isal_hip_ragged_items(2, ok, -4096, None) == -1
    with pytest.raises(ValueError):
        engine.ragged_items([5, -1], 4096)
    # the largest length: 2^31 - 1 bytes in 2 KiB tiles, no overflow
    big = (ctypes.c_int * 2)(2**31 - 1, 2**31 - 1)
    assert L.isal_hip_ragged_items(2, big, 2048, None) == 2 * 2**20


class _Fake:
    """nstripes*per pointers over addresses that are never dereferenced."""

    def __init__(self, per, nstripes, base):
        self.per = per
        self.arr = (U8P * (per * nstripes))()
        for i in range(per * nstripes):
            self.arr[i] = ctypes.cast(ctypes.c_void_p(base + 4096 * i), U8P)

    def set(self, s, i, address):
        self.arr[s * self.per + i] = ctypes.cast(ctypes.c_void_p(address), U8P)
        return self


def _create(engine, k, rows, nstripes, lens, data, coding, tbls=True, out=True):
    g = (ctypes.c_ubyte * (32 * max(1, k) * max(1, rows)))()
    ln = (ctypes.c_int * len(lens))(*lens) if lens is not None else None
    h, bad = ctypes.c_void_p(), ctypes.c_int(-7)
    rc = engine.lib().isal_hip_ragged_create(
        ctypes.byref(h) if out else None, k, rows, ctypes.cast(g, U8P) if tbls else None, nstripes,
        ctypes.cast(ln, INTP) if ln is not None else None, data.arr if data is not None else None,
        coding.arr if coding is not None else None, ctypes.byref(bad))
    assert not h.value, "a failed create returned an object"
    return rc, bad.value


def test_ragged_create_rejects_bad_arguments_without_gpu(engine):
    """Every refusal of the header's table, with the stripe it must name."""
    k, rows, S = 4, 2, 4
    lens = [4096, 0, 100, 7]

    def d():
        return _Fake(k, S, 0x100000)

    def c():
        return _Fake(rows, S, 0x900000)

    # counts and NULL arguments: *bad_stripe = -1
    assert _create(engine, k, rows, S, lens, d(), c(), out=False)[0] == EINVAL
    assert _create(engine, k, rows, S, lens, d(), c(), tbls=False) == (EINVAL, -1)
    assert _create(engine, k, rows, S, None, d(), c()) == (EINVAL, -1)
    assert _create(engine, k, rows, S, lens, None, c()) == (EINVAL, -1)
    assert _create(engine, k, rows, S, lens, d(), None) == (EINVAL, -1)
    assert _create(engine, k, rows, 0, lens, d(), c()) == (EINVAL, -1)
    assert _create(engine, k, rows, -3, lens, d(), c()) == (EINVAL, -1)
    assert _create(engine, 0, rows, S, lens, d(), c()) == (EINVAL, -1)
    assert _create(engine, k, 0, S, lens, d(), c()) == (EINVAL, -1)
    assert _create(engine, 250, 7, 1, [16], _Fake(250, 1, 0x100000), _Fake(7, 1, 0x900000)) == (EINVAL, -1)  # 257
    # a negative length names its stripe, the first one
    assert _create(engine, k, rows, S, [4096, 0, -1, 7], d(), c()) == (EINVAL, 2)
    assert _create(engine, k, rows, S, [4096, -5, -1, 7], d(), c()) == (EINVAL, 1)
    # a NULL or misaligned shard pointer names its stripe, zero-length stripes included
    assert _create(engine, k, rows, S, lens, d().set(2, 3, 0), c()) == (EINVAL, 2)
    assert _create(engine, k, rows, S, lens, d(), c().set(3, 1, 0)) == (EINVAL, 3)
    assert _create(engine, k, rows, S, lens, d().set(0, 0, 0x100008), c()) == (EINVAL, 0)
    assert _create(engine, k, rows, S, lens, d(), c().set(1, 0, 0x900004)) == (EINVAL, 1)  # stripe 1 has length 0
    assert _create(engine, k, rows, S, lens, d().set(1, 2, 0), c()) == (EINVAL, 1)
    # the first offender wins
    assert _create(engine, k, rows, S, [4096, 0, -1, 7], d().set(1, 0, 0), c().set(3, 0, 8)) == (EINVAL, 1)
    L = engine.lib()
    assert L.isal_hip_ragged_encode(None, None) == EINVAL
    assert L.isal_hip_ragged_check(None, None, None) == EINVAL
    assert L.isal_hip_ragged_check(None, ctypes.c_void_p(0x1000), None) == EINVAL
    assert L.isal_hip_ragged_destroy(None) == 0


def test_ragged_create_refuses_more_than_2_30_items_without_gpu(engine):
    """k = rows = 1, stripes of 2^31 - 1 bytes are 2^20 items each at the
    2 KiB tile: 1025 of them are one launch too many. One pointer value
    repeated; the refusal comes before any pointer is classified."""
    n = 2**31 - 1
    S = 2**10 + 1
    u8 = ctypes.cast(ctypes.c_void_p(0x7000000), U8P)
    ptrs = (U8P * S)(*([u8] * S))
    g = (ctypes.c_ubyte * 32)()
    ln = (ctypes.c_int * S)(*([n] * S))
    assert engine.lib().isal_hip_ragged_items(S, ln, 2048, None) == S * 2**20 > 2**30
    h, bad = ctypes.c_void_p(), ctypes.c_int(-7)
    rc = engine.lib().isal_hip_ragged_create(ctypes.byref(h), 1, 1, ctypes.cast(g, U8P), S, ln, ptrs, ptrs,
                                             ctypes.byref(bad))
    assert (rc, bad.value, h.value) == (EINVAL, -1, None)
