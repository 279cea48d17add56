"""CPU tier: the overwrite batch's argument contract (include/isal_hip.h
"overwrite batch"), no GPU. Every refusal below is decided before the first
HIP call, so the codes are the same on a host without a GPU; the pointers are
addresses that are never dereferenced.
"""
import ctypes

import numpy as np

EINVAL = -1
U8P = ctypes.POINTER(ctypes.c_ubyte)
LEN, K, ROWS, NW, S = 4096, 10, 4, 3, 4


class _Fake:
    """A stripe-major pointer table of n entries per stripe over distinct,
    16-byte aligned, non-overlapping addresses 8 KiB apart."""

    def __init__(self, per_stripe, base):
        self.n = per_stripe
        self.arr = (U8P * (per_stripe * S))()
        for i in range(per_stripe * S):
            self.arr[i] = ctypes.cast(ctypes.c_void_p(base + 8192 * i), U8P)

    def address(self, s, i):
        return ctypes.cast(self.arr[s * self.n + i], ctypes.c_void_p).value

    def set(self, s, i, address):
        self.arr[s * self.n + i] = ctypes.cast(ctypes.c_void_p(address), U8P)
        return self


def _tables():
    return _Fake(NW, 0x1000000), _Fake(NW, 0x2000000), _Fake(ROWS, 0x3000000)


def _idx(**changes):
    idx = [(s + 3 * i) % K for s in range(S) for i in range(NW)]
    for at, v in changes.items():
        idx[int(at[1:])] = v
    return idx


def _create(engine, len_=LEN, k=K, rows=ROWS, nw=NW, nstripes=S, idx="good", old="good", new="good",
            coding="good", gftbls="good", out=True, want_bad=True):
    o, n, c = _tables()
    old = o if old == "good" else old
    new = n if new == "good" else new
    coding = c if coding == "good" else coding
    ix = np.array(_idx() if idx == "good" else idx, dtype=np.uint8) if idx is not None else None
    g = np.zeros(32 * K * ROWS, np.uint8) if gftbls == "good" else None
    h, bad = ctypes.c_void_p(0xdead), ctypes.c_int(-7)
    rc = engine.lib().isal_hip_overwrite_create(
        ctypes.byref(h) if out else None, len_, k, rows,
        ctypes.cast(ctypes.c_void_p(g.ctypes.data), U8P) if g is not None else None, nw, nstripes,
        ctypes.cast(ctypes.c_void_p(ix.ctypes.data), U8P) if ix is not None else None,
        old.arr if old is not None else None, new.arr if new is not None else None,
        coding.arr if coding is not None else None, ctypes.byref(bad) if want_bad else None)
    if out and rc != 0:
        assert not h.value, "a failed create returned an object"
    elif out:
        assert h.value and engine.lib().isal_hip_overwrite_destroy(h) == 0
    return rc, bad.value


def test_overwrite_create_rejects_null_arguments_without_gpu(engine):
    assert _create(engine, out=False)[0] == EINVAL
    assert _create(engine, gftbls=None) == (EINVAL, -1)
    assert _create(engine, idx=None) == (EINVAL, -1)
    assert _create(engine, old=None) == (EINVAL, -1)
    assert _create(engine, new=None) == (EINVAL, -1)
    assert _create(engine, coding=None) == (EINVAL, -1)


def test_overwrite_create_rejects_bad_counts_without_gpu(engine):
    assert _create(engine, nw=0) == (EINVAL, -1)
    assert _create(engine, nw=K + 1) == (EINVAL, -1)
    assert _create(engine, len_=-1) == (EINVAL, -1)
    assert _create(engine, nstripes=0) == (EINVAL, -1)
    assert _create(engine, rows=0) == (EINVAL, -1)
    assert _create(engine, k=0) == (EINVAL, -1)


def test_overwrite_create_names_the_first_stripe_with_a_bad_index(engine):
    assert _create(engine, idx=_idx(i7=K)) == (EINVAL, 2)  # index >= k, slot 1 of stripe 2
    assert _create(engine, idx=_idx(i7=255)) == (EINVAL, 2)
    dup = _idx()
    dup[1 * NW + 2] = dup[1 * NW + 0]
    assert _create(engine, idx=dup) == (EINVAL, 1)  # a duplicate within stripe 1
    dup[3 * NW + 1] = K  # a later offender does not change the answer
    assert _create(engine, idx=dup) == (EINVAL, 1)


def test_overwrite_create_names_the_first_stripe_with_a_bad_pointer(engine):
    for which in ("old", "new", "coding"):
        o, n, c = _tables()
        t = {"old": o, "new": n, "coding": c}[which]
        a = t.address(2, 1)
        assert _create(engine, **{which: t.set(2, 1, 0)}) == (EINVAL, 2), which  # NULL
        assert _create(engine, **{which: t.set(2, 1, a + 8)}) == (EINVAL, 2), which  # % 16 != 0
        t.set(2, 1, a)
        assert _create(engine, **{which: t.set(3, 0, a + 8).set(1, 0, 0)}) == (EINVAL, 1), which  # the first one


def test_overwrite_create_rejects_overlapping_ranges_within_a_stripe(engine):
    o, n, c = _tables()
    # new aliases old; new aliases a parity row; two parity rows; old of two slots
    assert _create(engine, new=_tables()[1].set(1, 2, o.address(1, 2))) == (EINVAL, 1)
    assert _create(engine, new=_tables()[1].set(3, 0, c.address(3, 3))) == (EINVAL, 3)
    assert _create(engine, coding=_tables()[2].set(0, 1, c.address(0, 2))) == (EINVAL, 0)
    assert _create(engine, old=_tables()[0].set(2, 0, o.address(2, 1))) == (EINVAL, 2)
    # a partial overlap: a parity row that starts in the last 16 bytes of an old range
    part = _tables()[2].set(2, 0, o.address(2, 1) + LEN - 16)
    assert _create(engine, coding=part) == (EINVAL, 2)
    # ... and one that starts in the last 16 bytes before a new range
    part = _tables()[2].set(1, 3, n.address(1, 0) - 16)
    assert _create(engine, coding=part) == (EINVAL, 1)


def test_overwrite_create_passes_the_checks_where_nothing_overlaps(engine):
    """Whatever a create with a sound argument set returns on this host (0 with
    a GPU, a HIP or pointer-kind code without), it is not a refusal that names
    a stripe: ranges that touch, a shard shared by two stripes and equal
    pointers at len 0 are no overlap."""
    o, n, c = _tables()
    assert _create(engine, len_=0, new=_tables()[1].set(1, 2, o.address(1, 2)))[1] == -1
    assert _create(engine, coding=_tables()[2].set(2, 0, o.address(2, 1) + LEN))[1] == -1  # touching
    assert _create(engine, coding=_tables()[2].set(2, 0, c.address(1, 0)))[1] == -1  # stripe 1's row in stripe 2
    assert _create(engine, nw=K, idx=[(s + i) % K for s in range(S) for i in range(K)],
                   old=_Fake(K, 0x4000000), new=_Fake(K, 0x5000000))[1] == -1  # nw = k
    assert _create(engine, idx=[i for _ in range(S) for i in range(NW)])[1] == -1  # one index set in every stripe


def test_overwrite_bad_stripe_is_optional(engine):
    assert _create(engine, idx=_idx(i7=K), want_bad=False)[0] == EINVAL


def test_overwrite_run_and_destroy_reject_null_and_unknown_flags(engine):
    L = engine.lib()
    assert L.isal_hip_overwrite_run(None, 0, None) == EINVAL
    assert L.isal_hip_overwrite_run(None, engine.OVERWRITE_COMMIT, None) == EINVAL
    for flags in (2, 3, 0x100, -1, -2):
        assert L.isal_hip_overwrite_run(None, flags, None) == EINVAL
    assert L.isal_hip_overwrite_destroy(None) == 0
    assert engine.OVERWRITE_COMMIT == 1
