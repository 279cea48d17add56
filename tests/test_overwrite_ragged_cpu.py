"""CPU tier: the ragged overwrite's argument contract (include/isal_hip.h
"Ragged overwrite"), no GPU. Every refusal below is decided before the first
HIP call, so the codes are the same on a host without a GPU; the pointers are
addresses that are never dereferenced.

A table row holds MAX_NW slots; stripe s uses the first NW[s] of them. The
tables of _create() fill the unused slots with what must be ignored: index
255, NULL and unaligned pointers.
"""
import ctypes

import numpy as np
import pytest

EINVAL = -1
INT_MAX = 2**31 - 1
U8P = ctypes.POINTER(ctypes.c_ubyte)
INTP = ctypes.POINTER(ctypes.c_int)
K, ROWS, MAX_NW, S = 10, 4, 3, 5
LENS = [4096, 100, 0, 4096, 17]
NW = [3, 1, 2, 0, 2]  # stripe 2 has no byte, stripe 3 no slot
GAP = 8192


class _Fake:
    """A stripe-major pointer table of n entries per stripe over distinct,
    16-byte aligned addresses `gap` bytes apart."""

    def __init__(self, per_stripe, base, nstripes=S, gap=GAP):
        self.n = per_stripe
        self.arr = (U8P * (per_stripe * nstripes))()
        for i in range(per_stripe * nstripes):
            self.arr[i] = ctypes.cast(ctypes.c_void_p(base + gap * i), U8P)

    def address(self, s, i):
        return ctypes.cast(self.arr[s * self.n + i], ctypes.c_void_p).value

    def set(self, s, i, address):
        self.arr[s * self.n + i] = ctypes.cast(ctypes.c_void_p(address), U8P)
        return self


def _tables(nw=NW):
    """old, new and coding; the slots from nw[s] on hold NULL (old) and an
    unaligned address (new)."""
    o, n, c = _Fake(MAX_NW, 0x1000000), _Fake(MAX_NW, 0x2000000), _Fake(ROWS, 0x3000000)
    for s in range(S):
        for i in range(nw[s], MAX_NW):
            o.set(s, i, 0)
            n.set(s, i, 0x2000000 + 7)
    return o, n, c


def _idx(nw=NW, **changes):
    idx = [(s + 3 * i) % K if i < nw[s] else 255 for s in range(S) for i in range(MAX_NW)]
    for at, v in changes.items():
        idx[int(at[1:])] = v
    return idx


def _call(engine, out, k, rows, g, nstripes, lens, max_nw, nw, ix, old, new, coding, want_bad=True):
    ln = np.array(lens, dtype=np.intc) if lens is not None else None
    nn = np.array(nw, dtype=np.intc) if nw is not None else None
    ix = np.array(ix, dtype=np.uint8) if ix is not None else None
    h, bad = ctypes.c_void_p(0xdead), ctypes.c_int(-7)
    rc = engine.lib().isal_hip_overwrite_create_ragged(
        ctypes.byref(h) if out else None, k, rows,
        ctypes.cast(ctypes.c_void_p(g.ctypes.data), U8P) if g is not None else None, nstripes,
        ln.ctypes.data_as(INTP) if ln is not None else None, max_nw,
        nn.ctypes.data_as(INTP) if nn is not None else None,
        ctypes.cast(ctypes.c_void_p(ix.ctypes.data), U8P) if ix is not None else None,
        old.arr if old is not None else None, new.arr if new is not None else None,
        coding.arr if coding is not None else None, ctypes.byref(bad) if want_bad else None)
    if out and rc != 0:
        assert not h.value, "a failed create returned an object"
    elif out:
        assert h.value and engine.lib().isal_hip_overwrite_destroy(h) == 0
    return rc, bad.value


def _create(engine, k=K, rows=ROWS, max_nw=MAX_NW, nstripes=S, lens="good", nw="good", idx="good", old="good",
            new="good", coding="good", gftbls="good", out=True, want_bad=True):
    counts = NW if nw == "good" or nw is None else [min(max(c, 0), MAX_NW) for c in nw]
    o, n, c = _tables(counts)
    return _call(engine, out, k, rows, np.zeros(32 * K * ROWS, np.uint8) if gftbls == "good" else None, nstripes,
                 LENS if lens == "good" else lens, max_nw, NW if nw == "good" else nw,
                 _idx(counts) if idx == "good" else idx, o if old == "good" else old, n if new == "good" else new,
                 c if coding == "good" else coding, want_bad)


def test_ragged_overwrite_create_rejects_null_arguments_without_gpu(engine):
    assert _create(engine, out=False)[0] == EINVAL
    for name in ("gftbls", "lens", "nw", "idx", "old", "new", "coding"):
        assert _create(engine, **{name: None}) == (EINVAL, -1), name


def test_ragged_overwrite_create_rejects_bad_counts_without_gpu(engine):
    assert _create(engine, nstripes=0) == (EINVAL, -1)
    assert _create(engine, nstripes=-1) == (EINVAL, -1)
    assert _create(engine, k=0) == (EINVAL, -1)
    assert _create(engine, k=257) == (EINVAL, -1)
    assert _create(engine, rows=0) == (EINVAL, -1)
    assert _create(engine, max_nw=0) == (EINVAL, -1)
    assert _create(engine, max_nw=K + 1) == (EINVAL, -1)
    assert _create(engine, k=2) == (EINVAL, -1)  # max_nw = 3 > k


def test_ragged_overwrite_create_names_the_first_stripe_with_a_bad_length_or_count(engine):
    assert _create(engine, lens=[4096, 100, -1, 4096, 17]) == (EINVAL, 2)
    assert _create(engine, lens=[4096, 100, 0, -5, -1]) == (EINVAL, 3)
    assert _create(engine, nw=[3, 1, 2, 0, -1]) == (EINVAL, 4)
    assert _create(engine, nw=[3, MAX_NW + 1, 2, 0, 2]) == (EINVAL, 1)
    assert _create(engine, nw=[3, 1, 2, 0, 2], lens=[4096, 100, 0, 4096, -17]) == (EINVAL, 4)
    # the first offender wins, whatever its kind
    assert _create(engine, nw=[3, 1, 2, -2, MAX_NW + 1], lens=[4096, -100, 0, 4096, 17]) == (EINVAL, 1)


def test_ragged_overwrite_create_names_the_first_stripe_with_a_bad_index(engine):
    at = 4 * MAX_NW + 1  # slot 1 of stripe 4, live
    assert _create(engine, idx=_idx(**{f"i{at}": K})) == (EINVAL, 4)
    assert _create(engine, idx=_idx(**{f"i{at}": 255})) == (EINVAL, 4)
    dup = _idx()
    dup[0 * MAX_NW + 2] = dup[0 * MAX_NW + 0]
    assert _create(engine, idx=dup) == (EINVAL, 0)  # a duplicate within stripe 0
    dup = _idx()
    dup[2 * MAX_NW + 1] = dup[2 * MAX_NW + 0]  # a stripe of zero length is still checked
    dup[at] = K  # a later offender does not change the answer
    assert _create(engine, idx=dup) == (EINVAL, 2)
    # stripes are checked in order: an earlier stripe's bad pointer wins over a later bad index
    o, n, c = _tables()
    assert _create(engine, idx=_idx(**{f"i{at}": K}), coding=c.set(1, 0, 0)) == (EINVAL, 1)


def test_ragged_overwrite_padded_slots_are_ignored(engine):
    """Index 255, NULL and unaligned pointers past nw[s] (what _tables and _idx
    put there) are not refused, and neither is a duplicate of a live index."""
    assert _create(engine)[1] == -1
    idx = _idx()
    idx[1 * MAX_NW + 1] = idx[1 * MAX_NW + 0]  # stripe 1 uses one slot
    idx[3 * MAX_NW + 0] = K  # stripe 3 uses none
    o, n, c = _tables()
    o.set(1, 2, c.address(1, 0))  # a padded pointer that aliases a live one
    n.set(3, 0, 8)
    assert _create(engine, idx=idx, old=o, new=n)[1] == -1


def test_ragged_overwrite_create_names_the_first_stripe_with_a_bad_pointer(engine):
    for which, i in (("old", 0), ("new", 1), ("coding", 3)):
        o, n, c = _tables()
        t = {"old": o, "new": n, "coding": c}[which]
        a = t.address(4, i)
        assert _create(engine, **{which: t.set(4, i, 0)}) == (EINVAL, 4), which  # NULL
        assert _create(engine, **{which: t.set(4, i, a + 8)}) == (EINVAL, 4), which  # % 16 != 0
        assert _create(engine, **{which: t.set(0, 0, 0)}) == (EINVAL, 0), which  # the first one


def test_ragged_overwrite_bad_pointers_of_empty_stripes_are_still_refused(engine):
    """Stripe 2 has length 0 and two slots, stripe 3 has a length and no slot:
    their live pointers (2*nw[s] + rows) are checked like any other."""
    o, n, c = _tables()
    assert _create(engine, old=o.set(2, 1, 0)) == (EINVAL, 2)
    o, n, c = _tables()
    assert _create(engine, new=n.set(2, 0, n.address(2, 0) + 4)) == (EINVAL, 2)
    o, n, c = _tables()
    assert _create(engine, coding=c.set(2, 3, 0)) == (EINVAL, 2)
    o, n, c = _tables()
    assert _create(engine, coding=c.set(3, 1, c.address(3, 1) + 1)) == (EINVAL, 3)
    # ... but stripe 3's slots are all padding
    o, n, c = _tables()
    assert _create(engine, old=o.set(3, 0, 4), new=n.set(3, 2, 0))[1] == -1


def test_ragged_overwrite_create_rejects_overlapping_ranges_within_a_stripe(engine):
    o, n, c = _tables()
    # new aliases old; new aliases a parity row; two parity rows; old of two slots
    assert _create(engine, new=_tables()[1].set(0, 2, o.address(0, 2))) == (EINVAL, 0)
    assert _create(engine, new=_tables()[1].set(4, 0, c.address(4, 3))) == (EINVAL, 4)
    assert _create(engine, coding=_tables()[2].set(3, 1, c.address(3, 2))) == (EINVAL, 3)  # no slot, a length
    assert _create(engine, old=_tables()[0].set(0, 0, o.address(0, 1))) == (EINVAL, 0)
    # a partial overlap over the stripe's own length: 100 bytes in stripe 1, 17 in stripe 4
    assert _create(engine, coding=_tables()[2].set(1, 0, o.address(1, 0) + 96)) == (EINVAL, 1)
    assert _create(engine, coding=_tables()[2].set(4, 2, n.address(4, 1) - 16)) == (EINVAL, 4)
    # touching ranges pass: 100 bytes end before +112, 17 before +32
    assert _create(engine, coding=_tables()[2].set(1, 0, o.address(1, 0) + 112))[1] == -1
    assert _create(engine, coding=_tables()[2].set(4, 2, n.address(4, 1) - 32))[1] == -1
    # equal pointers at length 0 pass; a shard shared by two stripes is no overlap
    assert _create(engine, new=_tables()[1].set(2, 1, o.address(2, 1)))[1] == -1
    assert _create(engine, coding=_tables()[2].set(4, 0, c.address(0, 0)))[1] == -1


def test_ragged_overwrite_overlap_is_measured_over_the_stripes_own_length(engine):
    """Two ranges 4096 bytes apart: refused in a stripe of 8192 bytes, accepted
    in the same table with that stripe at 4096 bytes."""
    o, n, c = _tables()
    c.set(0, 1, o.address(0, 1) + 4096)
    assert _create(engine, lens=[8192, 100, 0, 4096, 17], coding=c) == (EINVAL, 0)
    assert _create(engine, lens=[4096, 100, 0, 4096, 17], coding=c)[1] == -1
    # the same distance in a later stripe, with the first one sound
    o, n, c = _tables()
    c.set(3, 0, c.address(3, 1) - 4096)
    assert _create(engine, lens=[4096, 100, 0, 4097, 17], coding=c) == (EINVAL, 3)
    assert _create(engine, lens=[8192, 100, 0, 4096, 17], coding=c)[1] == -1


def test_ragged_overwrite_item_limit_is_refused_before_anything_is_allocated(engine):
    """More than 2^30 items at the 2 KiB tile: 1025 stripes of INT_MAX bytes
    (2^20 tiles each). Stripes may share shards, so one row of addresses 4 GiB
    apart serves every stripe; 1024 such stripes are exactly the limit."""
    n = 1025
    per = INT_MAX // 2048 + 1
    assert per == 2**20 and 1024 * per == 2**30 < n * per
    gap = 1 << 32
    o, nn, c = _Fake(1, 0x10000000000, 1, gap), _Fake(1, 0x20000000000, 1, gap), _Fake(ROWS, 0x30000000000, 1, gap)
    old, new, coding = _Fake(1, 0, n), _Fake(1, 0, n), _Fake(ROWS, 0, n)
    for s in range(n):
        old.set(s, 0, o.address(0, 0))
        new.set(s, 0, nn.address(0, 0))
        for l in range(ROWS):
            coding.set(s, l, c.address(0, l))
    g = np.zeros(32 * K * ROWS, np.uint8)
    args = (engine, True, K, ROWS, g, n, [INT_MAX] * n, 1, [1] * n, [s % K for s in range(n)], old, new, coding)
    assert _call(*args) == (EINVAL, -1)
    # a stripe without a slot has no items: the same window with one count at 0 is within the limit
    nw = [1] * n
    nw[7] = 0
    rc, bad = _call(engine, True, K, ROWS, g, n, [INT_MAX] * n, 1, nw, [s % K for s in range(n)], old, new, coding)
    assert bad == -1  # whatever this host answers about the (fake) memory, no stripe is named
    # a bad stripe is named before the limit is looked at
    lens = [INT_MAX] * n
    lens[1000] = -1
    assert _call(engine, True, K, ROWS, g, n, lens, 1, [1] * n, [s % K for s in range(n)], old, new,
                 coding) == (EINVAL, 1000)


def test_ragged_overwrite_bad_stripe_is_optional(engine):
    assert _create(engine, lens=[4096, 100, -1, 4096, 17], want_bad=False)[0] == EINVAL
    at = 4 * MAX_NW + 1
    assert _create(engine, idx=_idx(**{f"i{at}": K}), want_bad=False)[0] == EINVAL


def test_ragged_overwrite_accepts_a_whole_stripe_of_256_shards(engine):
    """nw = k = 256 passes validation: the counts are ints because 256 does not
    fit a byte. One stripe of 256 slots, one of none."""
    k = 256
    old, new, coding = _Fake(k, 0x4000000, 2), _Fake(k, 0x8000000, 2), _Fake(ROWS, 0xc000000, 2)
    g = np.zeros(32 * k * ROWS, np.uint8)
    idx = [(i * 7) % k for i in range(k)] + [255] * k
    assert len(set(idx[:k])) == k
    rc, bad = _call(engine, True, k, ROWS, g, 2, [4096, 4096], k, [k, 0], idx, old, new, coding)
    assert bad == -1
    idx[5] = idx[200]
    assert _call(engine, True, k, ROWS, g, 2, [4096, 4096], k, [k, 0], idx, old, new, coding) == (EINVAL, 0)


def test_ragged_overwrite_python_wrapper_pads_to_the_stride(engine):
    """Overwrite.ragged checks its sequences before the library is asked."""
    g = np.zeros(32 * K * ROWS, np.uint8)
    with pytest.raises(ValueError):
        engine.Overwrite.ragged(K, ROWS, g, [16, 16], [[1]], [[16]], [[32]], [48] * (2 * ROWS))
    with pytest.raises(ValueError):
        engine.Overwrite.ragged(K, ROWS, g, [16], [[1, 2]], [[16]], [[32, 64]], [48] * ROWS)
    with pytest.raises(ValueError):
        engine.Overwrite.ragged(K, ROWS, g, [16], [[1, 2]], [[16, 32]], [[64, 80]], [48] * ROWS, max_nw=1)
    # a refusal names the stripe: stripe 1 repeats an index; stripe 0's row is padded
    with pytest.raises(RuntimeError, match=r"\(-1, stripe 1\)"):
        engine.Overwrite.ragged(K, ROWS, g, [16, 16], [[1], [2, 2]], [[0x1000], [0x2000, 0x3000]],
                                [[0x4000], [0x5000, 0x6000]], [0x10000 + 64 * i for i in range(2 * ROWS)])
