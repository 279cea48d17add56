"""GPU tier: the ragged batch (include/isal_hip.h) — stripes of different shard
lengths encoded and checked by one launch per pass.

The checker is oracle.ec_encode_data per stripe with that stripe's own length,
never the engine's own output. Every stripe of a case lies in one device
allocation, each shard followed by at least 64 guard bytes, the parity
pre-filled with a poison byte; after every run the whole allocation is
compared with the host image, so a store bounded by another stripe's length
shows up as a written guard and a missing one as surviving poison.

Sizes: passes of 1-2 rows encode 2 KiB tiles (128 lanes of 16 bytes), every
other pass and the check 4 KiB tiles. For a tile T the lengths are 0, a byte
tail alone, one vector, a whole tile, a tile and a vector, two tiles with
three vectors and a 7-byte tail, and one byte: 7 stripes are 9 work items (not
a multiple of 8: items run in table order), 16 stripes 24 (a multiple of 8: the
XCD-contiguous order permutes them).
"""
import functools
import random

import numpy as np
import pytest
import torch

import ecutil
from test_scrub_cpu import matrix

pytestmark = pytest.mark.gpu

POISON, GUARD, GUARD_BYTES = 0xA5, 0x3C, 64
GARBAGE = 0x5A5A5A5A5A5A5A5A
CLEAN = 0xFFFFFFFFFFFFFFFF


def lens7(T):
    return [0, 5, 16, T, T + 16, 2 * T + 3 * 16 + 7, 1]


def lens16(T):
    return lens7(T) + lens7(T) + [3 * T, 2 * T + 1]


def shuffled(lens, seed):
    out = list(lens)
    random.Random(seed).shuffle(out)
    return out


def _tile_before_one(lens, T):
    return any(a == T and b == 1 for a, b in zip(lens, lens[1:]))


def _adjacent_zeros(lens):
    return any(a == 0 and b == 0 for a, b in zip(lens, lens[1:]))


def orders(T):
    """The fixed-seed shuffles of the cases, with what each is there for."""
    out = [shuffled(lens7(T), 3), shuffled(lens7(T), 14), shuffled(lens7(T), 1),
           shuffled(lens16(T), 5), shuffled(lens16(T), 69), shuffled(lens16(T), 3)]
    assert out[0][0] == 0 and out[1][-1] == 0 and _tile_before_one(out[2], T)
    assert _adjacent_zeros(out[3]) and out[4][0] == 0 and _tile_before_one(out[4], T) and out[5][-1] == 0
    for o in out:
        n = sum((x + T - 1) // T for x in o)
        assert (n % 8 == 0) == (len(o) == 16), (len(o), n)
    return out


@functools.lru_cache(maxsize=None)
def _reference(kind, k, rows, lens, seed):
    """Host images of a case, computed once and never written: the shard
    offsets, the image with the oracle's parity and the one with poison."""
    oracle = ecutil.oracle()
    coef = matrix(oracle, kind, k, rows)
    tbls = oracle.ec_init_tables(k, rows, coef)
    m = k + rows
    off, at = [], 0
    for n in lens:
        span = (n + GUARD_BYTES + 15) // 16 * 16
        off.append([at + i * span for i in range(m)])
        at += m * span
    want = np.full(at, GUARD, np.uint8)
    for s, n in enumerate(lens):
        if not n:
            continue
        data = [ecutil.fill_bytes(n, seed * 100000 + s * k + j) for j in range(k)]
        parity = [np.zeros(n, np.uint8) for _ in range(rows)]
        oracle.ec_encode_data(n, k, rows, tbls, data, parity)
        for i, sh in enumerate(data + parity):
            want[off[s][i]:off[s][i] + n] = sh
    poisoned = want.copy()
    for s, n in enumerate(lens):
        for l in range(rows):
            poisoned[off[s][k + l]:off[s][k + l] + n] = POISON
    for a in (want, poisoned, tbls, coef):
        a.setflags(write=False)
    return off, want, poisoned, tbls, coef


class Stripes:
    """The stripes of one case in one device allocation. `image` is what the
    device must hold (flip() changes both)."""

    def __init__(self, gpu, kind, k, rows, lens, seed, encoded=False):
        self.k, self.rows, self.m, self.lens, self.S = k, rows, k + rows, list(lens), len(lens)
        self.off, self.want, self.poisoned, self.tbls, self.coef = _reference(kind, k, rows, tuple(lens), seed)
        self.image = (self.want if encoded else self.poisoned).copy()
        self.dev = torch.from_numpy(self.image.copy()).to(gpu)
        base = int(self.dev.data_ptr())
        assert base % 16 == 0
        self.data = [base + self.off[s][j] for s in range(self.S) for j in range(k)]
        self.coding = [base + self.off[s][k + l] for s in range(self.S) for l in range(rows)]

    def where(self, pos):
        for s in range(self.S):
            for i in range(self.m):
                o = self.off[s][i]
                end = self.off[s][i + 1] if i + 1 < self.m else (self.off[s + 1][0] if s + 1 < self.S else len(self.image))
                if o <= pos < end:
                    what = "guard" if pos >= o + self.lens[s] else "bytes"
                    return f"stripe {s} (len {self.lens[s]}) shard {i} {what} at +{pos - o}"
        return f"byte {pos}"

    def same(self, what, want=None):
        want = self.image if want is None else want
        got = self.dev.cpu().numpy()
        if not np.array_equal(got, want):
            pos = int(np.nonzero(got != want)[0][0])
            raise AssertionError(f"{what}: {self.where(pos)}: got {got[pos]:#x}, want {want[pos]:#x}")
        return got

    def flip(self, s, shard, col, x=0x40):
        assert 0 <= col < self.lens[s] and x
        self.image[self.off[s][shard] + col] ^= x
        self.dev[self.off[s][shard] + col] ^= x

    def restore(self):
        self.image = self.want.copy()
        self.dev.copy_(torch.from_numpy(self.image.copy()))
        torch.cuda.synchronize()

    def model_bad(self, oracle):
        """Per stripe: ~0, or the first mismatch of the stored parity against
        the oracle's parity of the stored sources, column << 8 | row."""
        out = []
        for s, n in enumerate(self.lens):
            if not n:
                out.append(CLEAN)
                continue
            sh = [self.image[self.off[s][i]:self.off[s][i] + n].copy() for i in range(self.m)]
            true = [np.zeros(n, np.uint8) for _ in range(self.rows)]
            oracle.ec_encode_data(n, self.k, self.rows, self.tbls, sh[:self.k], true)
            diff = np.stack([t != p for t, p in zip(true, sh[self.k:])])  # (rows, n)
            cols = np.nonzero(diff.any(axis=0))[0]
            if not cols.size:
                out.append(CLEAN)
                continue
            col = int(cols[0])
            out.append(col << 8 | int(np.nonzero(diff[:, col])[0][0]))
        return out


def _passes(rows):
    return (rows + 7) // 8


def _encode(engine, st, rg, what, launches=None):
    torch.cuda.synchronize()
    before = engine.kernel_launches()
    rg.encode(0)
    torch.cuda.synchronize()
    assert engine.kernel_launches() - before == (_passes(st.rows) if launches is None else launches)
    return st.same(what, st.want)


def _check(engine, st, rg, launches=None, stream=0):
    """One check over garbage-filled words: the launch count, nothing written."""
    bad = torch.full((st.S,), GARBAGE, dtype=torch.int64, device=st.dev.device)
    torch.cuda.synchronize()
    before = engine.kernel_launches()
    rg.check(bad, stream=stream)
    torch.cuda.synchronize()
    assert engine.kernel_launches() - before == (_passes(st.rows) if launches is None else launches)
    st.same("after check")
    return [int(v) for v in bad.cpu().numpy().view(np.uint64)]


# (matrix, k, rows, the tile whose lengths the encode case uses)
ENCODE_CASES = [("rs", 4, 2, 2048), ("rs", 10, 4, 4096), ("cauchy", 20, 8, 4096), ("rs", 6, 10, 4096),
                ("rs", 6, 10, 2048), ("pq", 6, 2, 2048)]
GEOMETRIES = [("rs", 4, 2), ("rs", 10, 4), ("cauchy", 20, 8), ("rs", 6, 10), ("pq", 6, 2)]


@pytest.mark.parametrize("order", range(6))
@pytest.mark.parametrize("kind,k,rows,T", ENCODE_CASES)
def test_ragged_encode_matches_the_oracle_per_stripe(engine, gpu, kind, k, rows, T, order):
    """Byte-exact parity, sources and guards untouched, one launch per pass, a
    second run leaves the same image."""
    lens = orders(T)[order]
    st = Stripes(gpu, kind, k, rows, lens, 100 + order)
    rg = engine.Ragged(k, rows, st.tbls, lens, st.data, st.coding)
    try:
        first = _encode(engine, st, rg, "first run")
        assert np.array_equal(_encode(engine, st, rg, "second run"), first)
    finally:
        rg.close()


def test_ragged_all_zero_lengths_enqueue_nothing(engine, gpu):
    k, rows = 10, 4
    st = Stripes(gpu, "rs", k, rows, [0, 0, 0], 7)
    assert len(st.image) == 3 * (k + rows) * GUARD_BYTES
    rg = engine.Ragged(k, rows, st.tbls, st.lens, st.data, st.coding)
    try:
        _encode(engine, st, rg, "all lengths zero", launches=0)
        assert _check(engine, st, rg, launches=0) == [GARBAGE] * 3
    finally:
        rg.close()


def test_ragged_encode_is_ordered_on_the_callers_stream(engine, gpu):
    """The sources arrive by a copy queued on a side stream, the encode is
    queued behind it: the parity is that of the copied sources."""
    k, rows = 10, 4
    lens = orders(4096)[3]
    st = Stripes(gpu, "rs", k, rows, lens, 8)
    staged = torch.from_numpy(st.poisoned.copy()).pin_memory()
    st.dev.zero_()
    rg = engine.Ragged(k, rows, st.tbls, lens, st.data, st.coding)
    stream = torch.cuda.Stream(device=gpu)
    try:
        torch.cuda.synchronize()
        before = engine.kernel_launches()
        with torch.cuda.stream(stream):
            st.dev.copy_(staged, non_blocking=True)
            rg.encode(stream.cuda_stream)
        stream.synchronize()
        assert engine.kernel_launches() - before == 1
    finally:
        rg.close()
    st.same("side stream", st.want)


def _stripe_of(lens, n):
    return lens.index(n)


@pytest.mark.parametrize("order", [0, 3])
@pytest.mark.parametrize("kind,k,rows", GEOMETRIES)
def test_ragged_check_names_the_first_mismatch_of_each_stripe(engine, oracle, gpu, kind, k, rows, order):
    T = 4096
    lens = orders(T)[order]
    st = Stripes(gpu, kind, k, rows, lens, 200 + order)
    rg = engine.Ragged(k, rows, st.tbls, lens, st.data, st.coding)
    long_, two, one = _stripe_of(lens, 2 * T + 55), _stripe_of(lens, T + 16), _stripe_of(lens, 1)
    try:
        _encode(engine, st, rg, "encode")
        st.image = st.want.copy()
        assert _check(engine, st, rg) == [CLEAN] * st.S
        places = [
            [(long_, k - 1, 2 * T + 54)],  # the last byte of a byte tail
            [(two, 0, T)],  # the first byte of a second tile
            [(long_, k + rows - 1, T + 16 * 3 + 2)],  # a parity shard: the last row (the last pass)
            [(one, k // 2, 0)],  # a stripe of length 1
            # two corrupt stripes; in one a parity row at a smaller column than a data shard
            [(long_, k + rows - 1, 16 * 200 + 9), (long_, 1, 2 * T + 5), (two, k, T + 15)],
        ]
        for flips in places:
            for s, shard, col in flips:
                st.flip(s, shard, col)
            want = st.model_bad(oracle)
            hit = sorted({s for s, _, _ in flips})
            assert [s for s in range(st.S) if want[s] != CLEAN] == hit, (flips, want)
            assert _check(engine, st, rg) == want, flips
            st.restore()
            assert _check(engine, st, rg) == [CLEAN] * st.S
    finally:
        rg.close()


def _equal_lengths(gpu, encoded):
    T = 4096
    return Stripes(gpu, "rs", 10, 4, [T + 16 + 5] * 8, 300, encoded=encoded)


def test_ragged_equal_lengths_write_what_a_batch_writes(engine, gpu):
    st = _equal_lengths(gpu, encoded=False)
    n = st.lens[0]
    rg = engine.Ragged(st.k, st.rows, st.tbls, st.lens, st.data, st.coding)
    try:
        ragged = _encode(engine, st, rg, "ragged")
    finally:
        rg.close()
    st.dev.copy_(torch.from_numpy(st.poisoned.copy()))
    b = engine.Batch(n, st.k, st.rows, st.tbls, st.S, st.data, st.coding)
    try:
        b.encode(0)
        torch.cuda.synchronize()
    finally:
        b.close()
    assert np.array_equal(st.dev.cpu().numpy(), ragged)


def test_ragged_check_agrees_with_batch_check_on_equal_lengths(engine, oracle, gpu):
    st = _equal_lengths(gpu, encoded=True)
    n = st.lens[0]
    st.flip(1, 3, n - 1)
    st.flip(4, st.k + 2, 4096)
    st.flip(4, 0, 4096 + 3)
    st.flip(6, 9, 17)
    rg = engine.Ragged(st.k, st.rows, st.tbls, st.lens, st.data, st.coding)
    try:
        got = _check(engine, st, rg)
    finally:
        rg.close()
    bad = torch.full((st.S,), GARBAGE, dtype=torch.int64, device=gpu)
    b = engine.Batch(n, st.k, st.rows, st.tbls, st.S, st.data, st.coding)
    try:
        b.check(bad, 0)
        torch.cuda.synchronize()
    finally:
        b.close()
    assert got == [int(v) for v in bad.cpu().numpy().view(np.uint64)]
    assert got == st.model_bad(oracle) and [s for s in range(st.S) if got[s] != CLEAN] == [1, 4, 6]
