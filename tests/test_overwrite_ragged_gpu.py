"""GPU tier: the ragged overwrite (include/isal_hip.h "Ragged overwrite") —
a window of client writes, each stripe with its own byte count and its own
number of rewritten shards, folded into the parity by one launch per pass.

The checker never uses the engine's output: the wanted parity is oracle.encode
of the WHOLE stripe with the new bytes in place (a fresh encode, independent
of the delta algebra), the wanted data the new bytes after a commit and the old
ones without. Every comparison is over the whole device image, so guards,
untouched data shards, the `new` buffers and the canary row that every unused
slot points at must come back unchanged too. Unused slots hold index 255.

Sizes: LENS is one below, on and one above the 2 KiB tile of this object, a
multi-tile length, one vector, and lengths with a byte tail; 0 is a stripe
that is neither read nor written.
"""
import random

import numpy as np
import pytest
import torch

import ecutil

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTES, CANARY = 0x3C, 64, 0xA7
T = 2048
LONG = 2 * T + 3 * 16 + 5
LENS = [0, 1, 15, 16, 17, 2047, 2048, 2049, 4097, LONG]
PAD_IDX = 255


def _coef(oracle, gen, k, rows):
    a = oracle.gf_gen_rs_matrix(k + rows, k) if gen == "rs" else oracle.gf_gen_cauchy1_matrix(k + rows, k)
    return a[k * k:]


class RaggedWrites:
    """S encoded stripes and their pending writes in one device allocation, a
    (S*(k+rows) + S*max_nw + 1, span) byte matrix: shard i of stripe s (data,
    then parity) at row s*(k+rows) + i over lens[s] bytes, the new bytes of
    slot i of stripe s at row S*(k+rows) + s*max_nw + i, and the canary row
    last; span = the longest length + a guard of at least 64 bytes, rounded up
    so that every row starts 16-byte aligned. Everything past a stripe's own
    length is guard. idx_sets[s] lists the data shards stripe s rewrites, in
    slot order (possibly none). Host images: `before` (as uploaded),
    `parity_only` (after a run without commit) and `committed`."""

    def __init__(self, oracle, gpu, gen, k, rows, lens, idx_sets, seed, max_nw=None):
        assert len(lens) == len(idx_sets)
        self.k, self.rows, self.lens, self.S = k, rows, list(lens), len(lens)
        self.m, self.idx_sets = k + rows, [list(x) for x in idx_sets]
        self.max_nw = max_nw or max([len(x) for x in idx_sets] + [1])
        self.coef = _coef(oracle, gen, k, rows)
        self.tbls = oracle.ec_init_tables(k, rows, self.coef)
        self.span = (max(lens) + GUARD_BYTES + 15) // 16 * 16
        S, m, mw = self.S, self.m, self.max_nw
        self.new0, self.canary = S * m, S * m + S * mw
        host = np.full((self.canary + 1, self.span), GUARD, np.uint8)
        host[self.canary] = CANARY
        want = {}
        for s, (n, ix) in enumerate(zip(self.lens, self.idx_sets)):
            assert len(ix) <= mw and len(set(ix)) == len(ix) and all(0 <= j < k for j in ix)
            if n == 0:
                continue
            data = [ecutil.fill_bytes(n, seed * 100000 + s * k + j) for j in range(k)]
            new = [ecutil.fill_bytes(n, seed * 100000 + 50000 + s * mw + i) for i in range(len(ix))]
            cur = list(data)
            for i, j in enumerate(ix):
                if np.array_equal(new[i], data[j]):  # a one-byte write can repeat the old byte
                    new[i][0] ^= 0xFF
                cur[j] = new[i]
            parity = oracle.encode(self.coef, k, rows, data)
            want[s] = oracle.encode(self.coef, k, rows, cur) if ix else parity
            for i, sh in enumerate(data + parity):
                host[s * m + i, :n] = sh
            for i in range(len(ix)):
                host[self.new0 + s * mw + i, :n] = new[i]
        self.before = host
        after = host.copy()
        for s, parity in want.items():
            for l in range(rows):
                after[s * m + k + l, :self.lens[s]] = parity[l]
        self.parity_only = after
        self.committed = after.copy()
        for s, ix in enumerate(self.idx_sets):
            for i, j in enumerate(ix):
                self.committed[s * m + j, :self.lens[s]] = host[self.new0 + s * mw + i, :self.lens[s]]
        self.dev = torch.from_numpy(host).to(gpu)
        row = [int(self.dev[r].data_ptr()) for r in range(host.shape[0])]
        assert all(p % 16 == 0 for p in row)
        self.row = row
        self.old = [[row[s * m + j] for j in ix] for s, ix in enumerate(self.idx_sets)]
        self.new = [[row[self.new0 + s * mw + i] for i in range(len(ix))] for s, ix in enumerate(self.idx_sets)]
        self.coding = [row[s * m + k + l] for s in range(S) for l in range(rows)]

    @property
    def live(self):
        return sum(1 for n, ix in zip(self.lens, self.idx_sets) if n and ix)

    def overwrite(self, engine):
        """Unused slots: index 255, old and new at the canary row."""
        return engine.Overwrite.ragged(self.k, self.rows, self.tbls, self.lens, self.idx_sets, self.old, self.new,
                                       self.coding, max_nw=self.max_nw, pad_idx=PAD_IDX,
                                       pad_ptr=self.row[self.canary])

    def reset(self):
        self.dev.copy_(torch.from_numpy(self.before))
        torch.cuda.synchronize()

    def kind(self, r):
        if r == self.canary:
            return "the canary row of the unused slots"
        if r >= self.new0:
            s, i = divmod(r - self.new0, self.max_nw)
            return f"stripe {s} (len {self.lens[s]}) new buffer of slot {i}"
        s, i = divmod(r, self.m)
        if i >= self.k:
            return f"stripe {s} (len {self.lens[s]}, {len(self.idx_sets[s])} slots) parity row {i - self.k}"
        return (f"stripe {s} (len {self.lens[s]}) {'rewritten' if i in self.idx_sets[s] else 'untouched'} "
                f"data shard {i}")

    def check(self, want, what):
        got = self.dev.cpu().numpy()
        if not np.array_equal(got, want):
            r = int(np.nonzero((got != want).any(axis=1))[0][0])
            c = int(np.nonzero(got[r] != want[r])[0][0])
            s = (r - self.new0) // self.max_nw if self.new0 <= r < self.canary else r // self.m
            where = "guard" if r == self.canary or c >= self.lens[s] else f"byte {c}"
            raise AssertionError(f"{what}: {self.kind(r)} differs at {where} (and maybe later rows)")
        return got


def _run(engine, ow, commit, launches, stream=0):
    torch.cuda.synchronize()
    before = engine.kernel_launches()
    ow.run(commit=commit, stream=stream)
    torch.cuda.synchronize()
    assert engine.kernel_launches() - before == launches


def _sets(k, counts, seed):
    """One index set per count from a seeded shuffle, in shuffled slot order."""
    rng = random.Random(seed)
    return [rng.sample(range(k), c) for c in counts]


def _window(lens, counts, seed):
    """Every length with every count, in a seeded order."""
    pairs = [(n, c) for c in counts for n in lens]
    random.Random(seed).shuffle(pairs)
    return [n for n, _ in pairs], [c for _, c in pairs]


@pytest.mark.parametrize("commit", [False, True])
def test_ragged_overwrite_rs_4_2_every_length_in_every_count(engine, oracle, gpu, commit):
    """Case 1: counts 0-3 at stride 3, every length of LENS in every count,
    shuffled: one launch."""
    k, rows = 4, 2
    lens, counts = _window(LENS, [0, 1, 2, 3], 1)
    assert len(lens) == 40 and {(n, c) for n, c in zip(lens, counts)} == {(n, c) for n in LENS for c in range(4)}
    w = RaggedWrites(oracle, gpu, "rs", k, rows, lens, _sets(k, counts, 2), 1, max_nw=3)
    assert w.live == 27
    ow = w.overwrite(engine)
    try:
        _run(engine, ow, commit, 1)
        w.check(w.committed if commit else w.parity_only, f"commit={commit}")
    finally:
        ow.close()


def test_ragged_overwrite_rs_10_4_counts_up_to_k_committed_twice(engine, oracle, gpu):
    """Case 2: counts 1-4 and nw = k = 10 in one object, shuffled slot order;
    one launch per run; the second committed run finds a zero delta and
    changes no byte."""
    k, rows = 10, 4
    lens, counts = _window([17, 2049, LONG], [1, 2, 3, 4, 10], 3)
    sets = _sets(k, counts, 4)
    assert any(x != sorted(x) for x in sets) and max(len(x) for x in sets) == k
    w = RaggedWrites(oracle, gpu, "rs", k, rows, lens, sets, 2)
    assert w.max_nw == k
    ow = w.overwrite(engine)
    try:
        _run(engine, ow, True, 1)
        first = w.check(w.committed, "first committed run")
        _run(engine, ow, True, 1)
        assert np.array_equal(w.check(w.committed, "second committed run"), first)
    finally:
        ow.close()


def test_ragged_overwrite_cauchy_20_10_two_passes_commit_in_the_last(engine, oracle, gpu):
    """Case 3: rows 8 and 9 belong to the second pass; they come out wrong
    (unchanged) if the first pass already stored new over old."""
    k, rows = 20, 10
    assert engine.max_rows_per_pass() == 8
    lens, counts = _window([5, 2048, LONG], [1, 2, 3], 5)
    w = RaggedWrites(oracle, gpu, "cauchy", k, rows, lens, _sets(k, counts, 6), 3)
    for s in range(w.S):
        for l in (8, 9):
            assert not np.array_equal(w.before[s * w.m + k + l], w.committed[s * w.m + k + l])
    ow = w.overwrite(engine)
    try:
        _run(engine, ow, True, 2)
        w.check(w.committed, "two passes, committed")
        _run(engine, ow, True, 2)
        w.check(w.committed, "two passes, second committed run")
    finally:
        ow.close()


@pytest.mark.parametrize("gen,k,rows", [("rs", 10, 4), ("cauchy", 20, 10)])
def test_ragged_overwrite_without_commit_twice_restores_the_image(engine, oracle, gpu, gen, k, rows):
    """Case 4."""
    lens, counts = _window([0, 15, 2047, 4097], [0, 1, 2, 3], 7 + k)
    w = RaggedWrites(oracle, gpu, gen, k, rows, lens, _sets(k, counts, 8 + k), 4)
    passes = (rows + 7) // 8
    ow = w.overwrite(engine)
    try:
        _run(engine, ow, False, passes)
        w.check(w.parity_only, "first run")
        _run(engine, ow, False, passes)
        w.check(w.before, "second run")
    finally:
        ow.close()


@pytest.mark.parametrize("commit", [False, True])
def test_ragged_overwrite_with_nothing_to_do_launches_nothing(engine, oracle, gpu, commit):
    """Case 5: every stripe has no byte or no slot."""
    k, rows = 10, 4
    lens, counts = [0, 4097, 0, 16, 0], [3, 0, 0, 0, 1]
    w = RaggedWrites(oracle, gpu, "rs", k, rows, lens, _sets(k, counts, 9), 5, max_nw=3)
    assert w.live == 0
    ow = w.overwrite(engine)
    try:
        _run(engine, ow, commit, 0)
        w.check(w.before, f"commit={commit}")
    finally:
        ow.close()


@pytest.mark.parametrize("n,nw", [(5, 1), (LONG, 3), (LONG, 4)])
def test_ragged_overwrite_single_stripe(engine, oracle, gpu, n, nw):
    """Case 6: a byte tail alone, and three tiles with an odd and an even
    count (the pair group, and the pair group with the single one)."""
    k, rows = 10, 4
    w = RaggedWrites(oracle, gpu, "rs", k, rows, [n], _sets(k, [nw], 10 + nw), 6)
    ow = w.overwrite(engine)
    try:
        _run(engine, ow, False, 1)
        w.check(w.parity_only, "without commit")
        _run(engine, ow, False, 1)
        w.check(w.before, "second run")
        _run(engine, ow, True, 1)
        w.check(w.committed, "committed")
    finally:
        ow.close()


@pytest.mark.parametrize("commit", [False, True])
def test_ragged_overwrite_of_equal_shapes_equals_the_uniform_object(engine, oracle, gpu, commit):
    """Case 7: one length and one count: byte for byte what Overwrite(len, ...,
    nw, ...) leaves on a re-uploaded copy."""
    k, rows, S, nw = 10, 4, 12, 3
    w = RaggedWrites(oracle, gpu, "rs", k, rows, [LONG] * S, _sets(k, [nw] * S, 20), 7)
    ow = w.overwrite(engine)
    try:
        _run(engine, ow, commit, 1)
        ragged = w.check(w.committed if commit else w.parity_only, "ragged")
    finally:
        ow.close()
    w.reset()
    flat = lambda rows_: [p for r in rows_ for p in r]
    uni = engine.Overwrite(LONG, k, rows, w.tbls, nw, S, flat(w.idx_sets), flat(w.old), flat(w.new), w.coding)
    try:
        _run(engine, uni, commit, 1)
    finally:
        uni.close()
    assert np.array_equal(w.dev.cpu().numpy(), ragged)


def test_ragged_overwrite_is_ordered_on_the_callers_stream(engine, oracle, gpu):
    """Case 8: the new bytes arrive by a copy on a side stream; a run enqueued
    on that stream after the copy reads them."""
    k, rows = 10, 4
    lens, counts = _window([17, 2049, LONG], [1, 2, 3], 11)
    w = RaggedWrites(oracle, gpu, "rs", k, rows, lens, _sets(k, counts, 12), 8)
    staged = torch.from_numpy(w.before[w.new0:w.canary].copy()).pin_memory()
    w.dev[w.new0:w.canary] = 0x5A  # what a run that does not wait for the copy would read
    ow = w.overwrite(engine)
    stream = torch.cuda.Stream(device=gpu)
    try:
        torch.cuda.synchronize()
        before = engine.kernel_launches()
        with torch.cuda.stream(stream):
            w.dev[w.new0:w.canary].copy_(staged, non_blocking=True)
            ow.run(commit=True, stream=stream.cuda_stream)
        stream.synchronize()
        assert engine.kernel_launches() - before == 1
    finally:
        ow.close()
    w.check(w.committed, "side stream")


def test_ragged_overwrite_run_rejects_unknown_flags_and_enqueues_nothing(engine, oracle, gpu):
    """Case 9."""
    w = RaggedWrites(oracle, gpu, "rs", 4, 2, [64, 2049], [[1], [3, 0]], 9)
    ow = w.overwrite(engine)
    try:
        torch.cuda.synchronize()
        before = engine.kernel_launches()
        for flags in (2, 3, 1 << 8, -1):
            assert engine.lib().isal_hip_overwrite_run(ow._h, flags, None) == -1
        torch.cuda.synchronize()
        assert engine.kernel_launches() == before
        w.check(w.before, "refused runs")
    finally:
        ow.close()


def test_ragged_overwrite_create_names_the_overlapping_stripe_on_device_memory(engine, oracle, gpu):
    """The overlap refusal with real device pointers: stripe 1's new buffer is
    its own parity row 0; the same alias in an unused slot of stripe 0 passes."""
    w = RaggedWrites(oracle, gpu, "rs", 4, 2, [64, 64, 64], [[1], [3, 2], [0]], 10)
    new = [list(x) for x in w.new]
    new[1][1] = w.coding[1 * 2 + 0]
    with pytest.raises(RuntimeError, match=r"\(-1, stripe 1\)"):
        engine.Overwrite.ragged(w.k, w.rows, w.tbls, w.lens, w.idx_sets, w.old, new, w.coding)
    engine.Overwrite.ragged(w.k, w.rows, w.tbls, w.lens, w.idx_sets, w.old, w.new, w.coding, pad_idx=PAD_IDX,
                            pad_ptr=w.coding[0]).close()
