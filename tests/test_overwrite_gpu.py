"""GPU tier: the overwrite batch (include/isal_hip.h) — partial-stripe writes
folded into the parity by one launch per pass.

The checker never uses the engine's output: the wanted parity is oracle.encode
of the WHOLE stripe with the new bytes in place (a fresh encode, independent
of the delta algebra), the wanted data the new bytes after a commit and the old
ones without. Every comparison is over the whole device image, so guards,
untouched data shards and the `new` buffers must come back unchanged too.

Sizes: LEN is two full column tiles, a partial tile of three 16-byte lanes and
a 5-byte tail, for 2 KiB or 4 KiB tiles; 0, 5 and 16 are the degenerate ones.
"""
import random

import numpy as np
import pytest
import torch

import ecutil

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTES = 0x3C, 64
LEN = 2 * 4096 + 3 * 16 + 5


def _coef(oracle, gen, k, rows):
    a = oracle.gf_gen_rs_matrix(k + rows, k) if gen == "rs" else oracle.gf_gen_cauchy1_matrix(k + rows, k)
    return a[k * k:]


class Writes:
    """S encoded stripes and their pending writes in one device allocation, a
    (S*(k+rows) + S*nw, span) byte matrix: shard i of stripe s (data, then
    parity) at row s*(k+rows) + i, the new bytes of slot i of stripe s at row
    S*(k+rows) + s*nw + i; span = len + a guard of at least 64 bytes, rounded
    up so that every row starts 16-byte aligned. Host images: `before` (as
    uploaded), `parity_only` (after a run without commit) and `committed`."""

    def __init__(self, oracle, gpu, gen, k, rows, len_, idx_sets, seed):
        self.k, self.rows, self.len, self.S, self.nw = k, rows, len_, len(idx_sets), len(idx_sets[0])
        self.m, self.idx_sets = k + rows, [list(x) for x in idx_sets]
        self.coef = _coef(oracle, gen, k, rows)
        self.tbls = oracle.ec_init_tables(k, rows, self.coef)
        self.span = (len_ + GUARD_BYTES + 15) // 16 * 16
        S, m, nw = self.S, self.m, self.nw
        self.new0 = S * m
        host = np.full((S * m + S * nw, self.span), GUARD, np.uint8)
        after = None
        want_parity = []
        for s, ix in enumerate(self.idx_sets):
            assert len(ix) == nw and len(set(ix)) == nw and all(0 <= j < k for j in ix)
            data = [ecutil.fill_bytes(len_, seed * 100000 + s * k + j) for j in range(k)]
            new = [ecutil.fill_bytes(len_, seed * 100000 + 50000 + s * nw + i) for i in range(nw)]
            cur = list(data)
            for i, j in enumerate(ix):
                assert len_ == 0 or not np.array_equal(new[i], data[j])
                cur[j] = new[i]
            parity = oracle.encode(self.coef, k, rows, data) if len_ else [data[0]] * rows
            want_parity.append(oracle.encode(self.coef, k, rows, cur) if len_ else parity)
            for i, sh in enumerate(data + parity):
                host[s * m + i, :len_] = sh
            for i in range(nw):
                host[self.new0 + s * nw + i, :len_] = new[i]
        self.before = host
        after = host.copy()
        for s in range(S):
            for l in range(rows):
                after[s * m + k + l, :len_] = want_parity[s][l]
        self.parity_only = after
        self.committed = after.copy()
        for s, ix in enumerate(self.idx_sets):
            for i, j in enumerate(ix):
                self.committed[s * m + j, :len_] = host[self.new0 + s * nw + i, :len_]
        self.dev = torch.from_numpy(host).to(gpu)
        row = [int(self.dev[r].data_ptr()) for r in range(host.shape[0])]
        assert all(p % 16 == 0 for p in row)
        self.row = row
        self.idx = [j for ix in self.idx_sets for j in ix]
        self.old = [row[s * m + j] for s, ix in enumerate(self.idx_sets) for j in ix]
        self.new = [row[self.new0 + r] for r in range(S * nw)]
        self.coding = [row[s * m + k + l] for s in range(S) for l in range(rows)]

    def overwrite(self, engine):
        return engine.Overwrite(self.len, self.k, self.rows, self.tbls, self.nw, self.S, self.idx, self.old,
                                self.new, self.coding)

    def reset(self):
        self.dev.copy_(torch.from_numpy(self.before))
        torch.cuda.synchronize()

    def kind(self, r):
        if r >= self.new0:
            s, i = divmod(r - self.new0, self.nw)
            return f"stripe {s} new buffer of slot {i}"
        s, i = divmod(r, self.m)
        if i >= self.k:
            return f"stripe {s} parity row {i - self.k}"
        return f"stripe {s} {'rewritten' if i in self.idx_sets[s] else 'untouched'} data shard {i}"

    def check(self, want, what):
        got = self.dev.cpu().numpy()
        if not np.array_equal(got, want):
            r = int(np.nonzero((got != want).any(axis=1))[0][0])
            c = int(np.nonzero(got[r] != want[r])[0][0])
            where = "guard" if c >= self.len else f"byte {c}"
            raise AssertionError(f"{what}: {self.kind(r)} differs at {where} (and maybe later rows)")
        return got


def _run(engine, w, ow, commit, launches, stream=0):
    torch.cuda.synchronize()
    before = engine.kernel_launches()
    ow.run(commit=commit, stream=stream)
    torch.cuda.synchronize()
    assert engine.kernel_launches() - before == launches


def _seeded_sets(k, nw, S, seed):
    """Per-stripe index sets from a seeded shuffle, in shuffled slot order."""
    rng = random.Random(seed)
    return [rng.sample(range(k), nw) for _ in range(S)]


@pytest.mark.parametrize("commit", [False, True])
def test_overwrite_rs_4_2_every_index(engine, oracle, gpu, commit):
    """Case 1: one write per stripe, every index across the stripes."""
    k, rows, S = 4, 2, 9
    sets = [[j] for j in (2, 0, 3, 1, 1, 3, 0, 2, 0)]
    assert {x[0] for x in sets} == set(range(k)) and len(sets) == S
    w = Writes(oracle, gpu, "rs", k, rows, LEN, sets, 1)
    ow = w.overwrite(engine)
    try:
        _run(engine, w, ow, commit, 1)
        w.check(w.committed if commit else w.parity_only, f"commit={commit}")
    finally:
        ow.close()


@pytest.mark.parametrize("nw", [1, 3])
def test_overwrite_rs_10_4_seeded_sets_committed(engine, oracle, gpu, nw):
    """Case 2: the typical small write; one launch; a second committed run
    finds a zero delta and changes no byte."""
    k, rows, S = 10, 4, 24
    sets = _seeded_sets(k, nw, S, 20 + nw)
    assert len({tuple(sorted(x)) for x in sets}) >= 8 and (nw == 1 or any(x != sorted(x) for x in sets))
    w = Writes(oracle, gpu, "rs", k, rows, LEN, sets, 2 + nw)
    ow = w.overwrite(engine)
    try:
        _run(engine, w, ow, True, 1)
        first = w.check(w.committed, "first committed run")
        _run(engine, w, ow, True, 1)
        assert np.array_equal(w.check(w.committed, "second committed run"), first)
    finally:
        ow.close()


def test_overwrite_cauchy_20_10_two_passes_commit_in_the_last(engine, oracle, gpu):
    """Case 3: rows 8 and 9 belong to the second pass; they come out wrong
    (unchanged) if the first pass already stored new over old."""
    k, rows, S, nw = 20, 10, 6, 2
    assert engine.max_rows_per_pass() == 8
    w = Writes(oracle, gpu, "cauchy", k, rows, LEN, _seeded_sets(k, nw, S, 30), 6)
    for s in range(S):
        for l in (8, 9):
            assert not np.array_equal(w.before[s * w.m + k + l], w.committed[s * w.m + k + l])
    ow = w.overwrite(engine)
    try:
        _run(engine, w, ow, True, 2)
        w.check(w.committed, "two passes, committed")
        _run(engine, w, ow, True, 2)
        w.check(w.committed, "two passes, second committed run")
    finally:
        ow.close()


@pytest.mark.parametrize("gen,k,rows,nw", [("rs", 10, 4, 3), ("cauchy", 20, 10, 2)])
def test_overwrite_without_commit_twice_restores_the_parity(engine, oracle, gpu, gen, k, rows, nw):
    """Case 4."""
    w = Writes(oracle, gpu, gen, k, rows, LEN, _seeded_sets(k, nw, 8, 40 + k), 7)
    passes = (rows + 7) // 8
    ow = w.overwrite(engine)
    try:
        _run(engine, w, ow, False, passes)
        w.check(w.parity_only, "first run")
        _run(engine, w, ow, False, passes)
        w.check(w.before, "second run")
    finally:
        ow.close()


def test_overwrite_uniform_index_equals_the_composed_route(engine, oracle, gpu):
    """Case 5: every stripe rewrites shard 6: byte for byte what the XOR of old
    and new (here on the host), uploaded, gives through Batch.update(6)."""
    k, rows, S, j0 = 10, 4, 16, 6
    w = Writes(oracle, gpu, "rs", k, rows, LEN, [[j0]] * S, 8)
    ow = w.overwrite(engine)
    try:
        _run(engine, w, ow, False, 1)
        fused = w.check(w.parity_only, "overwrite")
    finally:
        ow.close()
    w.reset()
    delta = np.full((S, w.span), GUARD, np.uint8)
    for s in range(S):
        delta[s, :LEN] = w.before[s * w.m + j0, :LEN] ^ w.before[w.new0 + s, :LEN]
    scratch = torch.from_numpy(delta).to(gpu)
    data = [int(scratch[s].data_ptr()) if j == j0 else w.row[s * w.m + j] for s in range(S) for j in range(k)]
    b = engine.Batch(LEN, k, rows, w.tbls, S, data, w.coding)
    try:
        b.update(j0, 0)
        torch.cuda.synchronize()
    finally:
        b.close()
    assert np.array_equal(w.dev.cpu().numpy(), fused)
    assert np.array_equal(scratch.cpu().numpy(), delta)


def test_overwrite_whole_stripe_equals_a_fresh_encode(engine, oracle, gpu):
    """Case 6: nw = k, committed: the parity is what Batch.encode computes from
    the data shards as they stand afterwards."""
    k, rows, S = 10, 4, 5
    w = Writes(oracle, gpu, "rs", k, rows, LEN, _seeded_sets(k, k, S, 60), 9)
    ow = w.overwrite(engine)
    try:
        _run(engine, w, ow, True, 1)
        got = w.check(w.committed, "nw = k")
    finally:
        ow.close()
    fresh = torch.full((S * rows, w.span), GUARD, dtype=torch.uint8, device=gpu)
    b = engine.Batch(LEN, k, rows, w.tbls, S, [w.row[s * w.m + j] for s in range(S) for j in range(k)],
                     [int(fresh[r].data_ptr()) for r in range(S * rows)])
    try:
        b.encode(0)
        torch.cuda.synchronize()
    finally:
        b.close()
    fresh = fresh.cpu().numpy()
    for s in range(S):
        for l in range(rows):
            assert np.array_equal(fresh[s * rows + l], got[s * w.m + k + l]), (s, l)


@pytest.mark.parametrize("len_,launches", [(0, 0), (5, 1), (16, 1)])
@pytest.mark.parametrize("commit", [False, True])
def test_overwrite_short_ranges(engine, oracle, gpu, len_, launches, commit):
    """len of 0 (nothing launched), a byte tail alone, one 16-byte lane alone."""
    w = Writes(oracle, gpu, "rs", 10, 4, len_, _seeded_sets(10, 3, 3, 70 + len_), 10)
    assert len_ or w.span == GUARD_BYTES
    ow = w.overwrite(engine)
    try:
        _run(engine, w, ow, commit, launches)
        w.check(w.committed if commit else w.parity_only, f"len={len_} commit={commit}")
    finally:
        ow.close()


def test_overwrite_single_stripe_byte_tail_two_passes(engine, oracle, gpu):
    """Case 7: one stripe, len = 5, and the pass rule on the byte path."""
    for gen, k, rows, nw, launches in (("rs", 4, 2, 1, 1), ("cauchy", 20, 10, 2, 2)):
        w = Writes(oracle, gpu, gen, k, rows, 5, _seeded_sets(k, nw, 1, 80 + k), 11)
        ow = w.overwrite(engine)
        try:
            _run(engine, w, ow, True, launches)
            w.check(w.committed, f"{gen} {k}+{rows}")
        finally:
            ow.close()


def test_overwrite_is_ordered_on_the_callers_stream(engine, oracle, gpu):
    """Case 7: the new bytes arrive by a copy on a side stream; a run enqueued
    on that stream after the copy reads them."""
    k, rows, S, nw = 10, 4, 24, 3
    w = Writes(oracle, gpu, "rs", k, rows, LEN, _seeded_sets(k, nw, S, 90), 12)
    staged = torch.from_numpy(w.before[w.new0:].copy()).pin_memory()
    w.dev[w.new0:, :LEN] = 0x5A  # what a run that does not wait for the copy would read
    ow = w.overwrite(engine)
    stream = torch.cuda.Stream(device=gpu)
    try:
        torch.cuda.synchronize()
        before = engine.kernel_launches()
        with torch.cuda.stream(stream):
            w.dev[w.new0:].copy_(staged, non_blocking=True)
            ow.run(commit=True, stream=stream.cuda_stream)
        stream.synchronize()
        assert engine.kernel_launches() - before == 1
    finally:
        ow.close()
    w.check(w.committed, "side stream")


def test_overwrite_run_rejects_unknown_flags_and_enqueues_nothing(engine, oracle, gpu):
    w = Writes(oracle, gpu, "rs", 4, 2, 64, [[1], [3]], 13)
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


def test_overwrite_create_names_the_overlapping_stripe_on_device_memory(engine, oracle, gpu):
    """The overlap refusal with real device pointers: stripe 1's new buffer is
    its own parity row 0."""
    w = Writes(oracle, gpu, "rs", 4, 2, 64, [[1], [3], [0]], 14)
    new = list(w.new)
    new[1] = w.coding[1 * 2 + 0]
    with pytest.raises(RuntimeError, match=r"\(-1, stripe 1\)"):
        engine.Overwrite(w.len, w.k, w.rows, w.tbls, w.nw, w.S, w.idx, w.old, new, w.coding)
