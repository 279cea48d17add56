"""GPU tier: the repair batch (include/isal_hip.h) — stripes with mixed erasure
patterns rebuilt by one launch per pass.

The checker is ecutil.decode_matrix + oracle.ec_init_tables +
oracle.ec_encode_data per stripe, never the engine's own output. Every stripe
is decodable (see test_repair_cpu.py), so none is skipped.

Sizes: each len is the smallest that still reaches two full column tiles, a
partial tile of 16-byte lanes and a byte tail, for the 128-lane blocks of
1-2 rows (2 KiB tiles) and the 256-lane blocks of 3-8 rows (4 KiB tiles).
"""
import itertools
import random

import numpy as np
import pytest
import torch

import ecutil

pytestmark = pytest.mark.gpu

POISON, GUARD, GUARD_BYTES = 0xA5, 0x3C, 64


def _matrix(oracle, gen, k, m):
    return oracle.gf_gen_rs_matrix(m, k) if gen == "rs" else oracle.gf_gen_cauchy1_matrix(m, k)


class Stripes:
    """S encoded stripes in one device allocation: shard (s, i) at row s*m + i
    of a (S*m, span) byte matrix, span = len + a guard of at least 64 bytes,
    rounded up so every shard starts 16-byte aligned. `want` is the host image
    the device must hold after the rebuild (the checker's bytes in the erased
    shards, everything else as uploaded)."""

    def __init__(self, oracle, gpu, a, k, m, len_, patterns, seed):
        self.k, self.m, self.len, self.S = k, m, len_, len(patterns)
        self.patterns = [tuple(sorted(p)) for p in patterns]
        self.span = (len_ + GUARD_BYTES + 15) // 16 * 16
        host = np.full((self.S * m, self.span), GUARD, np.uint8)
        for s in range(self.S):
            data = [ecutil.fill_bytes(len_, seed * 1000 + s * k + j) for j in range(k)]
            parity = oracle.encode(a[k * k:], k, m - k, data) if len_ else [data[0]] * (m - k)
            for i, sh in enumerate(data + parity):
                host[s * m + i, :len_] = sh
        self.want = host.copy()
        rows = {}
        for s, pat in enumerate(self.patterns):
            if pat not in rows:
                ret, c, surv = ecutil.decode_matrix(a, k, list(pat), oracle)
                assert ret == 0, f"the checker calls {pat} singular"
                rows[pat] = (oracle.ec_init_tables(k, len(pat), c), surv)
            tbls, surv = rows[pat]
            dst = [np.zeros(len_, np.uint8) for _ in pat]
            if len_:
                oracle.ec_encode_data(len_, k, len(pat), tbls, [host[s * m + i, :len_].copy() for i in surv], dst)
            for e, d in zip(pat, dst):
                assert np.array_equal(d, host[s * m + e, :len_]), "the checker does not rebuild the encoded shard"
                host[s * m + e, :len_] = POISON
        self.poisoned = host
        self.dev = torch.from_numpy(host).to(gpu)
        self.shards = [int(self.dev[r].data_ptr()) for r in range(self.S * m)]
        assert all(p % 16 == 0 for p in self.shards)

    def errs(self, seed):
        """Every stripe's erasures in a shuffled order."""
        rng, out = random.Random(seed), []
        for pat in self.patterns:
            e = list(pat)
            rng.shuffle(e)
            out += e
        return out

    def repoison(self):
        self.dev.copy_(torch.from_numpy(self.poisoned))
        torch.cuda.synchronize()

    def check(self, what):
        got = self.dev.cpu().numpy()
        m, n = self.m, self.len
        for s, pat in enumerate(self.patterns):
            for i in range(m):
                r = s * m + i
                kind = "rebuilt shard" if i in pat else "survivor"
                assert np.array_equal(got[r, :n], self.want[r, :n]), f"{what}: stripe {s} {kind} {i} differs"
                assert np.array_equal(got[r, n:], self.want[r, n:]), f"{what}: stripe {s} shard {i}: guard written"
        return got


def _rebuild(engine, oracle, gpu, gen, k, m, nerrs, len_, patterns, seed, launches):
    a = _matrix(oracle, gen, k, m)
    st = Stripes(oracle, gpu, a, k, m, len_, patterns, seed)
    r = engine.Repair(len_, k, m, a, nerrs, st.S, st.errs(seed), st.shards)
    try:
        assert r.npatterns() == len(set(st.patterns))
        torch.cuda.synchronize()
        before = engine.kernel_launches()
        r.run(0)
        torch.cuda.synchronize()
        assert engine.kernel_launches() - before == launches
        first = st.check("first run")
        before = engine.kernel_launches()
        r.run(0)
        torch.cuda.synchronize()
        assert engine.kernel_launches() - before == launches
        assert np.array_equal(st.check("second run"), first)
    finally:
        r.close()
    return st


def _cycle(pats, n, seed):
    out = [pats[i % len(pats)] for i in range(n)]
    random.Random(seed).shuffle(out)
    return out


@pytest.mark.parametrize("nerrs", [1, 2])
def test_repair_rs_4_6_every_pattern(engine, oracle, gpu, nerrs):
    """Case 1: 128-lane blocks; data-only, parity-only and mixed erasures."""
    k, m = 4, 6
    pats = list(itertools.combinations(range(m), nerrs))
    stripes = _cycle(pats, 37, 10 + nerrs)
    assert set(stripes) == set(pats) and len(pats) == (6, 15)[nerrs - 1]
    if nerrs == 2:
        assert (4, 5) in stripes and (0, 1) in stripes and (0, 5) in stripes
    _rebuild(engine, oracle, gpu, "rs", k, m, nerrs, 8213, stripes, 20 + nerrs, 1)


@pytest.mark.parametrize("nerrs", [3, 4])
def test_repair_rs_10_14_seeded_patterns(engine, oracle, gpu, nerrs):
    """Case 2: the typical rebuild, 256-lane blocks, 3-4 rows."""
    k, m = 10, 14
    rng = random.Random(30 + nerrs)
    stripes = [tuple(sorted(rng.sample(range(m), nerrs))) for _ in range(64)]
    assert len(set(stripes)) >= 20
    _rebuild(engine, oracle, gpu, "rs", k, m, nerrs, 8240, stripes, 40 + nerrs, 1)


@pytest.mark.parametrize("nerrs", [6, 8])
def test_repair_cauchy_20_28_wide_passes(engine, oracle, gpu, nerrs):
    """Case 3: the 5-8 row route."""
    k, m = 20, 28
    rng = random.Random(50 + nerrs)
    pool = [tuple(sorted(rng.sample(range(m), nerrs))) for _ in range(10)]
    stripes = _cycle(pool, 24, 60 + nerrs)
    assert len(set(stripes)) >= 8
    _rebuild(engine, oracle, gpu, "cauchy", k, m, nerrs, 8208, stripes, 70 + nerrs, 1)


def test_repair_cauchy_4_14_nine_erasures_two_passes(engine, oracle, gpu):
    """Case 4: nerrs > 8 runs in two passes (8 rows + 1 row): two launches."""
    k, m, nerrs = 4, 14, 9
    rng = random.Random(80)
    stripes = []
    while len(stripes) < 6:
        p = tuple(sorted(rng.sample(range(m), nerrs)))
        if p not in stripes:
            stripes.append(p)
    assert engine.max_rows_per_pass() == 8
    _rebuild(engine, oracle, gpu, "cauchy", k, m, nerrs, 4112, stripes, 81, 2)


def test_repair_empty_shards_launch_nothing(engine, oracle, gpu):
    st = _rebuild(engine, oracle, gpu, "rs", 10, 14, 3, 0, [(0, 7, 12), (1, 2, 3)], 90, 0)
    assert st.span == GUARD_BYTES


def test_repair_byte_tail_only(engine, oracle, gpu):
    _rebuild(engine, oracle, gpu, "rs", 10, 14, 3, 5, [(0, 7, 12), (1, 2, 3), (11, 12, 13)], 91, 1)
    _rebuild(engine, oracle, gpu, "rs", 4, 6, 2, 5, [(0, 5), (4, 5)], 92, 1)


def test_repair_single_stripe(engine, oracle, gpu):
    _rebuild(engine, oracle, gpu, "rs", 10, 14, 4, 8240, [(2, 9, 10, 13)], 93, 1)


def test_repair_uniform_pattern_equals_a_batch_with_decode_tables(engine, oracle, gpu):
    """All 64 stripes on one pattern: byte for byte what a Batch computes on
    the same pointers once set_tables() gave it the decode tables."""
    k, m, nerrs, n, S = 10, 14, 3, 8240, 64
    pat = (3, 8, 11)
    a = _matrix(oracle, "rs", k, m)
    st = _rebuild(engine, oracle, gpu, "rs", k, m, nerrs, n, [pat] * S, 94, 1)
    repaired = st.dev.cpu().numpy()
    st.repoison()
    ret, c, surv = ecutil.decode_matrix(a, k, list(pat), oracle)
    assert ret == 0
    data = [st.shards[s * m + i] for s in range(S) for i in surv]
    coding = [st.shards[s * m + e] for s in range(S) for e in pat]
    b = engine.Batch(n, k, nerrs, oracle.ec_init_tables(k, nerrs, a[k * k:(k + nerrs) * k]), S, data, coding)
    try:
        b.set_tables(oracle.ec_init_tables(k, nerrs, c))
        b.encode(0)
        torch.cuda.synchronize()
    finally:
        b.close()
    assert np.array_equal(st.dev.cpu().numpy(), repaired)


def test_repair_is_ordered_on_the_callers_stream(engine, oracle, gpu):
    """run() on a non-default stream, then a device-to-host copy on that
    stream: the copy reads finished data."""
    k, m, nerrs, n = 10, 14, 3, 8240
    rng = random.Random(95)
    stripes = [tuple(sorted(rng.sample(range(m), nerrs))) for _ in range(64)]
    a = _matrix(oracle, "rs", k, m)
    st = Stripes(oracle, gpu, a, k, m, n, stripes, 96)
    r = engine.Repair(n, k, m, a, nerrs, st.S, st.errs(97), st.shards)
    out = torch.empty(st.dev.shape, dtype=torch.uint8).pin_memory()
    stream = torch.cuda.Stream(device=gpu)
    try:
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            r.run(stream.cuda_stream)
            out.copy_(st.dev, non_blocking=True)
        stream.synchronize()
    finally:
        r.close()
    assert np.array_equal(out.numpy(), st.want)
