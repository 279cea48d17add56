"""GPU tier: the ragged repair (include/isal_hip.h "Ragged repair") — stripes of
mixed lengths AND mixed erasure counts rebuilt by one launch per pass of each
count class.

The checker is ecutil.decode_matrix + oracle.ec_init_tables +
oracle.ec_encode_data per stripe, never the engine's own output. Every pattern
is decodable (the geometries of test_repair_gpu.py; asserted at construction),
so none is skipped.

Lengths: LENS straddles the 2 KiB tiles of 1-2 row passes and the 4 KiB tiles
of 3-8 row passes (one below, exact, one above, and more than two tiles), one
16-byte vector, and the byte tail; 0 is a stripe that must not be touched.
"""
import itertools
import random

import numpy as np
import pytest
import torch

import ecutil

pytestmark = pytest.mark.gpu

POISON, GUARD, GUARD_BYTES = 0xA5, 0x3C, 64
LENS = [0, 1, 15, 16, 17, 2047, 2048, 2049, 4095, 4096, 4097, 4112, 8197]


def _matrix(oracle, gen, k, m):
    return oracle.gf_gen_rs_matrix(m, k) if gen == "rs" else oracle.gf_gen_cauchy1_matrix(m, k)


class RaggedStripes:
    """test_repair_gpu.py's Stripes with a length per stripe: S encoded stripes
    in one device allocation, shard (s, i) at offset off[s] + i * span[s],
    span[s] = lens[s] + a guard of at least 64 bytes, rounded up so every
    shard starts 16-byte aligned. `want` is the host image the device must
    hold after the rebuild (the checker's bytes in the erased shards,
    everything else, guards included, as uploaded)."""

    def __init__(self, oracle, gpu, a, k, m, lens, patterns, seed):
        assert len(lens) == len(patterns)
        self.k, self.m, self.lens, self.S = k, m, list(lens), len(lens)
        self.patterns = [tuple(sorted(p)) for p in patterns]
        self.span = [(n + GUARD_BYTES + 15) // 16 * 16 for n in self.lens]
        self.off = [0]
        for sp in self.span:
            self.off.append(self.off[-1] + m * sp)
        host = np.full(self.off[-1], GUARD, np.uint8)
        for s, n in enumerate(self.lens):
            data = [ecutil.fill_bytes(n, seed * 1000 + s * k + j) for j in range(k)]
            parity = oracle.encode(a[k * k:], k, m - k, data) if n else [data[0]] * (m - k)
            for i, sh in enumerate(data + parity):
                self._shard(host, s, i)[:] = sh
        self.want = host.copy()
        rows = {}
        for s, pat in enumerate(self.patterns):
            n = self.lens[s]
            if not pat:
                continue
            if pat not in rows:
                ret, c, surv = ecutil.decode_matrix(a, k, list(pat), oracle)
                assert ret == 0, f"the checker calls {pat} singular"
                rows[pat] = (oracle.ec_init_tables(k, len(pat), c), surv)
            tbls, surv = rows[pat]
            dst = [np.zeros(n, np.uint8) for _ in pat]
            if n:
                oracle.ec_encode_data(n, k, len(pat), tbls, [self._shard(host, s, i).copy() for i in surv], dst)
            for e, d in zip(pat, dst):
                assert np.array_equal(d, self._shard(host, s, e)), "the checker does not rebuild the encoded shard"
                self._shard(host, s, e)[:] = POISON
        self.poisoned = host
        self.dev = torch.from_numpy(host).to(gpu)
        base = int(self.dev.data_ptr())
        self.shards = [base + self.off[s] + i * self.span[s] for s in range(self.S) for i in range(m)]
        assert all(p % 16 == 0 for p in self.shards)

    def _shard(self, image, s, i):
        at = self.off[s] + i * self.span[s]
        return image[at:at + self.lens[s]]

    def errs(self, seed):
        """Every stripe's erasures in a shuffled order."""
        rng, out = random.Random(seed), []
        for pat in self.patterns:
            e = list(pat)
            rng.shuffle(e)
            out.append(e)
        return out

    def launches(self, engine):
        """Sum of ceil(c / max_rows_per_pass) over the count classes present."""
        rows = engine.max_rows_per_pass()
        present = {len(p) for p, n in zip(self.patterns, self.lens) if p and n}
        return sum((c + rows - 1) // rows for c in present)

    def repoison(self):
        self.dev.copy_(torch.from_numpy(self.poisoned))
        torch.cuda.synchronize()

    def check(self, what):
        """The whole image: rebuilt shards, survivors and every guard."""
        got = self.dev.cpu().numpy()
        if not np.array_equal(got, self.want):
            at = int(np.flatnonzero(got != self.want)[0])
            s = max(x for x in range(self.S) if self.off[x] <= at)
            i, b = divmod(at - self.off[s], self.span[s])
            kind = "guard" if b >= self.lens[s] else "rebuilt shard" if i in self.patterns[s] else "survivor"
            raise AssertionError(f"{what}: stripe {s} (len {self.lens[s]}, lost {self.patterns[s]}) shard {i} "
                                 f"byte {b} ({kind}): {got[at]:#x}, want {self.want[at]:#x}")
        return got


def _rebuild(engine, oracle, gpu, gen, k, m, lens, patterns, seed):
    a = _matrix(oracle, gen, k, m)
    st = RaggedStripes(oracle, gpu, a, k, m, lens, patterns, seed)
    launches = st.launches(engine)
    r = engine.Repair.ragged(k, m, a, st.lens, st.errs(seed), st.shards)
    try:
        assert r.npatterns() == len({p for p in st.patterns if p})
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
    return st, launches


def _mixed(pools, per_length, seed):
    """per_length stripes of every length of LENS for each pool of patterns,
    the pool's patterns taken in turn, then all of them shuffled."""
    stripes = []
    for pool in pools:
        for j in range(per_length * len(LENS)):
            stripes.append((LENS[j % len(LENS)], pool[j % len(pool)]))
    random.Random(seed).shuffle(stripes)
    return [n for n, _ in stripes], [p for _, p in stripes]


@pytest.mark.parametrize("seed", [1, 2])
def test_ragged_repair_rs_4_6_every_pattern_of_counts_0_1_2(engine, oracle, gpu, seed):
    """The small-tile passes: every pattern of every count, every length in
    every count."""
    k, m = 4, 6
    pools = [[()], list(itertools.combinations(range(m), 1)), list(itertools.combinations(range(m), 2))]
    # 15 patterns and 13 lengths: 3 * 13 stripes take every pattern at least twice
    lens, pats = _mixed(pools, 3, 100 + seed)
    assert {p for p in pats} == {p for pool in pools for p in pool} and len(set(pats)) == 1 + 6 + 15
    for c in (0, 1, 2):
        assert {n for n, p in zip(lens, pats) if len(p) == c} == set(LENS)
    _, launches = _rebuild(engine, oracle, gpu, "rs", k, m, lens, pats, 110 + seed)
    assert launches == 2


@pytest.mark.parametrize("seed", [1, 2])
def test_ragged_repair_rs_10_14_counts_1_to_4(engine, oracle, gpu, seed):
    """The typical rebuild window: 2 KiB tiles for one and two lost shards,
    4 KiB tiles for three and four."""
    k, m = 10, 14
    rng = random.Random(120 + seed)
    pools = [[tuple(sorted(rng.sample(range(m), c))) for _ in range(9)] for c in (1, 2, 3, 4)]
    lens, pats = _mixed(pools, 1, 130 + seed)
    assert len(set(pats)) >= 25
    _, launches = _rebuild(engine, oracle, gpu, "rs", k, m, lens, pats, 140 + seed)
    assert launches == 4


@pytest.mark.parametrize("seed", [1, 2])
def test_ragged_repair_cauchy_20_28_wide_passes(engine, oracle, gpu, seed):
    """Wide passes on 4 KiB tiles: counts 3, 6 and 8."""
    k, m = 20, 28
    rng = random.Random(150 + seed)
    pools = [[tuple(sorted(rng.sample(range(m), c))) for _ in range(4)] for c in (3, 6, 8)]
    lens, pats = _mixed(pools, 1, 160 + seed)
    _, launches = _rebuild(engine, oracle, gpu, "cauchy", k, m, lens, pats, 170 + seed)
    assert launches == 3


@pytest.mark.parametrize("seed", [1, 2])
def test_ragged_repair_cauchy_4_14_nine_erasures_with_three(engine, oracle, gpu, seed):
    """Count 9 runs two passes, 8 rows on 4 KiB tiles and 1 row on 2 KiB
    tiles, beside a class of count 3: three launches."""
    k, m = 4, 14
    rng = random.Random(180 + seed)
    pools = [[tuple(sorted(rng.sample(range(m), c))) for _ in range(5)] for c in (9, 3)]
    assert engine.max_rows_per_pass() == 8
    lens, pats = _mixed(pools, 1, 190 + seed)
    _, launches = _rebuild(engine, oracle, gpu, "cauchy", k, m, lens, pats, 200 + seed)
    assert launches == 3


def test_ragged_repair_nothing_to_do_launches_nothing(engine, oracle, gpu):
    """Every stripe empty or whole: run returns 0 and enqueues nothing."""
    lens = [0, 4097, 0, 17, 0]
    pats = [(0, 7, 12), (), (3,), (), (1, 2, 3, 13)]
    st, launches = _rebuild(engine, oracle, gpu, "rs", 10, 14, lens, pats, 210)
    assert launches == 0 and np.array_equal(st.poisoned, st.want)


def test_ragged_repair_single_stripe(engine, oracle, gpu):
    _, launches = _rebuild(engine, oracle, gpu, "rs", 10, 14, [8197], [(2, 9, 10, 13)], 211)
    assert launches == 1
    _, launches = _rebuild(engine, oracle, gpu, "rs", 4, 6, [5], [(4,)], 212)  # a byte tail only
    assert launches == 1


def test_ragged_repair_single_class(engine, oracle, gpu):
    k, m = 10, 14
    rng = random.Random(213)
    pool = [tuple(sorted(rng.sample(range(m), 3))) for _ in range(7)]
    lens, pats = _mixed([pool], 2, 214)
    _, launches = _rebuild(engine, oracle, gpu, "rs", k, m, lens, pats, 215)
    assert launches == 1


def test_ragged_repair_of_equal_lengths_and_one_count_equals_the_repair_batch(engine, oracle, gpu):
    """The device image is byte for byte what Repair(len, ...) leaves on a
    copy of the same shards."""
    k, m, nerrs, n, S = 10, 14, 3, 8240, 64
    rng = random.Random(216)
    pats = [tuple(sorted(rng.sample(range(m), nerrs))) for _ in range(S)]
    a = _matrix(oracle, "rs", k, m)
    st, _ = _rebuild(engine, oracle, gpu, "rs", k, m, [n] * S, pats, 217)
    ragged = st.dev.cpu().numpy()
    st.repoison()
    flat = [e for row in st.errs(218) for e in row]
    r = engine.Repair(n, k, m, a, nerrs, S, flat, st.shards)
    try:
        r.run(0)
        torch.cuda.synchronize()
    finally:
        r.close()
    assert np.array_equal(st.dev.cpu().numpy(), ragged)


def test_ragged_repair_is_ordered_on_the_callers_stream(engine, oracle, gpu):
    """run() on a non-default stream, then a device-to-host copy on that
    stream: the copy reads finished data."""
    k, m = 10, 14
    rng = random.Random(219)
    pools = [[tuple(sorted(rng.sample(range(m), c))) for _ in range(9)] for c in (1, 3, 4)]
    lens, pats = _mixed(pools, 2, 220)
    a = _matrix(oracle, "rs", k, m)
    st = RaggedStripes(oracle, gpu, a, k, m, lens, pats, 221)
    r = engine.Repair.ragged(k, m, a, st.lens, st.errs(222), st.shards)
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
