"""GPU tier: the ragged scrub (include/isal_hip.h "Ragged scrub") — one launch
that names, for every inconsistent stripe of a batch of mixed lengths, the one
shard that explains its mismatches.

As in tests/test_scrub_gpu.py the checker never uses the engine: parity comes
from oracle.encode, the wanted verdict from the model of
tests/test_scrub_cpu.py fed with that parity over each stripe's own length.
Every stripe of a case lies in one device allocation, each shard followed by
at least 64 guard bytes of 0x3C; after every run the whole allocation is
compared with the host image, since a scrub writes nothing. The guard is no
codeword: a kernel that read past lens[s] would see 0x3C in the sources and
in the parity and report a clean stripe as inconsistent. The verdict words are
prefilled with garbage before each run, and every run is also compared with
Ragged.check: verdict CLEAN exactly where bad == ~0.

Sizes: 256 lanes of 16 bytes cover a 4 KiB tile. LENS holds two tiles with a
one-vector-and-5-byte end, a byte tail alone, one lane alone, one and two
exact tiles, three tiles less a byte, a lane and a byte, and two stripes of
length 0 between them: the item index never equals stripe * tiles.
"""
import numpy as np
import pytest
import torch

import ecutil
from test_scrub_cpu import CLEAN, MULTI, matrix, model_verdict

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTES = 0x3C, 64
GARBAGE = 0x5A5A5A5A
TILE = 4096
LENS = [TILE + 16 + 5, 0, 5, 16, TILE, 2 * TILE, 0, 3 * TILE - 1, 17]
LIVE = [s for s, n in enumerate(LENS) if n]


class Stripes:
    """len(lens) encoded stripes in one device allocation, a (S*(k+rows), span)
    byte matrix: shard i of stripe s (data, then parity from the oracle) in the
    first lens[s] bytes of row s*(k+rows) + i, the rest of the row guard bytes
    (at least 64; span is a multiple of 16, so every row starts aligned).
    `clean` is the image as encoded, `image` what the device holds."""

    def __init__(self, oracle, gpu, kind, k, rows, lens, seed):
        self.oracle, self.k, self.rows, self.m, self.lens, self.S = oracle, k, rows, k + rows, list(lens), len(lens)
        self.coef = matrix(oracle, kind, k, rows)
        self.tbls = oracle.ec_init_tables(k, rows, self.coef)
        self.span = (max(lens) + GUARD_BYTES + 15) // 16 * 16
        host = np.full((self.S * self.m, self.span), GUARD, np.uint8)
        for s, n in enumerate(lens):
            if not n:
                continue
            data = [ecutil.fill_bytes(n, seed * 100000 + s * k + j) for j in range(k)]
            for i, sh in enumerate(data + oracle.encode(self.coef, k, rows, data)):
                host[s * self.m + i, :n] = sh
        self.clean = host
        self.image = host.copy()
        self.dev = torch.from_numpy(host).to(gpu)
        self.row = [int(self.dev[r].data_ptr()) for r in range(host.shape[0])]
        assert all(p % 16 == 0 for p in self.row)
        self.data = [self.row[s * self.m + j] for s in range(self.S) for j in range(k)]
        self.coding = [self.row[s * self.m + k + l] for s in range(self.S) for l in range(rows)]

    def flip(self, s, shard, col, x=0x40):
        """XOR x into byte col of shard `shard` of stripe s, on the device and in the image."""
        assert 0 <= col < self.lens[s] and x
        self.image[s * self.m + shard, col] ^= x
        self.dev[s * self.m + shard, col] ^= x

    def restore(self):
        self.image = self.clean.copy()
        self.dev.copy_(torch.from_numpy(self.clean))
        torch.cuda.synchronize()

    def want(self):
        """The model's verdict per stripe for the image as it stands."""
        out = []
        for s, n in enumerate(self.lens):
            if not n:
                out.append(CLEAN)
                continue
            rows_ = self.image[s * self.m:(s + 1) * self.m, :n]
            true = self.oracle.encode(self.coef, self.k, self.rows, [rows_[j].copy() for j in range(self.k)])
            out.append(model_verdict(self.oracle, self.coef, self.k, self.rows, list(rows_[self.k:]), true))
        return out

    def unchanged(self, what):
        got = self.dev.cpu().numpy()
        if not np.array_equal(got, self.image):
            r = int(np.nonzero((got != self.image).any(axis=1))[0][0])
            s, i = divmod(r, self.m)
            raise AssertionError(f"{what}: the scrub wrote to stripe {s} shard {i} or its guard")


def _words(verdict):
    return [int(v) for v in verdict.cpu().numpy().view(np.uint32)]


def _run(engine, st, sc, launches=1, stream=0):
    """One run over garbage-filled verdict words: the launch count, nothing
    written, the verdicts as uint32."""
    verdict = torch.full((st.S,), GARBAGE, dtype=torch.int32, device=st.dev.device)
    torch.cuda.synchronize()
    before = engine.kernel_launches()
    sc.run(verdict, stream=stream)
    torch.cuda.synchronize()
    assert engine.kernel_launches() - before == launches
    st.unchanged("after run")
    return _words(verdict)


def _check_agrees(engine, st, verdicts):
    """verdict[s] == CLEAN exactly where Ragged.check's bad[s] == ~0."""
    bad = torch.zeros(st.S, dtype=torch.int64, device=st.dev.device)
    r = engine.Ragged(st.k, st.rows, st.tbls, st.lens, st.data, st.coding)
    try:
        r.check(bad, 0)
        torch.cuda.synchronize()
    finally:
        r.close()
    bad = bad.cpu().numpy().view(np.uint64)
    for s in range(st.S):
        assert (verdicts[s] == CLEAN) == (int(bad[s]) == 0xFFFFFFFFFFFFFFFF), (s, verdicts[s], hex(int(bad[s])))


def _uniform_agrees(engine, st, verdicts):
    """Every stripe with a length: a uniform Scrub built for it alone gives the same word."""
    k, rows = st.k, st.rows
    for s, n in enumerate(st.lens):
        if not n:
            continue
        word = torch.full((1,), GARBAGE, dtype=torch.int32, device=st.dev.device)
        sc = engine.Scrub(n, k, rows, st.tbls, 1, st.data[s * k:(s + 1) * k], st.coding[s * rows:(s + 1) * rows])
        try:
            sc.run(word, 0)
            torch.cuda.synchronize()
        finally:
            sc.close()
        assert _words(word)[0] == verdicts[s], (s, n, _words(word)[0], verdicts[s])


def _scrub(engine, st, expect=None):
    """Create, run, compare with the model (and with `expect` where the case
    knows its answer), with the ragged check and with uniform scrubs."""
    want = st.want()
    if expect is not None:
        assert want == expect, ("the model disagrees with the case", want, expect)
    sc = engine.Scrub.ragged(st.k, st.rows, st.tbls, st.lens, st.data, st.coding)
    try:
        got = _run(engine, st, sc)
    finally:
        sc.close()
    assert got == want, (got, want)
    for s, n in enumerate(st.lens):
        assert n or got[s] == CLEAN
    _check_agrees(engine, st, got)
    _uniform_agrees(engine, st, got)
    return got


# (stripe, column) for shards 0, 1, ... in turn: the last byte of a byte tail
# behind a full vector in a second tile, the first byte (of a 5-byte stripe),
# a lane's byte 15 (the last byte of the only vector), the last byte of the
# last full vector of a tile, the first byte of a stripe's second tile, the
# last byte of a 15-byte tail in a third tile. Stripe 8 stays untouched.
PLACES = [(0, LENS[0] - 1), (2, 0), (3, 15), (4, TILE - 1), (5, TILE), (7, LENS[7] - 1)]


def _every_shard_in_turn(oracle, gpu, kind, seed):
    k, rows = 4, 2
    st = Stripes(oracle, gpu, kind, k, rows, LENS, seed)
    expect = [CLEAN] * st.S
    for i, (s, col) in enumerate(PLACES):
        st.flip(s, i, col, 1 + 37 * i % 255)
        expect[s] = i
    return st, expect


@pytest.mark.parametrize("kind", ["rs", "cauchy"])
def test_ragged_scrub_names_every_shard_in_turn(engine, oracle, gpu, kind):
    st, expect = _every_shard_in_turn(oracle, gpu, kind, 1)
    assert sorted(v for v in expect if v != CLEAN) == list(range(6)) and expect[8] == CLEAN
    _scrub(engine, st, expect=expect)


def test_ragged_scrub_blames_the_right_stripe(engine, oracle, gpu):
    """Only the last tile of the longest stripe and the 5-byte stripe are
    corrupt: an item that took another stripe's pointers, length or verdict
    word would show in a neighbour."""
    k, rows = 10, 4
    st = Stripes(oracle, gpu, "rs", k, rows, LENS, 2)
    st.flip(7, 6, 2 * TILE + 16 * 100 + 7)
    st.flip(2, k + 1, 4)
    expect = [CLEAN] * st.S
    expect[7], expect[2] = 6, k + 1
    _scrub(engine, st, expect=expect)


def test_ragged_scrub_many_places_and_two_shards(engine, oracle, gpu):
    """rs 10+4: shard 3 in all three tiles of one stripe is still shard 3; two
    shards in different tiles, and a data shard plus a parity row, are MULTI."""
    k, rows = 10, 4
    st = Stripes(oracle, gpu, "rs", k, rows, LENS, 3)
    for col, x in ((5, 0x01), (TILE + 100, 0x80), (2 * TILE + 4000, 0x33), (16 * 9 + 2, 0x7F), (16 * 9 + 11, 0xFF),
                   (LENS[7] - 1, 0x10)):
        st.flip(7, 3, col, x)
    st.flip(5, 2, 77)  # different tiles: two workgroups
    st.flip(5, 7, TILE + 77)
    st.flip(0, 4, 300)  # a data shard and a parity row, the row in the byte tail
    st.flip(0, k + 1, LENS[0] - 2)
    expect = [CLEAN] * st.S
    expect[7], expect[5], expect[0] = 3, MULTI, MULTI
    _scrub(engine, st, expect=expect)


def test_ragged_scrub_wide_pass(engine, oracle, gpu):
    """cauchy 20+8: the widest pass; a data shard, and parity row 7."""
    k, rows = 20, 8
    st = Stripes(oracle, gpu, "cauchy", k, rows, [2 * TILE, 5, TILE + 16], 4)
    st.flip(0, 13, TILE + 16 * 200 + 3)
    st.flip(2, k + 7, TILE + 9)
    _scrub(engine, st, expect=[13, CLEAN, k + 7])


def test_ragged_scrub_all_lengths_zero_enqueues_nothing(engine, oracle, gpu):
    st = Stripes(oracle, gpu, "rs", 10, 4, [0, 0, 0], 5)
    sc = engine.Scrub.ragged(10, 4, st.tbls, st.lens, st.data, st.coding)
    try:
        assert _run(engine, st, sc, launches=0) == [GARBAGE] * 3
    finally:
        sc.close()


def test_ragged_scrub_restore_gives_clean_everywhere(engine, oracle, gpu):
    st, expect = _every_shard_in_turn(oracle, gpu, "rs", 6)
    sc = engine.Scrub.ragged(st.k, st.rows, st.tbls, st.lens, st.data, st.coding)
    try:
        assert _run(engine, st, sc) == expect
        st.restore()
        got = _run(engine, st, sc)
        assert got == [CLEAN] * st.S
        _check_agrees(engine, st, got)
    finally:
        sc.close()


def test_ragged_scrub_is_ordered_on_the_callers_stream(engine, oracle, gpu):
    """A corrupting copy, then the run, queued on a side stream: the run sees
    the corruption. One launch."""
    k, rows = 10, 4
    st = Stripes(oracle, gpu, "rs", k, rows, LENS, 7)
    st.image[4 * st.m + 5, 99] ^= 0x08  # the image only: the device is still clean
    st.image[8 * st.m + k + 3, 16] ^= 0x80
    want = st.want()
    expect = [CLEAN] * st.S
    expect[4], expect[8] = 5, k + 3
    assert want == expect
    staged = torch.from_numpy(st.image.copy()).pin_memory()
    verdict = torch.full((st.S,), GARBAGE, dtype=torch.int32, device=gpu)
    sc = engine.Scrub.ragged(k, rows, st.tbls, st.lens, st.data, st.coding)
    stream = torch.cuda.Stream(device=gpu)
    try:
        torch.cuda.synchronize()
        before = engine.kernel_launches()
        with torch.cuda.stream(stream):
            st.dev.copy_(staged, non_blocking=True)
            sc.run(verdict, stream=stream.cuda_stream)
        stream.synchronize()
        assert engine.kernel_launches() - before == 1
    finally:
        sc.close()
    assert _words(verdict) == want
    st.unchanged("side stream")


def test_ragged_scrub_verdicts_feed_the_ragged_repair(engine, oracle, gpu):
    """Scrub.ragged -> indices -> Repair.ragged over the same lengths: the
    whole allocation equals its uncorrupted image afterwards."""
    st, expect = _every_shard_in_turn(oracle, gpu, "rs", 8)
    k, m = st.k, st.m
    got = _scrub(engine, st, expect=expect)
    errs = [[v] if v not in (CLEAN, MULTI) else [] for v in got]
    assert sum(len(e) for e in errs) == m
    a = oracle.gf_gen_rs_matrix(m, k)
    rp = engine.Repair.ragged(k, m, a, st.lens, errs, st.row)
    try:
        rp.run(0)
        torch.cuda.synchronize()
    finally:
        rp.close()
    assert np.array_equal(st.dev.cpu().numpy(), st.clean)
