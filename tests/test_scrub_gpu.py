"""GPU tier: the scrub batch (include/isal_hip.h) — one launch that names, for
every inconsistent stripe, the one shard that explains its mismatches.

The checker never uses the engine: the parity of the stored sources comes from
oracle.encode, the wanted verdict from the model of tests/test_scrub_cpu.py
(the header's per-column rule, written with the oracle's gf_mul) fed with that
parity. Every stripe of a case lies in one device allocation, each shard
followed by at least 64 guard bytes; after every run the whole allocation is
compared with the host image, since a scrub writes nothing. The verdict words
are prefilled with garbage before each run, and every run is also compared
with Batch.check: verdict CLEAN exactly where bad == ~0.

Sizes: 256 lanes of 16 bytes cover a 4 KiB column tile. LEN is a full tile, a
tile of one vector and a 5-byte tail; no case exceeds three tiles or 9 stripes.
"""
import numpy as np
import pytest
import torch

import ecutil
from test_scrub_cpu import CLEAN, MULTI, _gf, matrix, model_locate, model_verdict

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTES = 0x3C, 64
GARBAGE = 0x5A5A5A5A
TILE = 4096
LEN = TILE + 16 + 5


@pytest.fixture(autouse=True)
def _reload_knobs_after(engine):
    """Knobs are read once by the library: every test leaves it re-synced with
    os.environ."""
    yield
    engine.reload_config()


class Stripes:
    """S encoded stripes in one device allocation, a (S*(k+rows), span) byte
    matrix: shard i of stripe s (data, then parity from the oracle) in row
    s*(k+rows) + i, span = len + a guard of at least 64 bytes, rounded up so
    that every row starts 16-byte aligned. `clean` is the image as encoded,
    `image` what the device holds (flip() changes both)."""

    def __init__(self, oracle, gpu, kind, k, rows, len_, S, seed):
        self.oracle, self.k, self.rows, self.m, self.len, self.S = oracle, k, rows, k + rows, len_, S
        self.coef = matrix(oracle, kind, k, rows)
        self.tbls = oracle.ec_init_tables(k, rows, self.coef)
        self.span = (len_ + GUARD_BYTES + 15) // 16 * 16
        host = np.full((S * self.m, self.span), GUARD, np.uint8)
        for s in range(S):
            data = [ecutil.fill_bytes(len_, seed * 100000 + s * k + j) for j in range(k)]
            parity = oracle.encode(self.coef, k, rows, data) if len_ else [data[0]] * rows
            for i, sh in enumerate(data + parity):
                host[s * self.m + i, :len_] = sh
        self.clean = host
        self.image = host.copy()
        self.dev = torch.from_numpy(host).to(gpu)
        self.row = [int(self.dev[r].data_ptr()) for r in range(host.shape[0])]
        assert all(p % 16 == 0 for p in self.row)
        self.data = [self.row[s * self.m + j] for s in range(S) for j in range(k)]
        self.coding = [self.row[s * self.m + k + l] for s in range(S) for l in range(rows)]

    def flip(self, s, shard, col, x=0x40):
        """XOR x into byte col of shard `shard` of stripe s, on the device and in the image."""
        assert 0 <= col < self.len and x
        self.image[s * self.m + shard, col] ^= x
        self.dev[s * self.m + shard, col] ^= x

    def restore(self):
        self.image = self.clean.copy()
        self.dev.copy_(torch.from_numpy(self.clean))
        torch.cuda.synchronize()

    def want(self):
        """The model's verdict per stripe for the image as it stands."""
        out = []
        for s in range(self.S):
            rows_ = self.image[s * self.m:(s + 1) * self.m, :self.len]
            if not self.len:
                out.append(CLEAN)
                continue
            true = self.oracle.encode(self.coef, self.k, self.rows, [rows_[j].copy() for j in range(self.k)])
            out.append(model_verdict(self.oracle, self.coef, self.k, self.rows, list(rows_[self.k:]), true))
        return out

    def unchanged(self, what):
        got = self.dev.cpu().numpy()
        if not np.array_equal(got, self.image):
            r = int(np.nonzero((got != self.image).any(axis=1))[0][0])
            s, i = divmod(r, self.m)
            raise AssertionError(f"{what}: the scrub wrote to stripe {s} shard {i} or its guard")


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
    return [int(v) for v in verdict.cpu().numpy().view(np.uint32)]


def _check_agrees(engine, st, verdicts):
    """verdict[s] == CLEAN exactly where Batch.check's bad[s] == ~0."""
    bad = torch.zeros(st.S, dtype=torch.int64, device=st.dev.device)
    b = engine.Batch(st.len, st.k, st.rows, st.tbls, st.S, st.data, st.coding)
    try:
        b.check(bad, 0)
        torch.cuda.synchronize()
    finally:
        b.close()
    bad = bad.cpu().numpy().view(np.uint64)
    for s in range(st.S):
        assert (verdicts[s] == CLEAN) == (int(bad[s]) == 0xFFFFFFFFFFFFFFFF), (s, verdicts[s], hex(int(bad[s])))


def _scrub(engine, st, expect=None):
    """Create, run, compare with the model (and with `expect` where the case
    knows its answer), compare with the check."""
    want = st.want()
    if expect is not None:
        assert want == expect, ("the model disagrees with the case", want, expect)
    sc = engine.Scrub(st.len, st.k, st.rows, st.tbls, st.S, st.data, st.coding)
    try:
        got = _run(engine, st, sc)
    finally:
        sc.close()
    assert got == want, (got, want)
    _check_agrees(engine, st, got)
    return got


# first byte, a lane's byte 15, the last full vector, the last byte of the tail, ...
PLACES = [0, 16 * 37 + 15, TILE + 3, LEN - 1, TILE + 16, 16 * 255 + 8, TILE - 1, 16 * 128]


def _every_shard_in_turn(oracle, gpu, kind, k, rows, seed):
    st = Stripes(oracle, gpu, kind, k, rows, LEN, k + rows + 1, seed)
    for i in range(k + rows):
        st.flip(i, i, PLACES[i % len(PLACES)], 1 + 37 * i % 255)
    return st


@pytest.mark.parametrize("kind", ["rs", "cauchy"])
def test_scrub_names_every_shard_in_turn(engine, oracle, gpu, kind):
    k, rows = 4, 2
    st = _every_shard_in_turn(oracle, gpu, kind, k, rows, 1)
    _scrub(engine, st, expect=list(range(k + rows)) + [CLEAN])


@pytest.mark.parametrize("xor", ["1", "0"])
def test_scrub_pq_matrix_with_and_without_the_xor_form(engine, oracle, gpu, monkeypatch, xor):
    monkeypatch.setenv("ISAL_HIP_ENC_XOR", xor)
    engine.reload_config()
    k, rows = 6, 2
    st = _every_shard_in_turn(oracle, gpu, "pq", k, rows, 2)
    _scrub(engine, st, expect=list(range(k + rows)) + [CLEAN])


def test_scrub_same_shard_in_many_places(engine, oracle, gpu):
    """Shard 3 of rs 10+4 flipped in three different tiles and twice within
    one lane (two dwords, and two bytes of one dword): still shard 3."""
    st = Stripes(oracle, gpu, "rs", 10, 4, 3 * TILE, 2, 3)
    for col, x in ((5, 0x01), (TILE + 100, 0x80), (2 * TILE + 4000, 0x33), (16 * 9 + 2, 0x7F), (16 * 9 + 3, 0x10),
                   (16 * 9 + 11, 0xFF)):
        st.flip(0, 3, col, x)
    _scrub(engine, st, expect=[3, CLEAN])


def test_scrub_two_shards_give_multi(engine, oracle, gpu):
    k, rows = 10, 4
    st = Stripes(oracle, gpu, "rs", k, rows, 2 * TILE, 5, 4)
    st.flip(0, 2, 77)  # different tiles: two workgroups
    st.flip(0, 7, TILE + 77)
    st.flip(1, 2, 16 * 10 + 1)  # two lanes of one tile
    st.flip(1, 7, 16 * 200 + 1)
    st.flip(2, 1, 1234, 0x21)  # one byte column: with four rows no single shard explains it
    st.flip(2, 8, 1234, 0xC4)
    st.flip(3, 4, 300)  # a data shard and a parity row
    st.flip(3, k + 1, 5000)
    _scrub(engine, st, expect=[MULTI, MULTI, MULTI, MULTI, CLEAN])


def test_scrub_two_shards_can_imitate_a_third_with_two_rows(engine, oracle, gpu):
    """The documented limit, pinned: with rows = 2, flips of two shards in one
    byte column whose syndromes add up to a multiple of a third shard's column
    are reported as that third shard. The flips are found by search."""
    k, rows = 4, 2
    st = Stripes(oracle, gpu, "rs", k, rows, LEN, 2, 5)
    mul, _ = _gf(oracle)
    a, b = 0, 2
    found = None
    for xa in range(1, 256):
        for xb in range(1, 256):
            e = [int(mul[int(st.coef[l * k + a]), xa]) ^ int(mul[int(st.coef[l * k + b]), xb]) for l in range(rows)]
            c = model_locate(oracle, st.coef, k, rows, e)
            if c not in (CLEAN, MULTI, a, b):
                found = (xa, xb, c)
                break
        if found:
            break
    assert found, "no imitation among 255 x 255 flips of shards 0 and 2"
    xa, xb, c = found
    st.flip(0, a, TILE + 16 + 2, xa)  # in the byte tail
    st.flip(0, b, TILE + 16 + 2, xb)
    _scrub(engine, st, expect=[c, CLEAN])


def test_scrub_wide_pass(engine, oracle, gpu):
    """cauchy 20+8: the widest pass; a data shard, and parity row 7."""
    k, rows = 20, 8
    st = Stripes(oracle, gpu, "cauchy", k, rows, 2 * TILE, 3, 6)
    st.flip(0, 13, TILE + 16 * 200 + 3)
    st.flip(1, k + 7, 16 * 100 + 9)
    _scrub(engine, st, expect=[13, k + 7, CLEAN])


@pytest.mark.parametrize("len_", [5, 16])
def test_scrub_short_shards(engine, oracle, gpu, len_):
    """A byte tail alone, one 16-byte lane alone."""
    k, rows = 10, 4
    st = Stripes(oracle, gpu, "rs", k, rows, len_, 3, 7 + len_)
    st.flip(0, 6, len_ - 1)
    st.flip(2, k + 2, 0)
    _scrub(engine, st, expect=[6, CLEAN, k + 2])


def test_scrub_len_zero_enqueues_nothing(engine, oracle, gpu):
    st = Stripes(oracle, gpu, "rs", 10, 4, 0, 3, 8)
    sc = engine.Scrub(0, 10, 4, st.tbls, 3, st.data, st.coding)
    try:
        assert _run(engine, st, sc, launches=0) == [GARBAGE] * 3
    finally:
        sc.close()


def test_scrub_restore_gives_clean_everywhere(engine, oracle, gpu):
    k, rows = 4, 2
    st = _every_shard_in_turn(oracle, gpu, "rs", k, rows, 9)
    sc = engine.Scrub(st.len, k, rows, st.tbls, st.S, st.data, st.coding)
    try:
        assert _run(engine, st, sc) == list(range(k + rows)) + [CLEAN]
        st.restore()
        got = _run(engine, st, sc)
        assert got == [CLEAN] * st.S
        _check_agrees(engine, st, got)
    finally:
        sc.close()


def test_scrub_verdicts_feed_the_repair_batch(engine, oracle, gpu):
    """Scrub.run -> indices -> Repair(nerrs=1): every stripe equals its
    uncorrupted image afterwards."""
    k, rows = 4, 2
    m = k + rows
    st = _every_shard_in_turn(oracle, gpu, "rs", k, rows, 10)
    got = _scrub(engine, st, expect=list(range(m)) + [CLEAN])
    bad = [s for s in range(st.S) if got[s] not in (CLEAN, MULTI)]
    assert bad == list(range(m))
    a = oracle.gf_gen_rs_matrix(m, k)
    rp = engine.Repair(st.len, k, m, a, 1, len(bad), [got[s] for s in bad],
                       [st.row[s * m + i] for s in bad for i in range(m)])
    try:
        rp.run(0)
        torch.cuda.synchronize()
    finally:
        rp.close()
    assert np.array_equal(st.dev.cpu().numpy(), st.clean)


def test_scrub_is_ordered_on_the_callers_stream(engine, oracle, gpu):
    """A corrupting copy, then the run, queued on a side stream: the run sees
    the corruption. One launch."""
    k, rows = 10, 4
    st = Stripes(oracle, gpu, "rs", k, rows, LEN, 4, 11)
    st.image[1 * st.m + 5, 99] ^= 0x08  # the image only: the device is still clean
    st.image[3 * st.m + k + 3, LEN - 2] ^= 0x80
    want = st.want()
    assert want == [CLEAN, 5, CLEAN, k + 3]
    staged = torch.from_numpy(st.image.copy()).pin_memory()
    verdict = torch.full((st.S,), GARBAGE, dtype=torch.int32, device=gpu)
    sc = engine.Scrub(st.len, k, rows, st.tbls, st.S, st.data, st.coding)
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
    assert [int(v) for v in verdict.cpu().numpy().view(np.uint32)] == want
    st.unchanged("side stream")
