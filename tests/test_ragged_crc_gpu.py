"""GPU tier: the ragged checksum (include/isal_hip.h isal_hip_ragged_crc,
isal_hip_ragged_encode_crc) — crc32_iscsi of every shard of stripes of
different lengths in one pass launch and one combine launch.

The checker is oracle.crc32_iscsi per shard with that stripe's own length,
never the engine's own output. The layout is test_ragged_gpu's: every stripe of
a case in one device allocation, 64 guard bytes after every shard; the words
lie inside a larger device array with sentinel words on both sides. After every
call the whole shard allocation and the sentinels are compared: a checksum
writes no shard byte and no word outside crc.

Lengths: with ISAL_HIP_CRC_TILES=2 a block is B = 2 tiles of T = 4096 bytes, so
shards of a few KiB reach every branch of the pass (full tiles through F' and
F, the ragged tile, the straddling lane) and of the combine (Horner over
blocks, the last block with 0, 1 or 2 full tiles, with and without a tail).
13 stripes are 18 blocks of one shard; the 16-stripe order has 24, a multiple
of 8.
"""
import functools
import os
import random

import numpy as np
import pytest
import torch

import ecutil
from test_ragged_gpu import POISON, Stripes, _reference, shuffled

pytestmark = pytest.mark.gpu

T = 4096
B = 2 * T
KNOB = "ISAL_HIP_CRC_TILES"
SENTINEL, PAD = 0x7E57C0DE, 16
GARBAGE = 0x5A5A5A5A
CRC_LAUNCHES = 2  # the header's count: one pass, one combine

LENS13 = [0, 1, 5, 16, T - 1, T, T + 1, T + 16, B, B + 1, B + T, 2 * B + 3 * 16 + 7, 3 * B]
LENS16 = LENS13 + [B + T + 16, 2 * B + 1, 7]
GEOMETRIES = [(10, 4), (3, 2), (1, 2), (4, 9)]  # (k, rows), all rs; rows = 9 is two encode passes
INITS = [0, 0xFFFFFFFF, random.Random(41).getrandbits(32)]


def _blocks(lens, block=B):
    return sum((n + block - 1) // block for n in lens)


def orders():
    out = [shuffled(LENS13, 18), shuffled(LENS13, 2), shuffled(LENS16, 9)]
    assert out[0][0] == 0 and out[1][-1] == 0
    assert _blocks(out[0]) % 8 and _blocks(out[2]) % 8 == 0 and len(out[2]) == 16
    return out


@pytest.fixture
def tiles2(engine):
    """ISAL_HIP_CRC_TILES=2 for the objects a test creates, put back after it."""
    before = os.environ.get(KNOB)
    os.environ[KNOB] = "2"
    engine.lib().isal_hip_config_reload()
    try:
        yield
    finally:
        if before is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = before
        engine.lib().isal_hip_config_reload()


@functools.lru_cache(maxsize=None)
def _oracle_words(k, rows, lens, seed, init):
    """The oracle's checksum of every shard of the encoded case (oracle parity),
    stripe-major, sources then parity; computed once per case and init."""
    o = ecutil.oracle()
    off, want, _, _, _ = _reference("rs", k, rows, lens, seed)
    out = np.array([o.crc32_iscsi(want[off[s][i]:off[s][i] + n], init)
                    for s, n in enumerate(lens) for i in range(k + rows)], dtype=np.uint32)
    out.setflags(write=False)
    return out


def _image_words(oracle, st, init):
    """The oracle's checksums of what the device holds now (st.image)."""
    return np.array([oracle.crc32_iscsi(st.image[st.off[s][i]:st.off[s][i] + n], init)
                     for s, n in enumerate(st.lens) for i in range(st.m)], dtype=np.uint32)


class Words:
    """nstripes*(k+rows) garbage words between PAD sentinel words on each side."""

    def __init__(self, st):
        self.n = st.S * st.m
        self.dev = torch.empty(self.n + 2 * PAD, dtype=torch.int32, device=st.dev.device)
        self.crc = self.dev[PAD:PAD + self.n]
        self.garbage()

    def garbage(self):
        self.dev.fill_(SENTINEL)
        self.crc.fill_(GARBAGE)

    def read(self, what):
        got = self.dev.cpu().numpy().view(np.uint32)
        assert (got[:PAD] == SENTINEL).all() and (got[PAD + self.n:] == SENTINEL).all(), f"{what}: a sentinel word written"
        return got[PAD:PAD + self.n].copy()


def _passes(rows):
    return (rows + 7) // 8


def _run(engine, st, words, call, launches, what, stream=0):
    """One call over garbage words: the launch count, no shard byte and no
    sentinel written; returns the words."""
    words.garbage()
    torch.cuda.synchronize()
    before = engine.kernel_launches()
    call(words.crc, stream)
    torch.cuda.synchronize()
    assert engine.kernel_launches() - before == launches, what
    st.same(what)
    return words.read(what)


def _expect(got, want, st, what):
    if not np.array_equal(got, want):
        pos = int(np.nonzero(got != want)[0][0])
        s, i = divmod(pos, st.m)
        raise AssertionError(f"{what}: stripe {s} (len {st.lens[s]}) shard {i}: got {got[pos]:#010x}, want {want[pos]:#010x}")


@pytest.mark.parametrize("order", range(3))
@pytest.mark.parametrize("k,rows", GEOMETRIES)
def test_ragged_crc_matches_the_oracle_per_shard(engine, gpu, tiles2, k, rows, order):
    """Every word equals the oracle's for three init values; a stripe of length
    0 yields init; a second call over garbage rewrites every word; two
    launches per call; nothing but crc is written."""
    lens = orders()[order]
    seed = 400 + order
    st = Stripes(gpu, "rs", k, rows, lens, seed, encoded=True)
    rg = engine.Ragged(k, rows, st.tbls, lens, st.data, st.coding)
    words = Words(st)
    zero = lens.index(0)
    try:
        for init in INITS:
            want = _oracle_words(k, rows, tuple(lens), seed, init)
            assert (want[zero * st.m:(zero + 1) * st.m] == init).all()
            for run in ("first call", "second call"):
                got = _run(engine, st, words, lambda crc, s: rg.crc(init, crc, s), CRC_LAUNCHES, f"init {init:#x} {run}")
                _expect(got, want, st, f"init {init:#x} {run}")
    finally:
        rg.close()


@pytest.mark.parametrize("order", range(3))
@pytest.mark.parametrize("k,rows", GEOMETRIES)
def test_ragged_encode_crc_is_encode_then_crc(engine, gpu, tiles2, k, rows, order):
    """From poisoned parity: the shards end byte-identical to Ragged.encode's
    (and to the oracle's parity), the words are the oracle's checksums of oracle
    parity, the launches are the encode's plus the checksum's."""
    lens = orders()[order]
    seed = 400 + order
    init = INITS[order]
    st = Stripes(gpu, "rs", k, rows, lens, seed)
    rg = engine.Ragged(k, rows, st.tbls, lens, st.data, st.coding)
    words = Words(st)
    try:
        st.image = st.want.copy()  # what the device must hold after the call
        got = _run(engine, st, words, lambda crc, s: rg.encode_crc(init, crc, s), _passes(rows) + CRC_LAUNCHES,
                   "encode_crc")
        _expect(got, _oracle_words(k, rows, tuple(lens), seed, init), st, "encode_crc")
        fused = st.dev.cpu().numpy()
        st.dev.copy_(torch.from_numpy(st.poisoned.copy()))
        rg.encode(0)
        torch.cuda.synchronize()
        assert np.array_equal(st.dev.cpu().numpy(), fused), "encode_crc and encode leave different shards"
    finally:
        rg.close()


def test_ragged_crc_default_block_size(engine, gpu):
    """Without the knob: a stripe of more than two default blocks (64 tiles
    each at the most) and a 7-byte tail, beside a 5-byte and an empty stripe."""
    before = os.environ.pop(KNOB, None)
    engine.lib().isal_hip_config_reload()
    k, rows, seed, init = 3, 2, 77, INITS[2]
    lens = [2 * 64 * T + 7, 5, 0]
    try:
        st = Stripes(gpu, "rs", k, rows, lens, seed, encoded=True)
        rg = engine.Ragged(k, rows, st.tbls, lens, st.data, st.coding)
        words = Words(st)
        try:
            got = _run(engine, st, words, lambda crc, s: rg.crc(init, crc, s), CRC_LAUNCHES, "default block")
            _expect(got, _oracle_words(k, rows, tuple(lens), seed, init), st, "default block")
        finally:
            rg.close()
    finally:
        if before is not None:
            os.environ[KNOB] = before
        engine.lib().isal_hip_config_reload()


def test_ragged_crc_all_zero_lengths_enqueue_nothing(engine, gpu, tiles2):
    k, rows = 10, 4
    st = Stripes(gpu, "rs", k, rows, [0, 0, 0], 7)
    rg = engine.Ragged(k, rows, st.tbls, st.lens, st.data, st.coding)
    words = Words(st)
    try:
        for call in (rg.crc, rg.encode_crc):
            got = _run(engine, st, words, lambda crc, s: call(0x1234, crc, s), 0, "all lengths zero")
            assert (got == GARBAGE).all(), "crc written although every length is 0"
    finally:
        rg.close()


def test_ragged_crc_is_ordered_behind_encode_on_one_stream(engine, gpu, tiles2):
    """encode, then crc, on one non-default stream with nothing between them:
    the parity words are those of the fresh parity."""
    k, rows, seed, init = 10, 4, 402, INITS[1]
    lens = orders()[2]
    st = Stripes(gpu, "rs", k, rows, lens, seed)
    rg = engine.Ragged(k, rows, st.tbls, lens, st.data, st.coding)
    words = Words(st)
    stream = torch.cuda.Stream(device=gpu)
    try:
        torch.cuda.synchronize()
        rg.encode(stream.cuda_stream)
        rg.crc(init, words.crc, stream.cuda_stream)
        stream.synchronize()
        st.same("after encode and crc", st.want)
        got = words.read("side stream")
        want = _oracle_words(k, rows, tuple(lens), seed, init)
        _expect(got, want, st, "side stream")
        parity = [s * st.m + k + l for s, n in enumerate(lens) if n for l in range(rows)]
        poisoned = np.array([ecutil.oracle().crc32_iscsi(np.full(n, POISON, np.uint8), init)
                             for n in lens if n for _ in range(rows)], dtype=np.uint32)
        assert (want[parity] != poisoned).all(), "the case cannot tell fresh parity from poison"
    finally:
        rg.close()


def test_ragged_crc_after_corruption_changes_exactly_that_shards_word(engine, oracle, gpu, tiles2):
    """What the scrub contract asks callers for: one flipped byte changes the
    word of its shard and no other."""
    k, rows, seed, init = 10, 4, 401, INITS[2]
    lens = orders()[1]
    st = Stripes(gpu, "rs", k, rows, lens, seed, encoded=True)
    rg = engine.Ragged(k, rows, st.tbls, lens, st.data, st.coding)
    words = Words(st)
    try:
        clean = _run(engine, st, words, lambda crc, s: rg.crc(init, crc, s), CRC_LAUNCHES, "clean")
        _expect(clean, _oracle_words(k, rows, tuple(lens), seed, init), st, "clean")
        places = [(lens.index(2 * B + 55), k - 1, 2 * B + 54),  # the last byte of a byte tail, third block
                  (lens.index(B + T), k + rows - 1, B + 16 * 255 + 3),  # a parity shard, the last block's full tile
                  (lens.index(1), 0, 0)]
        for s, shard, col in places:
            st.flip(s, shard, col)
            got = _run(engine, st, words, lambda crc, s_: rg.crc(init, crc, s_), CRC_LAUNCHES, "corrupt")
            _expect(got, _image_words(oracle, st, init), st, "corrupt")
            assert [int(p) for p in np.nonzero(got != clean)[0]] == [s * st.m + shard], (s, shard, col)
            st.restore()
    finally:
        rg.close()
