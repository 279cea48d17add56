"""GPU tier: the ragged CRC64 checksum (include/isal_hip.h isal_hip_ragged_crc64,
isal_hip_ragged_encode_crc64) — any crc64_* flavour of every shard of stripes
of different lengths in one pass launch and one combine launch.

The checker is oracle.crc64(variant, shard, init) per shard with that stripe's
own length, never the engine's own output. The layout is test_ragged_gpu's:
every stripe of a case in one device allocation, 64 guard bytes after every
shard; the words lie inside a larger device array with sentinel words on both
sides. After every call the whole shard allocation and the sentinels are
compared: a checksum writes no shard byte and no word outside crc.

Lengths: with ISAL_HIP_CRC_TILES=2 a block is B = 2 tiles of T = 4096 bytes, so
shards of a few KiB reach every branch of the pass (full tiles through F'_u and
F_u, a last block with 0, 1 or 2 full tiles) and of the combine (Horner over
blocks, the last block through the ring product, a tail of whole chunks, of
bytes, of both, of neither). The 15 listed lengths are 20 blocks of one shard.
Work items are (block, shard) and a workgroup takes two: the order that ends
with the empty stripe has a 7-byte stripe more, 21 blocks, so with an odd shard
count (3+2, 1+2, 4+9) the last workgroup has one item and pairs straddle
blocks of different tile counts; the 16-stripe order has 24 blocks, a multiple
of 8.
"""
import functools
import random

import numpy as np
import pytest
import torch

import ecutil
from test_ragged_crc_gpu import KNOB, tiles2  # noqa: F401  (the ISAL_HIP_CRC_TILES=2 fixture)
from test_ragged_gpu import POISON, Stripes, _reference, shuffled

pytestmark = pytest.mark.gpu

T = 4096
B = 2 * T
SENTINEL, PAD = 0x7E57C0DE7E57C0DE, 16
GARBAGE = 0x5A5A5A5A5A5A5A5A
CRC_LAUNCHES = 2  # the header's count: one pass, one combine

LENS15 = [0, 1, 5, 15, 16, 17, T - 1, T, T + 1, T + 16, B, B + 1, B + T, 2 * B + 55, 3 * B]
ROCKSOFT_REFL, ECMA_NORM = 6, 1  # CRC64NVME, and a norm flavour (isal_hip.h ISAL_HIP_CRC64_*)
# (k, rows, variant), all rs: every flavour on 10+4; the odd shard counts, and rows = 9 (two encode passes)
CASES = [(10, 4, v) for v in range(8)] + [(k, rows, v) for k, rows in [(3, 2), (1, 2), (4, 9)]
                                          for v in (ROCKSOFT_REFL, ECMA_NORM)]
INITS = [0, 0xFFFFFFFFFFFFFFFF, random.Random(43).getrandbits(64)]


def _blocks(lens, block=B):
    return sum((n + block - 1) // block for n in lens)


def orders():
    out = [shuffled(LENS15, 18), shuffled(LENS15 + [7], 31), shuffled(LENS15 + [3 * B + T + 16], 9)]
    assert out[0][0] == 0 and out[1][-1] == 0
    assert _blocks(out[0]) % 8 and _blocks(out[1]) % 2 == 1
    assert _blocks(out[2]) % 8 == 0 and len(out[2]) == 16
    return out


@functools.lru_cache(maxsize=None)
def _oracle_words(k, rows, lens, seed, variant, init):
    """The oracle's checksum of every shard of the encoded case (oracle parity),
    stripe-major, sources then parity; computed once per case, variant and init."""
    o = ecutil.oracle()
    off, want, _, _, _ = _reference("rs", k, rows, lens, seed)
    out = np.array([o.crc64(variant, want[off[s][i]:off[s][i] + n], init)
                    for s, n in enumerate(lens) for i in range(k + rows)], dtype=np.uint64)
    out.setflags(write=False)
    return out


def _image_words(oracle, st, variant, init):
    """The oracle's checksums of what the device holds now (st.image)."""
    return np.array([oracle.crc64(variant, st.image[st.off[s][i]:st.off[s][i] + n], init)
                     for s, n in enumerate(st.lens) for i in range(st.m)], dtype=np.uint64)


def _i64(x):
    return x - (1 << 64) if x >> 63 else x


class Words:
    """nstripes*(k+rows) garbage 64-bit words between PAD sentinel words on each side."""

    def __init__(self, st):
        self.n = st.S * st.m
        self.dev = torch.empty(self.n + 2 * PAD, dtype=torch.int64, device=st.dev.device)
        self.crc = self.dev[PAD:PAD + self.n]
        self.garbage()

    def garbage(self):
        self.dev.fill_(_i64(SENTINEL))
        self.crc.fill_(_i64(GARBAGE))

    def read(self, what):
        got = self.dev.cpu().numpy().view(np.uint64)
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
        raise AssertionError(f"{what}: stripe {s} (len {st.lens[s]}) shard {i}: got {int(got[pos]):#018x}, "
                             f"want {int(want[pos]):#018x}")


@pytest.mark.parametrize("order", range(3))
@pytest.mark.parametrize("k,rows,variant", CASES)
def test_ragged_crc64_matches_the_oracle_per_shard(engine, gpu, tiles2, k, rows, variant, order):
    """Every word equals the oracle's for three init values; a stripe of length
    0 yields init; a second call over garbage rewrites every word; two
    launches per call; nothing but crc is written."""
    lens = orders()[order]
    seed = 500 + order
    st = Stripes(gpu, "rs", k, rows, lens, seed, encoded=True)
    rg = engine.Ragged(k, rows, st.tbls, lens, st.data, st.coding)
    words = Words(st)
    zero = lens.index(0)
    try:
        for init in INITS:
            want = _oracle_words(k, rows, tuple(lens), seed, variant, init)
            assert (want[zero * st.m:(zero + 1) * st.m] == init).all()
            for run in ("first call", "second call"):
                what = f"variant {variant} init {init:#x} {run}"
                got = _run(engine, st, words, lambda crc, s: rg.crc64(variant, init, crc, s), CRC_LAUNCHES, what)
                _expect(got, want, st, what)
    finally:
        rg.close()


@pytest.mark.parametrize("order", range(3))
@pytest.mark.parametrize("k,rows", [(10, 4), (3, 2), (1, 2), (4, 9)])
def test_ragged_encode_crc64_is_encode_then_crc64(engine, gpu, tiles2, k, rows, order):
    """From poisoned parity: the shards end byte-identical to Ragged.encode's
    (and to the oracle's parity), the words are the oracle's checksums of oracle
    parity, the launches are the encode's plus the checksum's."""
    lens = orders()[order]
    seed = 500 + order
    init = INITS[order]
    variant = (ROCKSOFT_REFL, ECMA_NORM)[(order + rows) % 2]
    st = Stripes(gpu, "rs", k, rows, lens, seed)
    rg = engine.Ragged(k, rows, st.tbls, lens, st.data, st.coding)
    words = Words(st)
    try:
        st.image = st.want.copy()  # what the device must hold after the call
        got = _run(engine, st, words, lambda crc, s: rg.encode_crc64(variant, init, crc, s),
                   _passes(rows) + CRC_LAUNCHES, "encode_crc64")
        _expect(got, _oracle_words(k, rows, tuple(lens), seed, variant, init), st, "encode_crc64")
        fused = st.dev.cpu().numpy()
        st.dev.copy_(torch.from_numpy(st.poisoned.copy()))
        rg.encode(0)
        torch.cuda.synchronize()
        assert np.array_equal(st.dev.cpu().numpy(), fused), "encode_crc64 and encode leave different shards"
    finally:
        rg.close()


def test_ragged_crc64_variants_alternate_on_one_object(engine, gpu, tiles2):
    """Each variant's image is built at its first use and kept: two flavours
    (and then all eight) used in turn on one object all stay right."""
    k, rows, seed, init = 3, 2, 501, INITS[2]
    lens = orders()[1]
    st = Stripes(gpu, "rs", k, rows, lens, seed, encoded=True)
    rg = engine.Ragged(k, rows, st.tbls, lens, st.data, st.coding)
    words = Words(st)
    try:
        for variant in [ROCKSOFT_REFL, ECMA_NORM, ROCKSOFT_REFL, ECMA_NORM] + list(range(8)) + [ROCKSOFT_REFL]:
            got = _run(engine, st, words, lambda crc, s: rg.crc64(variant, init, crc, s), CRC_LAUNCHES, f"variant {variant}")
            _expect(got, _oracle_words(k, rows, tuple(lens), seed, variant, init), st, f"variant {variant}")
    finally:
        rg.close()


def test_ragged_crc64_and_crc32c_do_not_disturb_each_other(engine, oracle, gpu, tiles2):
    """The two checksum states of one object are independent: CRC32C, CRC64,
    CRC32C, CRC64, each against its oracle."""
    k, rows, seed = 10, 4, 502
    lens = orders()[2]
    st = Stripes(gpu, "rs", k, rows, lens, seed, encoded=True)
    rg = engine.Ragged(k, rows, st.tbls, lens, st.data, st.coding)
    words = Words(st)
    words32 = torch.empty(st.S * st.m, dtype=torch.int32, device=gpu)
    init32 = 0x1B2E3D4C
    want32 = np.array([oracle.crc32_iscsi(st.want[st.off[s][i]:st.off[s][i] + n], init32)
                       for s, n in enumerate(lens) for i in range(st.m)], dtype=np.uint32)
    try:
        for turn in range(2):
            words32.fill_(0x5A5A5A5A)
            rg.crc(init32, words32, 0)
            torch.cuda.synchronize()
            assert np.array_equal(words32.cpu().numpy().view(np.uint32), want32), f"crc32c, turn {turn}"
            got = _run(engine, st, words, lambda crc, s: rg.crc64(ROCKSOFT_REFL, INITS[turn], crc, s), CRC_LAUNCHES,
                       f"crc64, turn {turn}")
            _expect(got, _oracle_words(k, rows, tuple(lens), seed, ROCKSOFT_REFL, INITS[turn]), st, f"crc64, turn {turn}")
    finally:
        rg.close()


def test_ragged_crc64_default_block_size(engine, gpu):
    """Without the knob: a stripe of more than two default blocks (128 tiles
    each at the most) and a 55-byte tail, beside a 5-byte and an empty stripe."""
    import os
    before = os.environ.pop(KNOB, None)
    engine.lib().isal_hip_config_reload()
    k, rows, seed, init = 3, 2, 78, INITS[2]
    lens = [2 * 128 * T + 55, 5, 0]
    try:
        st = Stripes(gpu, "rs", k, rows, lens, seed, encoded=True)
        rg = engine.Ragged(k, rows, st.tbls, lens, st.data, st.coding)
        words = Words(st)
        try:
            for variant in (ROCKSOFT_REFL, ECMA_NORM):
                got = _run(engine, st, words, lambda crc, s: rg.crc64(variant, init, crc, s), CRC_LAUNCHES, "default block")
                _expect(got, _oracle_words(k, rows, tuple(lens), seed, variant, init), st, "default block")
        finally:
            rg.close()
    finally:
        if before is not None:
            os.environ[KNOB] = before
        engine.lib().isal_hip_config_reload()


def test_ragged_crc64_all_zero_lengths_enqueue_nothing(engine, gpu, tiles2):
    k, rows = 10, 4
    st = Stripes(gpu, "rs", k, rows, [0, 0, 0], 7)
    rg = engine.Ragged(k, rows, st.tbls, st.lens, st.data, st.coding)
    words = Words(st)
    try:
        for call in (rg.crc64, rg.encode_crc64):
            got = _run(engine, st, words, lambda crc, s: call(ROCKSOFT_REFL, 0x1234, crc, s), 0, "all lengths zero")
            assert (got == GARBAGE).all(), "crc written although every length is 0"
    finally:
        rg.close()


def test_ragged_crc64_is_ordered_behind_encode_on_one_stream(engine, gpu, tiles2):
    """encode, then crc64, on one non-default stream with nothing between them:
    the parity words are those of the fresh parity."""
    k, rows, seed, init, variant = 10, 4, 502, INITS[1], ECMA_NORM
    lens = orders()[2]
    st = Stripes(gpu, "rs", k, rows, lens, seed)
    rg = engine.Ragged(k, rows, st.tbls, lens, st.data, st.coding)
    words = Words(st)
    stream = torch.cuda.Stream(device=gpu)
    try:
        torch.cuda.synchronize()
        rg.encode(stream.cuda_stream)
        rg.crc64(variant, init, words.crc, stream.cuda_stream)
        stream.synchronize()
        st.same("after encode and crc64", st.want)
        got = words.read("side stream")
        want = _oracle_words(k, rows, tuple(lens), seed, variant, init)
        _expect(got, want, st, "side stream")
        parity = [s * st.m + k + l for s, n in enumerate(lens) if n for l in range(rows)]
        poisoned = np.array([ecutil.oracle().crc64(variant, np.full(n, POISON, np.uint8), init)
                             for n in lens if n for _ in range(rows)], dtype=np.uint64)
        assert (want[parity] != poisoned).all(), "the case cannot tell fresh parity from poison"
    finally:
        rg.close()


def test_ragged_crc64_after_corruption_changes_exactly_that_shards_word(engine, oracle, gpu, tiles2):
    """What the scrub contract asks callers for: one flipped byte changes the
    word of its shard and no other."""
    k, rows, seed, init, variant = 10, 4, 501, INITS[2], ROCKSOFT_REFL
    lens = orders()[1]
    st = Stripes(gpu, "rs", k, rows, lens, seed, encoded=True)
    rg = engine.Ragged(k, rows, st.tbls, lens, st.data, st.coding)
    words = Words(st)
    try:
        clean = _run(engine, st, words, lambda crc, s: rg.crc64(variant, init, crc, s), CRC_LAUNCHES, "clean")
        _expect(clean, _oracle_words(k, rows, tuple(lens), seed, variant, init), st, "clean")
        places = [(lens.index(2 * B + 55), k - 1, 2 * B + 54),  # the last byte of a byte tail, third block
                  (lens.index(2 * B + 55), 0, 2 * B + 16),      # the tail's second whole chunk
                  (lens.index(B + T), k + rows - 1, B + 16 * 255 + 3),  # a parity shard, the last block's full tile
                  (lens.index(3 * B), 2, 5),                    # the first block of three, Horner twice
                  (lens.index(1), 0, 0)]
        for s, shard, col in places:
            st.flip(s, shard, col)
            got = _run(engine, st, words, lambda crc, s_: rg.crc64(variant, init, crc, s_), CRC_LAUNCHES, "corrupt")
            _expect(got, _image_words(oracle, st, variant, init), st, "corrupt")
            assert [int(p) for p in np.nonzero(got != clean)[0]] == [s * st.m + shard], (s, shard, col)
            st.restore()
    finally:
        rg.close()
