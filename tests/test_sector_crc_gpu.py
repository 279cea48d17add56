"""GPU tier: sector checksums (include/isal_hip.h isal_hip_batch_sector_crc,
isal_hip_ragged_sector_crc and their crc64 forms) — one word per 512 B .. 4 KiB
sector of every shard, in one launch.

The checker is the oracle's crc32_iscsi / crc64_<variant>, called once per
sector on the host over that sector's bytes alone, never the engine's own
output. The layout is test_ragged_gpu's: every stripe of a case in one device
allocation, 64 guard bytes after every shard; the words lie inside a larger
device array with sentinel words on both sides. After every call the whole
shard allocation and the sentinels are compared: a checksum writes no shard
byte and no word outside crc.

Lengths: with T = 4096 (the tile) and S the sector, LENS(S) reaches every
boundary the kernel has: a sector of fewer than 16 bytes (no whole chunk: the
byte loop starts at init), exactly one chunk, a chunk and a byte tail, a short
last sector with and without a byte tail, a last sector in a tile of its own,
tiles whose later sectors do not exist, and whole tiles. Sectors of 512 and
1024 bytes are joined inside a wave, 2048 and 4096 also across waves through
LDS: the uniform test runs all four sizes on both object kinds and all three
checksum families.
"""
import ctypes
import functools
import random

import numpy as np
import pytest
import torch

import ecutil
from test_ragged_gpu import Stripes, _reference

pytestmark = pytest.mark.gpu

T = 4096
PAD = 16
SENTINEL = {4: 0x7E57C0DE, 8: 0x7E57C0DE7E57C0DE}
GARBAGE = {4: 0x5A5A5A5A, 8: 0x5A5A5A5A5A5A5A5A}
CRC32C = -1  # the `kind` of a case: CRC32C, or a crc64 variant number
ROCKSOFT_REFL, ECMA_NORM = 6, 1  # CRC-64/NVME, and a norm flavour (isal_hip.h ISAL_HIP_CRC64_*)
_rng = random.Random(977)
INIT32, INIT64 = _rng.getrandbits(32) | 1, _rng.getrandbits(64) | 1  # random, non-zero


def LENS(S):
    return [0, 1, 15, 16, 17, S - 1, S, S + 1, S + 16 + 3, T - 1, T, T + 1, T + S + 5, 2 * T + 3 * 16 + 7, 3 * T]


def orders(S):
    """As listed, reversed, and with zero-length stripes first and last."""
    lens = LENS(S)
    out = [lens, lens[::-1], [0] + lens[2::2] + lens[1::2] + [0]]
    assert out[0][0] == 0 and out[1][-1] == 0 and out[2][0] == 0 and out[2][-1] == 0
    assert sorted(out[2][1:]) == sorted(lens)
    return out


def _width(kind):
    return 4 if kind == CRC32C else 8


def _init(kind):
    return INIT32 if kind == CRC32C else INIT64


def _crc(oracle, kind, a, init):
    return oracle.crc32_iscsi(a, init) if kind == CRC32C else oracle.crc64(kind, a, init)


def _sector_words(oracle, st, S, kind, init, image):
    """The oracle's word of every sector of every shard in `image`, in the
    ragged layout: (k+rows)*first[s] + j*ns + i."""
    out = []
    for s, n in enumerate(st.lens):
        for j in range(st.m):
            sh = image[st.off[s][j]:st.off[s][j] + n]
            out += [_crc(oracle, kind, sh[a:min(a + S, n)], init) for a in range(0, n, S)]
    return np.array(out, dtype=np.uint32 if kind == CRC32C else np.uint64)


@functools.lru_cache(maxsize=None)
def _oracle_words(k, rows, lens, seed, S, kind, init):
    """... of the encoded case (oracle parity); computed once per case."""
    st = _HostCase(k, rows, lens, seed)
    out = _sector_words(ecutil.oracle(), st, S, kind, init, st.want)
    out.setflags(write=False)
    return out


class _HostCase:
    """The host half of Stripes (offsets and the encoded image), no GPU."""

    def __init__(self, k, rows, lens, seed):
        self.k, self.rows, self.m, self.lens = k, rows, k + rows, list(lens)
        self.off, self.want, _, _, _ = _reference("rs", k, rows, tuple(lens), seed)


def _nwords(st, S):
    return st.m * sum(-(-n // S) for n in st.lens)


class Words:
    """n garbage words between PAD sentinel words on each side."""

    def __init__(self, st, n, kind):
        self.n, self.w = n, _width(kind)
        self.np = np.uint32 if self.w == 4 else np.uint64
        self.dev = torch.empty(n + 2 * PAD, dtype=torch.int32 if self.w == 4 else torch.int64, device=st.dev.device)
        self.crc = self.dev[PAD:PAD + n]
        self.garbage()

    def _signed(self, x):
        bits = 8 * self.w
        return x - (1 << bits) if x >> (bits - 1) else x

    def garbage(self):
        self.dev.fill_(self._signed(SENTINEL[self.w]))
        self.crc.fill_(self._signed(GARBAGE[self.w]))

    def read(self, what):
        got = self.dev.cpu().numpy().view(self.np)
        assert (got[:PAD] == SENTINEL[self.w]).all(), f"{what}: a word before crc written"
        assert (got[PAD + self.n:] == SENTINEL[self.w]).all(), f"{what}: a word after the last sector's written"
        return got[PAD:PAD + self.n].copy()


def _call(obj, kind, S, init):
    if kind == CRC32C:
        return lambda crc, stream: obj.sector_crc(S, init, crc, stream)
    return lambda crc, stream: obj.sector_crc64(kind, S, init, crc, stream)


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


def _where(st, S, pos):
    for s, n in enumerate(st.lens):
        ns = -(-n // S)
        if pos < st.m * ns:
            return f"stripe {s} (len {n}) shard {pos // ns} sector {pos % ns}"
        pos -= st.m * ns
    return f"word {pos} past the end"


def _expect(got, want, st, S, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        pos = int(np.nonzero(got != want)[0][0])
        raise AssertionError(f"{what}: {_where(st, S, pos)}: got {int(got[pos]):#x}, want {int(want[pos]):#x}")


def _ragged_case(engine, gpu, k, rows, S, order, kind):
    lens = orders(S)[order]
    seed = 900 + order
    init = _init(kind)
    st = Stripes(gpu, "rs", k, rows, lens, seed, encoded=True)
    first, total = engine.ragged_sector_offsets(lens, S)
    assert st.m * total == _nwords(st, S)
    rg = engine.Ragged(k, rows, st.tbls, lens, st.data, st.coding)
    words = Words(st, st.m * total, kind)
    want = _oracle_words(k, rows, tuple(lens), seed, S, kind, init)
    try:
        for run in ("first call", "second call"):  # the second rewrites every word over fresh garbage
            what = f"kind {kind} sector {S} {run}"
            got = _run(engine, st, words, _call(rg, kind, S, init), 1, what)
            _expect(got, want, st, S, what)
    finally:
        rg.close()


@pytest.mark.parametrize("order", range(3))
@pytest.mark.parametrize("S,k,rows", [(512, 1, 1), (512, 3, 2), (512, 10, 4), (4096, 1, 1), (4096, 3, 2), (4096, 10, 4),
                                      (1024, 3, 2)])
def test_ragged_sector_crc32c_matches_the_oracle_per_sector(engine, gpu, S, k, rows, order):
    """Every word equals crc32_iscsi of its sector's bytes for a random
    non-zero init; exactly one launch; the sentinels after the last word and
    every shard byte unchanged; a second call rewrites every word."""
    _ragged_case(engine, gpu, k, rows, S, order, CRC32C)


@pytest.mark.parametrize("order", range(3))
@pytest.mark.parametrize("S,variant", [(512, v) for v in range(8)] + [(4096, ROCKSOFT_REFL), (4096, ECMA_NORM)])
def test_ragged_sector_crc64_matches_the_oracle_per_sector(engine, gpu, S, variant, order):
    _ragged_case(engine, gpu, 3, 2, S, order, variant)


def _uniform(gpu, n, seed):
    return Stripes(gpu, "rs", 3, 2, [n, n, n], seed, encoded=True)


@pytest.mark.parametrize("S", [512, 1024, 2048, 4096])
@pytest.mark.parametrize("which", range(4))
def test_uniform_sector_checksums_match_the_oracle_and_the_ragged_object(engine, gpu, S, which):
    """One uniform batch per length, three stripes of 3+2: CRC32C, a reflected
    and a normal crc64 against the oracle, and against a ragged object over
    the same buffers (with equal lengths first[s] = s*ns, so the two layouts
    are the same words in the same order)."""
    n = [S - 1, S, T + S + 5, 2 * T + 3 * 16 + 7][which]
    seed = 940 + which
    st = _uniform(gpu, n, seed)
    k, rows = st.k, st.rows
    bt = engine.Batch(n, k, rows, st.tbls, st.S, st.data, st.coding)
    rg = engine.Ragged(k, rows, st.tbls, st.lens, st.data, st.coding)
    first, total = engine.ragged_sector_offsets(st.lens, S)
    ns = -(-n // S)
    assert list(first) == [s * ns for s in range(st.S)] and total == st.S * ns
    try:
        for kind in (CRC32C, ROCKSOFT_REFL, ECMA_NORM):
            init = _init(kind)
            words = Words(st, st.m * total, kind)
            want = _oracle_words(k, rows, tuple(st.lens), seed, S, kind, init)
            what = f"kind {kind} sector {S} len {n}"
            got_b = _run(engine, st, words, _call(bt, kind, S, init), 1, what + " batch")
            _expect(got_b, want, st, S, what + " batch")
            got_r = _run(engine, st, words, _call(rg, kind, S, init), 1, what + " ragged")
            _expect(got_r, got_b, st, S, what + " ragged against batch")
    finally:
        bt.close()
        rg.close()


@pytest.mark.parametrize("S", [512, 4096])
def test_more_work_items_than_resident_workgroups(engine, gpu, S):
    """Workgroups stay resident and stride over the (shard, tile) items, at
    most 2048 of them for CRC32C and 1280 for crc64: 32 stripes of 3+2 shards of
    17 tiles are 2720 items, so workgroups take a second and a third item (and
    the 4 KiB sector's LDS hand-off alternates its two slots)."""
    n, seed, nstripes = 16 * T + 37, 970, 32
    st = Stripes(gpu, "rs", 3, 2, [n] * nstripes, seed, encoded=True)
    assert st.S * st.m * -(-n // T) > 2048
    bt = engine.Batch(n, st.k, st.rows, st.tbls, st.S, st.data, st.coding)
    rg = engine.Ragged(st.k, st.rows, st.tbls, st.lens, st.data, st.coding)
    try:
        for kind in (CRC32C, ROCKSOFT_REFL, ECMA_NORM):
            init = _init(kind)
            words = Words(st, _nwords(st, S), kind)
            want = _oracle_words(st.k, st.rows, tuple(st.lens), seed, S, kind, init)
            for name, obj in (("batch", bt), ("ragged", rg)):
                what = f"kind {kind} sector {S} {name}"
                _expect(_run(engine, st, words, _call(obj, kind, S, init), 1, what), want, st, S, what)
    finally:
        bt.close()
        rg.close()


@pytest.mark.parametrize("kind", [CRC32C, ROCKSOFT_REFL])
def test_one_flipped_byte_changes_exactly_its_sectors_word(engine, oracle, gpu, kind):
    """Localisation: a byte flipped in one parity shard changes the word of the
    sector that holds it and no other, on both object kinds."""
    S, n, seed, init = 512, T + 512 + 5, 950, _init(kind)
    st = _uniform(gpu, n, seed)
    k, rows, ns = st.k, st.rows, -(-n // S)
    bt = engine.Batch(n, k, rows, st.tbls, st.S, st.data, st.coding)
    rg = engine.Ragged(k, rows, st.tbls, st.lens, st.data, st.coding)
    words = Words(st, st.m * st.S * ns, kind)
    try:
        for name, obj in (("batch", bt), ("ragged", rg)):
            clean = _run(engine, st, words, _call(obj, kind, S, init), 1, "clean")
            _expect(clean, _oracle_words(k, rows, tuple(st.lens), seed, S, kind, init), st, S, "clean")
            # a parity shard: the short last sector's byte tail, a middle sector's first byte, the last byte of tile 0
            for s, shard, col in [(1, k + 1, n - 2), (2, k, 3 * S), (0, k + rows - 1, T - 1)]:
                st.flip(s, shard, col)
                got = _run(engine, st, words, _call(obj, kind, S, init), 1, f"{name} corrupt")
                _expect(got, _sector_words(oracle, st, S, kind, init, st.image), st, S, f"{name} corrupt")
                assert [int(p) for p in np.nonzero(got != clean)[0]] == [(s * st.m + shard) * ns + col // S], (name, s, shard, col)
                st.restore()
    finally:
        bt.close()
        rg.close()


def test_all_zero_lengths_enqueue_nothing(engine, gpu):
    """Every length 0: the calls return 0, launch nothing and leave crc alone,
    on the ragged object and on a uniform batch of length 0."""
    k, rows = 3, 2
    st = Stripes(gpu, "rs", k, rows, [0, 0, 0], 7)
    rg = engine.Ragged(k, rows, st.tbls, st.lens, st.data, st.coding)
    bt = engine.Batch(0, k, rows, st.tbls, st.S, st.data, st.coding)
    assert engine.ragged_sector_offsets(st.lens, 512)[1] == 0
    try:
        for obj in (rg, bt):
            for kind in (CRC32C, ROCKSOFT_REFL):
                words = Words(st, 8, kind)
                got = _run(engine, st, words, _call(obj, kind, 512, _init(kind)), 0, "all lengths zero")
                assert (got == GARBAGE[_width(kind)]).all(), "crc written although every length is 0"
    finally:
        rg.close()
        bt.close()


def test_sector_crc_is_ordered_behind_encode_on_one_stream(engine, gpu):
    """ragged encode, then sector_crc, on one non-default stream with nothing
    between them: the parity sectors' words are those of the fresh parity."""
    k, rows, S, seed, kind = 3, 2, 512, 902, CRC32C
    lens = orders(S)[2]
    st = Stripes(gpu, "rs", k, rows, lens, seed)  # poisoned parity
    rg = engine.Ragged(k, rows, st.tbls, lens, st.data, st.coding)
    words = Words(st, _nwords(st, S), kind)
    stream = torch.cuda.Stream(device=gpu)
    try:
        torch.cuda.synchronize()
        rg.encode(stream.cuda_stream)
        rg.sector_crc(S, INIT32, words.crc, stream.cuda_stream)
        stream.synchronize()
        st.same("after encode and sector_crc", st.want)
        got = words.read("side stream")
        want = _oracle_words(k, rows, tuple(lens), seed, S, kind, INIT32)
        _expect(got, want, st, S, "side stream")
        stale = _sector_words(ecutil.oracle(), st, S, kind, INIT32, st.poisoned)
        # the words that tell fresh parity from the poison it replaced: nearly all of
        # the parity's (a 1-byte sector's parity byte may happen to be the poison byte)
        assert (stale != want).sum() > 0.9 * rows * sum(-(-n // S) for n in lens), "the case cannot tell fresh parity from poison"
    finally:
        rg.close()


def test_an_unaligned_shard_of_the_uniform_batch_is_refused(engine, gpu):
    """isal_hip_batch_check's rule: one shard 8 bytes off a 16-byte boundary,
    ISAL_HIP_EINVAL from both calls with nothing launched and crc untouched."""
    k, rows, n, S = 3, 2, 1024, 3
    buf = torch.zeros(S * (k + rows) * (n + 64) + 64, dtype=torch.uint8, device=gpu)
    base = int(buf.data_ptr())
    assert base % 16 == 0
    ptrs = [base + i * (n + 64) for i in range(S * (k + rows))]
    ptrs[k + 1] += 8  # a source of stripe 1
    data = [ptrs[s * (k + rows) + j] for s in range(S) for j in range(k)]
    coding = [ptrs[s * (k + rows) + k + l] for s in range(S) for l in range(rows)]
    a = engine.gf_gen_rs_matrix(k + rows, k)
    bt = engine.Batch(n, k, rows, engine.ec_init_tables(k, rows, a[k * k:]), S, data, coding)
    crc = torch.full((S * (k + rows) * 2 + 2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=gpu)
    L = engine.lib()
    try:
        torch.cuda.synchronize()
        before = engine.kernel_launches()
        p = ctypes.c_void_p(int(crc.data_ptr()))
        assert L.isal_hip_batch_sector_crc(bt._h, 512, INIT32, p, None) == -1
        assert L.isal_hip_batch_sector_crc64(bt._h, ROCKSOFT_REFL, 512, INIT64, p, None) == -1
        with pytest.raises(RuntimeError):
            bt.sector_crc(512, INIT32, crc, 0)
        torch.cuda.synchronize()
        assert engine.kernel_launches() == before
        assert (crc.cpu().numpy().view(np.uint64) == 0x5A5A5A5A5A5A5A5A).all()
    finally:
        bt.close()


def test_live_objects_refuse_bad_sectors_and_variants(engine, gpu):
    """The refusals a host without a GPU cannot reach: a live object with a bad
    sector, a bad variant or a NULL crc; nothing launched."""
    k, rows = 3, 2
    st = _uniform(gpu, 1024, 960)
    bt = engine.Batch(1024, k, rows, st.tbls, st.S, st.data, st.coding)
    rg = engine.Ragged(k, rows, st.tbls, st.lens, st.data, st.coding)
    words = Words(st, 64, ROCKSOFT_REFL)
    L = engine.lib()
    p = ctypes.c_void_p(int(words.crc.data_ptr()))
    try:
        before = engine.kernel_launches()
        for h, f32, f64 in ((bt._h, L.isal_hip_batch_sector_crc, L.isal_hip_batch_sector_crc64),
                            (rg._h, L.isal_hip_ragged_sector_crc, L.isal_hip_ragged_sector_crc64)):
            for sector in (0, 256, 768, 8192, -512):
                assert f32(h, sector, 1, p, None) == -1 and f64(h, 0, sector, 1, p, None) == -1
            for variant in (-1, 8):
                assert f64(h, variant, 512, 1, p, None) == -1
            assert f32(h, 512, 1, None, None) == -1 and f64(h, 0, 512, 1, None, None) == -1
        torch.cuda.synchronize()
        assert engine.kernel_launches() == before
        assert (words.read("refusals") == GARBAGE[8]).all()
    finally:
        bt.close()
        rg.close()
