"""GPU tier: the stripe batch's update, check and set_tables (include/isal_hip.h)
where the encode's tests do not reach.

The checker is always the oracle (oracle.ec_encode_data_update, oracle.encode,
ecutil.decode_matrix, oracle.crc32_iscsi / crc64), never the engine's own
encode, and every comparison is byte for byte.

Layout: as Stripes of test_repair_gpu.py, every shard of a batch lies in one
device allocation, each followed (and, when it starts at a byte offset,
preceded) by guard bytes. After every operation the whole allocation is
compared with a host image: the guards and every shard the operation must not
write are unchanged, the others hold the checker's bytes.

Sizes: the update runs 128-lane workgroups over 2 KiB column tiles, the
encode and the check 256 lanes over 4 KiB; no len exceeds three tiles and no
batch eight stripes.
"""
import random

import numpy as np
import pytest
import torch

import ecutil
from ecutil import fill_bytes

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTES = 0x3C, 64
EINVAL, EHIP = r"\(-1\)", r"\(-2\)"  # ISAL_HIP_EINVAL / ISAL_HIP_EHIP in the wrapper's exception
UPD_TILE, TILE = 2048, 4096
CLEAN = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(autouse=True)
def _reload_knobs_after(engine):
    """Knobs are read once by the library: tests that change one re-read them
    (_setenv), and every test leaves the library re-synced with os.environ."""
    yield
    engine.reload_config()


def _setenv(monkeypatch, name, value):
    import isal_amd

    if value is None:  # back to the library's default
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)
    isal_amd.reload_config()


class Shards:
    """S stripes of k sources and `rows` parity shards in one device
    allocation: shard (s, i) in row s*(k+rows) + i of a (S*(k+rows), span)
    byte matrix, at byte offset off[row] of its 16-byte aligned row, guard
    bytes everywhere else (at least 64 after every shard). Sources and parity
    start as seeded random bytes. `want` is the host image the device must
    hold; get() returns writable views into it."""

    def __init__(self, gpu, k, rows, n, S, seed, skew="aligned"):
        self.k, self.rows, self.m, self.n, self.S = k, rows, k + rows, n, S
        nrow = S * self.m
        self.off = np.zeros(nrow, np.int64)
        if skew == "all3":      # every shard at byte offset 3
            self.off[:] = 3
        elif skew == "last1":   # only the last stripe's last parity shard, at offset 1
            self.off[-1] = 1
        else:
            assert skew == "aligned"
        self.span = (int(self.off.max()) + n + GUARD_BYTES + 15) // 16 * 16
        self.want = np.full((nrow, self.span), GUARD, np.uint8)
        for r in range(nrow):
            self.want[r, self.off[r]:self.off[r] + n] = fill_bytes(n, seed * 4096 + r)
        self.dev = torch.from_numpy(self.want.copy()).to(gpu)
        base = int(self.dev.data_ptr())
        assert base % 16 == 0
        ptr = [base + r * self.span + int(self.off[r]) for r in range(nrow)]
        self.aligned = all(p % 16 == 0 for p in ptr)
        assert self.aligned == (skew == "aligned")
        self.data = [ptr[s * self.m + j] for s in range(S) for j in range(k)]
        self.coding = [ptr[s * self.m + k + l] for s in range(S) for l in range(rows)]

    def get(self, s, i):
        r = s * self.m + i
        return self.want[r, self.off[r]:self.off[r] + self.n]

    def src(self, s):
        return [self.get(s, j).copy() for j in range(self.k)]

    def parity(self, s):
        return [self.get(s, self.k + l) for l in range(self.rows)]

    def upload(self):
        """The device takes the host image."""
        self.dev.copy_(torch.from_numpy(self.want))
        torch.cuda.synchronize()

    def poke(self, s, i, col, x):
        """XOR x into byte col of shard (s, i), on the device and in the image."""
        r = s * self.m + i
        self.get(s, i)[col] ^= x
        self.dev[r, int(self.off[r]) + col] ^= x

    def verify(self, what):
        torch.cuda.synchronize()
        got = self.dev.cpu().numpy()
        for r in range(got.shape[0]):
            s, i = divmod(r, self.m)
            a, b = int(self.off[r]), int(self.off[r]) + self.n
            kind = "source" if i < self.k else "parity row"
            assert np.array_equal(got[r, a:b], self.want[r, a:b]), \
                f"{what}: stripe {s} {kind} {i if i < self.k else i - self.k} differs"
            assert np.array_equal(got[r, :a], self.want[r, :a]) and np.array_equal(got[r, b:], self.want[r, b:]), \
                f"{what}: stripe {s} shard {i}: guard written"


def _coef(oracle, kind, k, rows, seed):
    """rows x k coefficients: 'rs' the Vandermonde rows of gf_gen_rs_matrix
    (row 0 and column 0 are 0/1), 'random' any bytes, 'big' bytes >= 2 (no
    0/1 structure), 'mask' bytes >= 2 with row 0 and column 0 random 0/1 (the
    'mask' kind of test_gpu_parity._coef_01)."""
    rng = np.random.default_rng(seed)
    if kind == "rs":
        return oracle.gf_gen_rs_matrix(k + rows, k)[k * k:].copy()
    if kind == "random":
        return rng.integers(0, 256, rows * k, dtype=np.uint8)
    c = rng.integers(2, 256, (rows, k), dtype=np.uint8)
    if kind == "mask":
        c[0] = rng.integers(0, 2, k, dtype=np.uint8)
        c[:, 0] = rng.integers(0, 2, rows, dtype=np.uint8)
    else:
        assert kind == "big"
    return c.reshape(-1)


def _decode_coef(oracle, k, rows, seed):
    """rows recovery rows over k survivors (ecutil.decode_matrix) of the
    (k + rows, k) Vandermonde code, for the first seeded erasure pattern of
    `rows` shards, data and parity mixed, that the checker can invert."""
    a = oracle.gf_gen_rs_matrix(k + rows, k)
    rng = random.Random(seed)
    for _ in range(32):
        errs = sorted(rng.sample(range(k + rows), rows))
        ret, c, _ = ecutil.decode_matrix(a, k, errs, oracle)
        if ret == 0 and any(e < k for e in errs):
            return c
    raise AssertionError("no invertible erasure pattern found")


def _passes(rows):
    return (rows + 7) // 8


def _oracle_parity(oracle, coef, st, s):
    if st.n == 0:
        return [np.zeros(0, np.uint8) for _ in range(st.rows)]
    return oracle.encode(coef, st.k, st.rows, st.src(s))


def _expect_bad(oracle, coef, st):
    """bad[] as isal_hip.h defines it, from the oracle's parity of the image's
    sources against the image's parity: smallest mismatching column, then
    smallest row; ~0 for a consistent stripe."""
    out = np.full(st.S, CLEAN, np.uint64)
    for s in range(st.S):
        want = _oracle_parity(oracle, coef, st, s)
        mism = np.stack([st.get(s, st.k + l) != want[l] for l in range(st.rows)])
        if mism.any():
            col = int(np.nonzero(mism.any(axis=0))[0][0])
            row = int(np.nonzero(mism[:, col])[0][0])
            out[s] = np.uint64((col << 8) | row)
    return out


def _run_check(b, st, gpu):
    """One check into a result buffer pre-filled with zeros (a stale or
    unwritten word would read 0, a valid answer for no stripe here)."""
    bad = torch.zeros(st.S, dtype=torch.int64, device=gpu)
    b.check(bad, 0)
    torch.cuda.synchronize()
    return bad.cpu().numpy().view(np.uint64)


# --------------------------------------------------------------------------
# 1. batch update vs the oracle
# --------------------------------------------------------------------------

def _update_all(engine, oracle, gpu, k, rows, n, S, kind, skew, seed):
    coef = _coef(oracle, kind, k, rows, seed)
    tbls = oracle.ec_init_tables(k, rows, coef)
    st = Shards(gpu, k, rows, n, S, seed, skew)
    start = [[p.copy() for p in st.parity(s)] for s in range(S)]
    order = random.Random(seed).sample(range(k), k)
    # the checker: the same folds in the same order on the same starting bytes
    for s in range(S):
        src, par = st.src(s), [p.copy() for p in start[s]]
        if n:
            for v in order:
                oracle.ec_encode_data_update(n, k, rows, v, tbls, src[v], par)
        enc = _oracle_parity(oracle, coef, st, s)
        for l in range(rows):
            assert np.array_equal(par[l], start[s][l] ^ enc[l]), "the checker's update and encode disagree"
            st.get(s, k + l)[:] = par[l]
    b = engine.Batch(n, k, rows, tbls, S, st.data, st.coding)
    try:
        torch.cuda.synchronize()
        before = engine.kernel_launches()
        for v in order:
            b.update(v, 0)
        torch.cuda.synchronize()
        assert engine.kernel_launches() - before == (k * _passes(rows) if n else 0)
        st.verify(f"update of all {k} sources in order {order}")
    finally:
        b.close()


UPDATE_CASES = (
    # every ec_update_v16<P, 128> instance, and for rows > 8 a second pass of
    # 1, 4 and 8 rows on tables of its own (random coefficients): two full
    # 2 KiB tiles, a partial tile of three lanes and a byte tail
    [(5 + 2 * (rows % 2), rows, 2 * UPD_TILE + 48 + 3, 3, "rs" if rows in (3, 6) else "random", "aligned")
     for rows in (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16)]
    # lens around the update's own 2 KiB tile: one lane; the last lane of a
    # tile, the exact tile, the first lane of the next; a vector part plus
    # mad_bytes; the byte tail alone; nothing
    + [(10, 4, n, 3, "rs", "aligned") for n in (16, UPD_TILE - 16, UPD_TILE, UPD_TILE + 16, 4096 + 5, 5, 0)]
    # the byte-lane kernel ec_update_b1 (256 bytes per workgroup): every shard
    # misaligned, and a single misaligned pointer in the whole batch
    + [(5, rows, n, 2, "random", skew) for skew in ("all3", "last1") for rows in (3, 11)
       for n in (1, 255, 256, 257, 4096 + 5)]
)


@pytest.mark.parametrize("k,rows,n,S,kind,skew", UPDATE_CASES)
def test_batch_update_vs_oracle(engine, oracle, gpu, k, rows, n, S, kind, skew):
    """Parity that starts as random bytes, every source folded in by
    b.update(v) in a seeded random order == the oracle's
    ec_encode_data_update in that order == start ^ oracle.encode; sources and
    guards untouched; one launch per pass and source, none for len = 0."""
    _update_all(engine, oracle, gpu, k, rows, n, S, kind, skew, 100 + 31 * rows + n % 97)


def test_batch_update_first_and_last_source_alone(engine, oracle, gpu):
    """One update(0), then one update(k - 1): each result == the oracle's
    single-source update (the first and the last table offset vec_i*P*kTbl)."""
    k, rows, n, S = 12, 8, 2 * UPD_TILE + 48 + 3, 3
    coef = _coef(oracle, "random", k, rows, 7)
    tbls = oracle.ec_init_tables(k, rows, coef)
    st = Shards(gpu, k, rows, n, S, 7)
    b = engine.Batch(n, k, rows, tbls, S, st.data, st.coding)
    try:
        for v in (0, k - 1):
            for s in range(S):
                par = [p.copy() for p in st.parity(s)]
                oracle.ec_encode_data_update(n, k, rows, v, tbls, st.src(s)[v], par)
                for l in range(rows):
                    st.get(s, k + l)[:] = par[l]
            b.update(v, 0)
            st.verify(f"update({v}) alone")
    finally:
        b.close()


@pytest.mark.parametrize("skew", ["all3", "last1"])
def test_batch_check_refuses_a_misaligned_batch(engine, oracle, gpu, skew):
    """check needs every shard 16-byte aligned: ISAL_HIP_EINVAL otherwise,
    nothing launched, nothing written."""
    k, rows, n, S = 5, 3, 257, 2
    st = Shards(gpu, k, rows, n, S, 8, skew)
    b = engine.Batch(n, k, rows, oracle.ec_init_tables(k, rows, _coef(oracle, "rs", k, rows, 8)), S,
                     st.data, st.coding)
    try:
        bad = torch.zeros(S, dtype=torch.int64, device=gpu)
        torch.cuda.synchronize()
        before = engine.kernel_launches()
        with pytest.raises(RuntimeError, match=EINVAL):
            b.check(bad, 0)
        torch.cuda.synchronize()
        assert engine.kernel_launches() == before
        assert bool((bad == 0).all())
        st.verify("refused check")
    finally:
        b.close()


def test_batch_update_refuses_a_bad_source_index(engine, oracle, gpu):
    k, rows, n, S = 5, 3, UPD_TILE + 16, 2
    st = Shards(gpu, k, rows, n, S, 9)
    b = engine.Batch(n, k, rows, oracle.ec_init_tables(k, rows, _coef(oracle, "rs", k, rows, 9)), S,
                     st.data, st.coding)
    try:
        torch.cuda.synchronize()
        before = engine.kernel_launches()
        for v in (-1, k):
            with pytest.raises(RuntimeError, match=EINVAL):
                b.update(v, 0)
        torch.cuda.synchronize()
        assert engine.kernel_launches() == before
        st.verify("refused update")
    finally:
        b.close()


# --------------------------------------------------------------------------
# 2. batch check with more than one mismatch
# --------------------------------------------------------------------------

# Each case: k, rows, len, then steps. A step is (flips, (column, row)): the
# flips (shard index i of the stripe: i < k a source, k + l parity row l;
# column; XOR value) are ADDED to the corrupted stripe, then (column, row) is
# the first mismatch the contract names: smallest column, then smallest row.
CHECK_CASES = {
    # one mismatch per 4 KiB tile (one workgroup each), added from the last
    # tile down: a source byte (every row of that column differs) in the
    # middle, parity row 3 in the first tile
    "three_tiles_descending": (10, 4, 3 * TILE, [
        ([(10 + 0, 2 * TILE + 5, 0x40)], (2 * TILE + 5, 0)),
        ([(4, TILE + 777, 0x01)], (TILE + 777, 0)),
        ([(10 + 3, 100, 0x80)], (100, 3)),
    ]),
    # one 16-byte lane: row 0 differs at its byte 12, row 2 at its byte 1
    "two_rows_one_lane": (10, 4, 3 * TILE, [
        ([(10 + 0, TILE + 16 * 37 + 12, 0x02), (10 + 2, TILE + 16 * 37 + 1, 0x10)], (TILE + 16 * 37 + 1, 2)),
    ]),
    "two_rows_one_column": (10, 4, 3 * TILE, [
        ([(10 + 3, 5000, 0x04), (10 + 1, 5000, 0x20)], (5000, 1)),
    ]),
    # rows > 8: rows 0-7 in the first launch, 8-11 in the second
    "two_passes": (12, 12, 2 * TILE + 16, [
        ([(12 + 2, 6000, 0x08), (12 + 10, 3000, 0x01)], (3000, 10)),
        ([(12 + 2, 3000, 0x80)], (3000, 2)),
    ]),
    # aligned shards, len % 16 = 5: the verify's byte tail (dot_bytes<P, true>)
    "byte_tail": (10, 4, TILE + 5, [
        ([(10 + 2, TILE + 4, 0x01)], (TILE + 4, 2)),
        ([(10 + 1, TILE - 6, 0x40)], (TILE - 6, 1)),
    ]),
}


@pytest.mark.parametrize("xor", ["1", "0"])
@pytest.mark.parametrize("case", sorted(CHECK_CASES))
def test_batch_check_first_of_several_mismatches(engine, oracle, gpu, monkeypatch, xor, case):
    """Several corrupted bytes in the middle stripe of three: bad[1] is the
    smallest mismatching column, then the smallest row — across lanes,
    workgroups and, for rows > 8, both launches — as computed from the
    oracle's parity; its neighbours read ~0; once the bytes are restored a
    second check reads ~0 everywhere. Nothing is written to the shards."""
    k, rows, n, steps = CHECK_CASES[case]
    S, victim = 3, 1
    _setenv(monkeypatch, "ISAL_HIP_ENC_XOR", xor)
    coef = _coef(oracle, "rs", k, rows, 0)
    st = Shards(gpu, k, rows, n, S, 20 + n % 7)
    b = engine.Batch(n, k, rows, oracle.ec_init_tables(k, rows, coef), S, st.data, st.coding)
    try:
        b.encode(0)
        for s in range(S):
            for l, p in enumerate(_oracle_parity(oracle, coef, st, s)):
                st.get(s, k + l)[:] = p
        st.verify("encode")
        assert (_run_check(b, st, gpu) == CLEAN).all()
        done = []
        for flips, (col, row) in steps:
            for i, c, x in flips:
                st.poke(victim, i, c, x)
                done.append((i, c, x))
            want = _expect_bad(oracle, coef, st)
            assert want[victim] == np.uint64((col << 8) | row), "the checker disagrees with the case's own answer"
            assert want[0] == CLEAN and want[2] == CLEAN
            got = _run_check(b, st, gpu)
            assert [hex(int(v)) for v in got] == [hex(int(v)) for v in want], (case, done)
            st.verify("check")
        for i, c, x in done:
            st.poke(victim, i, c, x)
        assert (_expect_bad(oracle, coef, st) == CLEAN).all()
        assert (_run_check(b, st, gpu) == CLEAN).all(), "a restored stripe still reads as bad"
        st.verify("check after the restore")
    finally:
        b.close()


# --------------------------------------------------------------------------
# 3. set_tables on a live batch
# --------------------------------------------------------------------------

def _assert_batch_on_matrix(engine, oracle, gpu, b, st, coef, what, flip):
    """Everything the batch computes follows coef: encode == the oracle;
    update of all k sources from zeroed parity gives the same bytes; check
    reads ~0; one flipped byte (stripe, shard, column) is reported at its
    place."""
    k, rows, S = st.k, st.rows, st.S
    want = [_oracle_parity(oracle, coef, st, s) for s in range(S)]
    for s in range(S):  # stale parity the encode must overwrite
        for l in range(rows):
            st.get(s, k + l)[:] = 0xEE
    st.upload()
    b.encode(0)
    for s in range(S):
        for l in range(rows):
            st.get(s, k + l)[:] = want[s][l]
    st.verify(f"{what}: encode")
    st.dev.copy_(torch.from_numpy(np.where(_parity_mask(st), 0, st.want).astype(np.uint8)))
    for v in range(k):
        b.update(v, 0)
    st.verify(f"{what}: update of every source from zeroed parity")
    assert (_run_check(b, st, gpu) == CLEAN).all(), f"{what}: check of consistent stripes"
    s, i, col = flip
    st.poke(s, i, col, 0x40)
    exp = _expect_bad(oracle, coef, st)
    assert exp[s] != CLEAN and (exp[s] >> np.uint64(8)) == np.uint64(col)
    got = _run_check(b, st, gpu)
    assert [hex(int(v)) for v in got] == [hex(int(v)) for v in exp], f"{what}: check of one flipped byte"
    st.poke(s, i, col, 0x40)
    st.verify(f"{what}: check")


def _parity_mask(st):
    """True at the parity shards' bytes of the image."""
    m = np.zeros(st.want.shape, bool)
    for s in range(st.S):
        for l in range(st.rows):
            r = s * st.m + st.k + l
            m[r, st.off[r]:st.off[r] + st.n] = True
    return m


@pytest.mark.parametrize("k,rows,ldsx", [
    (10, 8, None), (11, 7, None),  # LDS product tables by default
    (10, 5, None),                 # the LDS-DMA ring by default ...
    (10, 5, "1"),                  # ... product tables when forced
    (10, 3, None),                 # no product tables
    (12, 12, None),                # two passes, product tables for both
])
def test_set_tables_sequence_on_one_batch(engine, oracle, gpu, monkeypatch, k, rows, ldsx):
    """One batch object taken through matrices with and without 0/1 rows and
    columns (the masks em), and back: after each replacement the coefficient
    tables, the masks and the LDS product tables all follow the new matrix."""
    if ldsx is not None:
        _setenv(monkeypatch, "ISAL_HIP_ENC_LDSX", ldsx)
    n, S = 2 * TILE + 16, 3
    seq = [("rs", _coef(oracle, "rs", k, rows, 0)),
           ("big", _coef(oracle, "big", k, rows, 31 * k + rows)),
           ("mask", _coef(oracle, "mask", k, rows, 37 * k + rows))]
    if (k, rows) != (12, 12):
        seq.append(("decode", _decode_coef(oracle, k, rows, 41 * k + rows)))
    seq.append(("rs again", seq[0][1]))
    st = Shards(gpu, k, rows, n, S, 30 + k + rows)
    # created on a matrix of its own, so the first set_tables is a replacement too
    b = engine.Batch(n, k, rows, oracle.ec_init_tables(k, rows, _coef(oracle, "random", k, rows, 5)), S,
                     st.data, st.coding)
    rng = random.Random(k * rows)
    try:
        for name, coef in seq:
            b.set_tables(oracle.ec_init_tables(k, rows, coef))
            flip = (rng.randrange(S), k + rng.randrange(rows), rng.randrange(n))
            _assert_batch_on_matrix(engine, oracle, gpu, b, st, coef, f"after set_tables({name})", flip)
    finally:
        b.close()


@pytest.mark.parametrize("order", [("rs", "big"), ("big", "rs")])
def test_set_tables_checksums_follow_the_tables(engine, oracle, gpu, order):
    """The fused encode + checksum kernels derive the CRC of a 0/1 parity row
    from the sources' (the rows xr): with the Vandermonde matrix row 0 is
    derived, with random coefficients nothing is. After each replacement, in
    both orders, all k + rows checksums of every stripe == the oracle's
    checksum of the oracle's parity."""
    k, rows, n, S = 10, 4, 65536, 2
    init32, init64 = 0x9E3779B9, 0x0123456789ABCDEF
    variants = (engine.CRC64_VARIANTS.index("ecma_refl"), engine.CRC64_VARIANTS.index("iso_norm"))
    coefs = {kind: _coef(oracle, kind, k, rows, 77) for kind in order}
    st = Shards(gpu, k, rows, n, S, 40)
    want = {}
    for kind, coef in coefs.items():
        par = [_oracle_parity(oracle, coef, st, s) for s in range(S)]
        shards = [st.src(s) + par[s] for s in range(S)]
        want[kind] = (par,
                      [oracle.crc32_iscsi(x, init32) for s in range(S) for x in shards[s]],
                      {v: [oracle.crc64(v, x, init64) for s in range(S) for x in shards[s]] for v in variants})
    b = engine.Batch(n, k, rows, oracle.ec_init_tables(k, rows, coefs[order[0]]), S, st.data, st.coding)
    crc = torch.zeros(S * (k + rows), dtype=torch.int32, device=gpu)
    crc64 = torch.zeros(S * (k + rows), dtype=torch.int64, device=gpu)
    try:
        for step, kind in enumerate((order[0], order[1], order[0])):
            if step:
                b.set_tables(oracle.ec_init_tables(k, rows, coefs[kind]))
            par, w32, w64 = want[kind]
            for s in range(S):
                for l in range(rows):
                    st.get(s, k + l)[:] = par[s][l]
            crc.zero_()
            b.encode_crc(init32, crc, 0)
            st.verify(f"step {step} ({kind}): encode_crc")
            assert [int(v) & 0xFFFFFFFF for v in crc.tolist()] == w32, f"step {step} ({kind}): crc32_iscsi"
            for v in variants:
                st.dev.copy_(torch.from_numpy(np.where(_parity_mask(st), 0x11, st.want).astype(np.uint8)))
                crc64.zero_()
                b.encode_crc64(v, init64, crc64, 0)
                st.verify(f"step {step} ({kind}): encode_crc64({engine.CRC64_VARIANTS[v]})")
                assert [int(x) & 0xFFFFFFFFFFFFFFFF for x in crc64.tolist()] == w64[v], \
                    f"step {step} ({kind}): crc64_{engine.CRC64_VARIANTS[v]}"
    finally:
        b.close()


def test_set_tables_failed_replacement_keeps_the_old_state(engine, oracle, gpu, monkeypatch):
    """ISAL_HIP_FAULT=7 fails the upload of the LDS product tables (a
    host-side early return: nothing is launched): set_tables returns
    ISAL_HIP_EHIP and the batch goes on computing the OLD matrix through the
    product tables, through the coefficient tables and masks (product tables
    off; update; check). Disarmed, the same replacement succeeds."""
    k, rows, n, S = 10, 8, 2 * TILE + 16, 3
    old, new = _coef(oracle, "rs", k, rows, 0), _coef(oracle, "big", k, rows, 51)
    st = Shards(gpu, k, rows, n, S, 50)
    b = engine.Batch(n, k, rows, oracle.ec_init_tables(k, rows, old), S, st.data, st.coding)
    try:
        _assert_batch_on_matrix(engine, oracle, gpu, b, st, old, "before", (1, k + 2, 4321))
        _setenv(monkeypatch, "ISAL_HIP_FAULT", "7")
        torch.cuda.synchronize()
        before = engine.kernel_launches()
        with pytest.raises(RuntimeError, match=EHIP):
            b.set_tables(oracle.ec_init_tables(k, rows, new))
        assert engine.kernel_launches() == before
        _assert_batch_on_matrix(engine, oracle, gpu, b, st, old, "after the failed set_tables", (2, k + 7, 17))
        _setenv(monkeypatch, "ISAL_HIP_ENC_LDSX", "0")
        _assert_batch_on_matrix(engine, oracle, gpu, b, st, old, "after the failed set_tables, no product tables",
                                (0, k + 0, 8200))
        _setenv(monkeypatch, "ISAL_HIP_ENC_LDSX", None)
        _setenv(monkeypatch, "ISAL_HIP_FAULT", None)
        b.set_tables(oracle.ec_init_tables(k, rows, new))
        _assert_batch_on_matrix(engine, oracle, gpu, b, st, new, "after the repeated set_tables", (1, k + 5, 4096))
        _setenv(monkeypatch, "ISAL_HIP_ENC_LDSX", "0")
        _assert_batch_on_matrix(engine, oracle, gpu, b, st, new, "after the repeated set_tables, no product tables",
                                (1, k + 5, 4095))
    finally:
        b.close()


def test_batch_without_memory_for_product_tables(engine, oracle, gpu, monkeypatch, capfd):
    """ISAL_HIP_FAULT=6 fails the allocation of the LDS product tables at
    create: the batch is created without them, its 8-row encode runs the
    LDS-DMA ring kernel (the ISAL_HIP_LOG=2 kernel line) and == the oracle,
    and no later launch reports a stale error. A set_tables once memory is
    back brings the product tables in."""
    k, rows, n, S = 10, 8, 2 * TILE + 16, 3
    coef = _coef(oracle, "rs", k, rows, 0)
    st = Shards(gpu, k, rows, n, S, 60)
    _setenv(monkeypatch, "ISAL_HIP_FAULT", "6")
    b = engine.Batch(n, k, rows, oracle.ec_init_tables(k, rows, coef), S, st.data, st.coding)
    try:
        _setenv(monkeypatch, "ISAL_HIP_LOG", "2")
        capfd.readouterr()
        _assert_batch_on_matrix(engine, oracle, gpu, b, st, coef, "without product tables", (1, k + 3, 5000))
        err = capfd.readouterr().err
        assert "kernel ec_encode_glds<8," in err and "ec_encode_ldsx" not in err, err
        _setenv(monkeypatch, "ISAL_HIP_FAULT", None)
        b.set_tables(oracle.ec_init_tables(k, rows, coef))
        _assert_batch_on_matrix(engine, oracle, gpu, b, st, coef, "with product tables", (2, k + 1, 16))
        err = capfd.readouterr().err
        assert "kernel ec_encode_ldsx<8," in err and "ec_encode_glds" not in err, err
    finally:
        b.close()
