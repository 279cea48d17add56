"""GPU tier: every instantiation of the fused encode + CRC32C and encode +
CRC64 kernels, launched once through the public batch calls and compared,
byte for byte and word for word, with the oracle.

isal_hip_batch_encode_crc is served by ec_encode_crc_v16<P, FusedPol<U>, REG,
SRC, X0, NB, NV> (crc_kernels.hip, launch_fused) and isal_hip_batch_encode_crc64
by ec_encode_crc64_v16<P, U, X0, SL, NV> (crc64_kernels.hip, launch_fused64).
Every instantiation is its own register allocation and its own schedule.
CELLS declares, as plain data, the template arguments of every one, spelled as
the launch log prints them (ISAL_HIP_LOG=2):

    ec_encode_crc_v16<P, U, SRC, X0, NB, NV>      240 = 8 P x 6 U x 5
        <P, U, 0, 0, 0, 1>        the second pass of rows > 8 (no source chains)
        <P, U, 1, X0, 4, NV>      X0 in {0, 1} x NV in {1, 2}
    ec_encode_crc64_v16<P, U, X0, SL, NV>         184 = 8 x 6 x 4 - 4 x 2
        <P, 10, X0, 3, 1>         P <= 4: chain steps pipelined into the GF rows
        <P, U, X0, 1, NV>         everywhere else, X0 in {0, 1} x NV in {1, 2}

tests/test_fused_crc_matrix_cpu.py holds CELLS equal to what the crc_fused_p*
and crc64_fused_p* objects were built with; the tests below launch every cell
of CELLS minus UNREACHABLE. So: built set == declared set ==
launched-and-checked set. UNREACHABLE is empty for both families: every built
instantiation is reached through engine.Batch(...).encode_crc / .encode_crc64.

Reaching a cell (REACH: cell -> (k, rows, form of parity row 0)); only
ISAL_HIP_CRC_TILES and ISAL_HIP_LOG are set, the mapping is the library's own:
  * U is the largest of 12, 10, 8, 6, 5, 4 that divides k, else 4
    (fused_group, crc_device.h);
  * X0 = 1 when parity row 0 is all 0/1 (isal_hip_xor_rows). The X0 = 1 cells
    use a 0/1 *mix* (ones at the first and the last source, at least one
    zero, so x0src is not all ones), the X0 = 0 cells a general row 0. All
    other rows are seeded random bytes with a 0 and a 1 entry planted. The
    coefficient bytes are built directly (encode needs no invertibility);
  * NV follows fused_nv32(k) / fused_nv(1, k): k = U gives NV = 2 in both
    families, NV1_K names the k that gives NV = 1. For CRC64 (k <= 32) the
    only multiples of 4 whose load group is 4 are k = 4 and k = 28, and both
    give NV = 2, so its U = 4, NV = 1 cells run at the remainder k = 14
    (12 + two singles);
  * the SRC = 0 cells run rows = 8 + P at k = U: that step launches
    <8, U, 1, X0, 4, 2> and then <P, U, 0, 0, 0, 1>, and the log must name
    both in that order. Row 0 of those cells is general for even P and the
    0/1 mix for odd P, so the first pass runs both of its X0 forms;
  * CRC64 SL = 3: k = 10, P = 1..4, both X0.
The launch log decides: a cell whose (k, rows, form) reaches another kernel,
or the encode-then-CRC fallback, fails.

Remainder cells (U = 4 only; CRC32C peels a group of 2, then singles, CRC64
singles only): k in {7, 13, 3} at P in {2, 4, 7}, both X0.

Shape of a cell: 3 stripes, ISAL_HIP_CRC_TILES=2, len = 5 * 4096 + 48 * 16:
three blocks per stripe of 2, 2 and 1 full tiles (the cross-tile chain step,
the one-tile prefetch, the LAST / PH = 1 variant on a 2-tile and on a 1-tile
block), the ragged tile shares the last block with a full tile and has lanes
inside and past len; 9 work items, so under NV = 2 the last workgroup's second
lane group has no item. EDGE_LENS adds, at P in {2, 4, 7} of every column:
4 * 4096 + 48 * 16 (CRC32C: the ragged tile alone in its block, a zero chain),
4 * 4096 (no ragged tile, no tail) and the first length with no
ISAL_HIP_CRC_TILES (the library's own halving rule).

Layout: all shards of a cell sit in one pool, each 16-byte aligned and
followed by 64 guard bytes (64 more in front of the first); parity and guards
are pre-filled with a poison byte, and after the run the *whole pool* is
compared with a host image of sources, oracle parity and untouched poison.

Reference: oracle.encode for parity, oracle.crc32_iscsi / oracle.crc64 on the
sources and on the oracle's parity for every one of the k + rows checksums,
with an init that is neither zero nor all ones. Never the engine's output.
Equality is exact.

CRC64 flavours: a cell <P, U, X0, SL, NV> runs variant (P + index of U in
GROUPS + X0) % 8. A column of 8 rows at one (U, X0, NV) therefore runs all
eight flavours, the U = 10 columns (P <= 4 pipelined, P >= 5 not) together do,
and at every P the X0 = 0 and X0 = 1 cells differ in parity of the variant:
one is a reflected flavour, the other a normal (byte-swapped chain) one.

Proof of which kernel ran (Launches): under ISAL_HIP_LOG=2 the step's
`isal_hip: kernel` lines are exactly the cell's name(s), and
kernel_launches() grows by the fused pass(es) plus COMBINE_LAUNCHES.
"""
import functools

import numpy as np
import pytest
import torch

from ecutil import fill_bytes

pytestmark = pytest.mark.gpu

# ---- the declared cells (plain data; importable without a GPU) ---------------

CRC32C, CRC64 = "ec_encode_crc_v16", "ec_encode_crc64_v16"
ROWS = tuple(range(1, 9))
GROUPS = (12, 10, 8, 6, 5, 4)  # fused_group's candidates
PIPELINED_ROWS = tuple(range(1, 5))  # CRC64, U = 10: SL = 3

# the (SRC, X0, NB, NV) tails of ec_encode_crc_v16<P, U, ...>
CRC32C_VARIANTS = ((0, 0, 0, 1), (1, 0, 4, 2), (1, 1, 4, 2), (1, 0, 4, 1), (1, 1, 4, 1))


def crc64_variants(P, U):
    """The (X0, SL, NV) tails of ec_encode_crc64_v16<P, U, ...>."""
    if U == 10 and P in PIPELINED_ROWS:
        return ((0, 3, 1), (1, 3, 1))
    return ((0, 1, 2), (1, 1, 2), (0, 1, 1), (1, 1, 1))


CELLS = {
    CRC32C: {(P, U) + v for P in ROWS for U in GROUPS for v in CRC32C_VARIANTS},
    CRC64: {(P, U) + v for P in ROWS for U in GROUPS for v in crc64_variants(P, U)},
}

# Built cells that no (k, rows, coefficients) reaches through the batch calls
UNREACHABLE = {CRC32C: set(), CRC64: set()}

# k with k's load group == U and NV == 1 (fused_nv32(k) / fused_nv(1, k));
# CRC64 with U = 4: a remainder k (12 + two singles)
NV1_K = {
    CRC32C: {12: 36, 10: 30, 8: 32, 6: 42, 5: 35, 4: 28},
    CRC64: {12: 24, 10: 20, 8: 16, 6: 18, 5: 15, 4: 14},
}

# launches of one call beside the fused pass(es), counted by the launchers'
# isal_hip_count_launch: crc32c_combine / crc64_combine
COMBINE_LAUNCHES = {CRC32C: 1, CRC64: 1}
ROWS_PER_PASS = 8

GENERAL, MIX = "general", "mix"  # parity row 0: any bytes / a 0/1 mix


def group_of(k):
    """fused_group (crc_device.h)."""
    for u in GROUPS:
        if k >= u and k % u == 0:
            return u
    return 4


def _reach32(cell):
    P, U, SRC, X0, _, NV = cell
    if not SRC:
        return U, ROWS_PER_PASS + P, MIX if P % 2 else GENERAL
    return (U if NV == 2 else NV1_K[CRC32C][U]), P, MIX if X0 else GENERAL


def _reach64(cell):
    P, U, X0, SL, NV = cell
    return (U if NV == 2 or SL == 3 else NV1_K[CRC64][U]), P, MIX if X0 else GENERAL


# cell -> (k, rows, form of row 0)
REACH = {
    CRC32C: {c: _reach32(c) for c in CELLS[CRC32C]},
    CRC64: {c: _reach64(c) for c in CELLS[CRC64]},
}

# Remainder groups (U = 4): family -> {k: the NV that k gives}
REMAINDER_ROWS = (2, 4, 7)
REMAINDER_K = {CRC32C: {7: 2, 13: 2, 3: 2}, CRC64: {7: 2, 13: 1, 3: 2}}


def remainder_cell(family, k, P, X0):
    NV = REMAINDER_K[family][k]
    return (P, 4, 1, X0, 4, NV) if family == CRC32C else (P, 4, X0, 1, NV)


def crc64_variant(cell):
    """The crc64 flavour a CRC64 cell runs (see the module docstring)."""
    P, U, X0 = cell[:3]
    return (P + GROUPS.index(U) + X0) % 8


TILE = 4096
STRIPES = 3
TILES_KNOB = 2
CELL_LEN = 5 * TILE + 48 * 16
# (len, ISAL_HIP_CRC_TILES or None for the library's own rule)
EDGE_ROWS = (2, 4, 7)
EDGE_LENS = ((4 * TILE + 48 * 16, TILES_KNOB), (4 * TILE, TILES_KNOB), (5 * TILE + 768, None))

GUARD = 64
POISON = 0xA5
INIT32 = 0x9E3779B9
INIT64 = 0x0123456789ABCDEF


def name_of(family, cell):
    return f"{family}<{', '.join(str(x) for x in cell)}>"


def launched_names(family, cell, rows, form):
    """The kernel lines one call of the cell's step prints, in order."""
    if family == CRC32C and rows > ROWS_PER_PASS:
        first = (ROWS_PER_PASS, cell[1], 1, int(form == MIX), 4, 2)
        assert first in CELLS[CRC32C] and rows - ROWS_PER_PASS == cell[0]
        return [name_of(family, first), name_of(family, cell)]
    return [name_of(family, cell)]


def coefficients(k, rows, form, seed):
    """rows x k coefficient bytes: row 0 of the given form, every other row
    seeded random bytes with a 0 and a 1 entry planted."""
    assert k >= 3
    c = fill_bytes(rows * k, 0xC0EF + seed).reshape(rows, k).copy()
    for l in range(1, rows):
        c[l, l % k], c[l, (l + 1) % k] = 0, 1
    if form == MIX:
        c[0] = fill_bytes(k, 0x0101 + seed) & 1
        c[0, 0], c[0, k - 1], c[0, 1] = 1, 1, 0
        assert c[0].max() <= 1 and 0 < int(c[0].sum()) < k
    else:
        c[0, 0], c[0, k - 1], c[0, 1] = 0, 1, 0x8E
        assert c[0].max() > 1
    return c.reshape(-1)


# ---- running one cell ---------------------------------------------------------

@pytest.fixture(autouse=True)
def _reload_knobs_after(engine):
    """Knobs are read once by the library: every test leaves it re-synced with
    os.environ."""
    yield
    engine.reload_config()


def _knobs(engine, monkeypatch, tiles):
    monkeypatch.delenv("ISAL_HIP_CRC_XROWS", raising=False)
    monkeypatch.setenv("ISAL_HIP_LOG", "2")
    if tiles is None:
        monkeypatch.delenv("ISAL_HIP_CRC_TILES", raising=False)
    else:
        monkeypatch.setenv("ISAL_HIP_CRC_TILES", str(tiles))
    engine.reload_config()


class Launches:
    """What one step launched: the kernel lines of the log must be exactly
    `names`, in order, and kernel_launches() must grow by them plus `extra`."""

    def __init__(self, engine, capfd, what):
        self.engine, self.capfd, self.what = engine, capfd, what

    def __call__(self, step, names, extra):
        torch.cuda.synchronize()
        self.capfd.readouterr()
        before = self.engine.kernel_launches()
        step()
        torch.cuda.synchronize()
        grew = self.engine.kernel_launches() - before
        err = self.capfd.readouterr().err
        named = [line.split("kernel ", 1)[1] for line in err.splitlines() if line.startswith("isal_hip: kernel ")]
        assert named == names, (self.what, "launched", named)
        assert grew == len(names) + extra, (self.what, "kernel_launches grew by", grew)


@functools.lru_cache(maxsize=None)
def _source(s, j):
    """Source shard j of stripe s at the longest length, shared by every cell
    (a shorter cell takes its head); read-only."""
    a = fill_bytes(max(CELL_LEN, *(n for n, _ in EDGE_LENS)), 7919 * s + 31 * j + 5)
    a.setflags(write=False)
    return a


def _first_difference(got, want, n, nsh):
    """Where two pool images differ first: which shard or guard, which byte."""
    at = int(np.flatnonzero(got != want)[0])
    slot, off = divmod(at - GUARD, n + GUARD) if at >= GUARD else (-1, at)
    where = "the guard in front of the pool" if slot < 0 else (
        f"stripe {slot // nsh} shard {slot % nsh} " + (f"byte {off}" if off < n else f"guard byte {off - n}"))
    return f"pool byte {at}: {where}: got {int(got[at]):#04x}, want {int(want[at]):#04x}"


def run_cell(engine, oracle, gpu, capfd, family, cell, k, rows, form, n):
    """One call of encode_crc / encode_crc64 over STRIPES stripes of n bytes:
    which kernels ran, the whole pool, every checksum."""
    what = f"{name_of(family, cell)} k={k} rows={rows} row0={form} len={n}"
    assert n % 16 == 0 and n >= TILE
    nsh, stride = k + rows, n + GUARD
    coef = coefficients(k, rows, form, 100 * k + rows)
    tbls = engine.ec_init_tables(k, rows, coef)
    image = np.full(GUARD + STRIPES * nsh * stride, POISON, np.uint8)

    def at(s, i):
        return GUARD + (s * nsh + i) * stride

    data = [[_source(s, j)[:n] for j in range(k)] for s in range(STRIPES)]
    for s in range(STRIPES):
        for j in range(k):
            image[at(s, j):at(s, j) + n] = data[s][j]
    pool = torch.from_numpy(image).to(gpu)
    base = int(pool.data_ptr())
    assert base % 16 == 0 and all(at(s, i) % 16 == 0 for s in range(STRIPES) for i in range(nsh))
    dptr = [base + at(s, j) for s in range(STRIPES) for j in range(k)]
    cptr = [base + at(s, k + l) for s in range(STRIPES) for l in range(rows)]
    if family == CRC32C:
        init, mask = INIT32 ^ cell[0], 0xFFFFFFFF
        out = torch.zeros(STRIPES * nsh, dtype=torch.int32, device=gpu)
        reference = lambda buf: oracle.crc32_iscsi(buf, init)  # noqa: E731
    else:
        variant, init, mask = crc64_variant(cell), INIT64 ^ cell[0], 0xFFFFFFFFFFFFFFFF
        out = torch.zeros(STRIPES * nsh, dtype=torch.int64, device=gpu)
        reference = lambda buf: oracle.crc64(variant, buf, init)  # noqa: E731
        what += f" crc64_{engine.CRC64_VARIANTS[variant]}"
    assert init not in (0, mask)
    b = engine.Batch(n, k, rows, tbls, STRIPES, dptr, cptr)
    try:
        step = (lambda: b.encode_crc(init, out, 0)) if family == CRC32C else (
            lambda: b.encode_crc64(variant, init, out, 0))
        passes = launched_names(family, cell, rows, form)
        assert len(passes) == (rows + ROWS_PER_PASS - 1) // ROWS_PER_PASS
        Launches(engine, capfd, what)(step, passes, COMBINE_LAUNCHES[family])
    finally:
        b.close()
    want = []
    for s in range(STRIPES):
        parity = oracle.encode(coef, k, rows, data[s])
        for l in range(rows):
            image[at(s, k + l):at(s, k + l) + n] = parity[l]
        want += [reference(buf) for buf in data[s] + parity]
    got_pool = pool.cpu().numpy()
    assert np.array_equal(got_pool, image), (what, _first_difference(got_pool, image, n, nsh))
    got = [int(v) & mask for v in out.tolist()]
    wrong = [(i // nsh, i % nsh, hex(got[i]), hex(want[i])) for i in range(len(want)) if got[i] != want[i]]
    assert not wrong, (what, "(stripe, shard, got, want)", wrong[:4])


def _column(family, U, tail):
    """The cells of `family` with load group U and the given last arguments, by P."""
    return sorted(c for c in CELLS[family] if c[1] == U and c[2:] == tuple(tail))


def _run_column(engine, oracle, gpu, monkeypatch, capfd, family, cells, shapes):
    assert cells and not set(cells) & UNREACHABLE[family]
    for cell in cells:
        k, rows, form = REACH[family][cell]
        for n, tiles in shapes:
            _knobs(engine, monkeypatch, tiles)
            run_cell(engine, oracle, gpu, capfd, family, cell, k, rows, form, n)


CRC64_COLUMNS = sorted({(c[1],) + c[2:] for c in CELLS[CRC64]}, reverse=True)  # (U, X0, SL, NV)


# The NV = 1 columns run at k up to 42, where the oracle's encode of 8 row
# counts takes as long as two of the slowest column tests of
# test_kernel_matrix_gpu.py: every CRC32C column is two tests, by P range.
ROW_HALVES = (ROWS[:4], ROWS[4:])


@pytest.mark.parametrize("rows", ROW_HALVES, ids=lambda r: f"P{r[0]}-{r[-1]}")
@pytest.mark.parametrize("tail", CRC32C_VARIANTS, ids=lambda t: "SRC%d-X0%d-NB%d-NV%d" % t)
@pytest.mark.parametrize("U", GROUPS)
def test_fused_crc32c_every_rows_of_a_column(engine, oracle, gpu, monkeypatch, capfd, U, tail, rows):
    assert sum(ROW_HALVES, ()) == ROWS
    cells = [c for c in _column(CRC32C, U, tail) if c[0] in rows]
    assert [c[0] for c in cells] == list(rows)
    _run_column(engine, oracle, gpu, monkeypatch, capfd, CRC32C, cells, [(CELL_LEN, TILES_KNOB)])


@pytest.mark.parametrize("tail", CRC32C_VARIANTS, ids=lambda t: "SRC%d-X0%d-NB%d-NV%d" % t)
@pytest.mark.parametrize("U", GROUPS)
def test_fused_crc32c_edge_lengths(engine, oracle, gpu, monkeypatch, capfd, U, tail):
    cells = [c for c in _column(CRC32C, U, tail) if c[0] in EDGE_ROWS]
    assert [c[0] for c in cells] == list(EDGE_ROWS)
    _run_column(engine, oracle, gpu, monkeypatch, capfd, CRC32C, cells, EDGE_LENS)


@pytest.mark.parametrize("column", CRC64_COLUMNS, ids=lambda c: "U%d-X0%d-SL%d-NV%d" % c)
def test_fused_crc64_every_rows_of_a_column(engine, oracle, gpu, monkeypatch, capfd, column):
    cells = _column(CRC64, column[0], column[1:])
    pipelined = [P for P in ROWS if (P in PIPELINED_ROWS) == (column[2] == 3)]
    assert [c[0] for c in cells] == (pipelined if column[0] == 10 else list(ROWS))
    _run_column(engine, oracle, gpu, monkeypatch, capfd, CRC64, cells, [(CELL_LEN, TILES_KNOB)])


@pytest.mark.parametrize("column", CRC64_COLUMNS, ids=lambda c: "U%d-X0%d-SL%d-NV%d" % c)
def test_fused_crc64_edge_lengths(engine, oracle, gpu, monkeypatch, capfd, column):
    cells = [c for c in _column(CRC64, column[0], column[1:]) if c[0] in EDGE_ROWS]
    _run_column(engine, oracle, gpu, monkeypatch, capfd, CRC64, cells, EDGE_LENS)


@pytest.mark.parametrize("X0", [0, 1])
@pytest.mark.parametrize("k", sorted(REMAINDER_K[CRC32C]))
@pytest.mark.parametrize("family", [CRC32C, CRC64])
def test_fused_crc_remainder_groups(engine, oracle, gpu, monkeypatch, capfd, family, k, X0):
    assert k % 4 and group_of(k) == 4
    for P in REMAINDER_ROWS:
        cell = remainder_cell(family, k, P, X0)
        assert cell in CELLS[family]
        _knobs(engine, monkeypatch, TILES_KNOB)
        run_cell(engine, oracle, gpu, capfd, family, cell, k, P, MIX if X0 else GENERAL, CELL_LEN)
