"""CPU tier: the fused checksum kernel matrix is complete, checked without a GPU.

tests/test_fused_crc_matrix_gpu.py declares, as plain data (CELLS), the
template arguments of every instantiation of the fused encode + CRC32C and
encode + CRC64 kernels, and launches every declared cell that its REACH table
reaches. Here the declared set is held equal to the set the crc_fused_p1..8
and crc64_fused_p1..8 objects were built with, read from their kernel
descriptors (*.kd): a new load-group candidate, row count, lane-group count or
flag with no cell fails, and so does a cell that names a kernel that is not
built. Only kernel names are examined, no instructions.

The counts: ec_encode_crc_v16 8 P x 6 U x 5 = 240 (the second pass of
rows > 8, and X0 x NV with source chains); ec_encode_crc64_v16 8 x 6 x 4 = 192
less the 4 x 2 that load group 10 with P <= 4 does not build (there one
pipelined kernel per X0 replaces the NV pair) = 184.

The reach table is checked in pure Python: every cell is reached or declared
unreachable, the k of a cell maps to its U by the divisor rule, the remainder
k do leave a remainder, and the CRC64 flavours cycle as the GPU module says.
"""
import glob
import os
import re

import pytest

import test_fused_crc_matrix_gpu as fused
from test_fused_crc_matrix_gpu import CELLS, CRC32C, CRC64, REACH, UNREACHABLE
from test_kernel_objects_cpu import BUILD, LLVM, _device_kernels, _run

OBJECTS = {CRC32C: "crc_fused_p*.o", CRC64: "crc64_fused_p*.o"}
EXPECTED = {CRC32C: 240, CRC64: 184}

INT = r"Li(\d+)E"
BOOL = r"Lb([01])E"
POLICY = rf"NS_6EncPolI{INT}{INT}{INT}{INT}EE"  # EncPol<U, LD, ST, ORDER>
# family -> its template argument list in the Itanium mangling
MANGLED = {
    CRC32C: rf"I{INT}{POLICY}{BOOL}{BOOL}{BOOL}{INT}{INT}E",  # P, FusedPol<U>, REG, SRC, X0, NB, NV
    CRC64: rf"I{INT}{INT}{BOOL}{INT}{INT}E",  # P, U, X0, SL, NV
}
# the groups a cell is made of, in CELLS' order; the rest is the policy's tail and REG
CELL = {CRC32C: (0, 1, 6, 7, 8, 9), CRC64: (0, 1, 2, 3, 4)}
REG = {CRC32C: 5}  # the group that holds REG


def built_cells(kernels):
    """family -> [(cell, the other template arguments)] for every kernel name
    of the two families, cell as CELLS spells it. A name of a family that the
    pattern does not match is an error: it would be an instantiation this
    module cannot see."""
    out = {f: [] for f in MANGLED}
    for name in sorted(kernels):
        for family, args in MANGLED.items():
            if not re.search(rf"\d+{family}I", name):
                continue
            m = re.search(rf"{len(family)}{family}{args}Ev", name)
            assert m, f"{name}: template arguments of {family} not understood"
            g = [int(x) for x in m.groups()]
            out[family].append((tuple(g[i] for i in CELL[family]),
                                tuple(x for i, x in enumerate(g) if i not in CELL[family])))
    return out


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    objects = {f: sorted(glob.glob(os.path.join(BUILD, pat))) for f, pat in OBJECTS.items()}
    if not all(objects.values()) or not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")):
        pytest.skip("kernel objects not built here (make -C isa-l_amd)")
    d = tmp_path_factory.mktemp("fused")
    kernels, per_object = set(), {}
    for family, objs in objects.items():
        assert len(objs) == 8, (family, objs)
        for o in objs:
            stem = os.path.basename(o)[:-2]
            fb, co = d / f"{stem}.fatbin", d / f"{stem}.co"
            _run(f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", o, str(d / f"{stem}.tmp.o"))
            _run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fb}",
                 "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}")
            per_object[stem] = _device_kernels(str(co))
            kernels |= per_object[stem]
    return built_cells(kernels), per_object


@pytest.mark.parametrize("family", sorted(MANGLED))
def test_built_instantiations_equal_the_declared_cells(built, family):
    cells = {c for c, _ in built[0][family]}
    declared = CELLS[family]
    assert cells - declared == set(), f"{family}: built with no cell in the matrix: {sorted(cells - declared)}"
    assert declared - cells == set(), f"{family}: cells that name no built kernel: {sorted(declared - cells)}"
    assert len(cells) == EXPECTED[family], (family, len(cells))
    # one kernel per cell: a second memory policy (or REG form) behind a cell
    # would be an instantiation with no cell
    assert len(built[0][family]) == len(cells), (family, len(built[0][family]), len(cells))
    tails = {t for _, t in built[0][family]}
    assert len(tails) == 1, f"{family}: more than one memory policy / REG form built: {sorted(tails)}"
    if family in REG:
        other = [i for i in range(10) if i not in CELL[family]]
        assert next(iter(tails))[other.index(REG[family])] == 0, f"{family}: a REG = true kernel is built"


def test_each_object_holds_the_kernels_of_its_own_row_count(built):
    """crc_fused_pP.o and crc64_fused_pP.o hold exactly the cells with that P."""
    for stem, kernels in built[1].items():
        P = int(stem.rsplit("_p", 1)[1])
        family = CRC64 if stem.startswith("crc64") else CRC32C
        cells = {c for c, _ in built_cells(kernels)[family]}
        assert cells == {c for c in CELLS[family] if c[0] == P}, stem


def test_the_name_patterns_read_template_arguments():
    """The parser itself, on names spelled the way the compiler spells them."""
    names = {"_ZN12_GLOBAL__N_117ec_encode_crc_v16ILi3ENS_6EncPolILi10ELi1ELi1ELi0EEELb0ELb1ELb1ELi4ELi2EEEvPKmiiiPKjiijjjjjyS6_PjS7_iii",
             "_ZN12_GLOBAL__N_117ec_encode_crc_v16ILi7ENS_6EncPolILi4ELi1ELi1ELi0EEELb0ELb0ELb0ELi0ELi1EEEvPKmiiiPKjiijjjjjyS6_PjS7_iii",
             "_ZN12_GLOBAL__N_119ec_encode_crc64_v16ILi3ELi10ELb1ELi3ELi1EEEvPKmiPKjiijjjjiyiS2_Pm",
             "_ZN12_GLOBAL__N_119ec_encode_crc64_v16ILi6ELi5ELb0ELi1ELi2EEEvPKmiPKjiijjjjiyiS2_Pm",
             "_ZN12_GLOBAL__N_116crc64_shards_preEPKmiiijjjiS1_Pm"}
    got = built_cells(names)
    assert got[CRC32C] == [((3, 10, 1, 1, 4, 2), (1, 1, 0, 0)), ((7, 4, 0, 0, 0, 1), (1, 1, 0, 0))]
    assert got[CRC64] == [((3, 10, 1, 3, 1), ()), ((6, 5, 0, 1, 2), ())]
    for cell, _ in got[CRC32C]:
        assert cell in CELLS[CRC32C]
    for cell, _ in got[CRC64]:
        assert cell in CELLS[CRC64]
    with pytest.raises(AssertionError, match="not understood"):  # a template argument more
        built_cells({"_ZN12_GLOBAL__N_119ec_encode_crc64_v16ILi3ELi10ELb1ELb0ELi3ELi1EEEvPKmiPKjiijjjjiyiS2_Pm"})
    with pytest.raises(AssertionError, match="not understood"):  # the policy spelled out of place
        built_cells({"_ZN12_GLOBAL__N_117ec_encode_crc_v16ILi3ELi10ELb0ELb1ELb1ELi4ELi2EEEvPKmiii"})


def test_the_declared_counts():
    assert {f: len(c) for f, c in CELLS.items()} == EXPECTED
    for family, cells in CELLS.items():
        assert {c[0] for c in cells} == set(fused.ROWS) and {c[1] for c in cells} == set(fused.GROUPS)


@pytest.mark.parametrize("family", sorted(MANGLED))
def test_every_cell_is_reached_or_declared_unreachable(family):
    assert UNREACHABLE[family] <= CELLS[family]
    assert set(REACH[family]) | UNREACHABLE[family] == CELLS[family]
    limit = {CRC32C: 64, CRC64: 32}[family]  # the largest fused k
    for cell in CELLS[family] - UNREACHABLE[family]:
        k, rows, form = REACH[family][cell]
        assert 3 <= k <= limit and form in (fused.GENERAL, fused.MIX), (cell, k, form)
        assert fused.group_of(k) == cell[1], (cell, k)  # the divisor rule
        x0 = cell[3] if family == CRC32C else cell[2]
        if family == CRC32C and not cell[2]:  # SRC = 0: the second pass of rows = 8 + P
            assert rows == fused.ROWS_PER_PASS + cell[0] and k == cell[1], cell
            first = fused.launched_names(family, cell, rows, form)[0]
            assert first == fused.name_of(family, (8, cell[1], 1, int(form == fused.MIX), 4, 2)), cell
        else:
            assert rows == cell[0] and (form == fused.MIX) == bool(x0), cell
            assert fused.launched_names(family, cell, rows, form) == [fused.name_of(family, cell)]
        if cell[-1] == 2 or (family == CRC64 and cell[3] == 3):  # NV = 2, the pipelined path: k = U
            assert k == cell[1], cell
        elif family == CRC32C and not cell[2]:
            pass
        else:  # NV = 1: a larger k of the same group
            assert k == fused.NV1_K[family][cell[1]] > cell[1], cell


def test_both_first_pass_forms_run_in_front_of_the_second_pass():
    for U in fused.GROUPS:
        forms = {REACH[CRC32C][c][2] for c in CELLS[CRC32C] if c[1] == U and not c[2]}
        assert forms == {fused.GENERAL, fused.MIX}, U


def test_remainder_cells_leave_a_remainder():
    """Only U = 4 has a remainder; every remainder k leaves one, and so does
    the k that reaches the NV = 1 cells of the CRC64 load group 4."""
    assert fused.NV1_K[CRC64][4] % 4 and fused.group_of(fused.NV1_K[CRC64][4]) == 4
    for family, ks in fused.REMAINDER_K.items():
        assert sorted(ks) == [3, 7, 13]
        for k, NV in ks.items():
            assert k % 4 and fused.group_of(k) == 4 and NV in (1, 2)
            for P in fused.REMAINDER_ROWS:
                for X0 in (0, 1):
                    assert fused.remainder_cell(family, k, P, X0) in CELLS[family]
    assert fused.REMAINDER_ROWS == (2, 4, 7) and fused.EDGE_ROWS == (2, 4, 7)


def test_crc64_flavours_cycle_over_the_cells():
    """All eight flavours in every U column, a reflected (even) and a normal
    (odd) one at every P."""
    for U in fused.GROUPS:
        assert {fused.crc64_variant(c) for c in CELLS[CRC64] if c[1] == U} == set(range(8)), U
        for P in fused.ROWS:
            parities = {fused.crc64_variant(c) % 2 for c in CELLS[CRC64] if c[1] == U and c[0] == P}
            assert parities == {0, 1}, (U, P)


def test_the_shape_has_the_blocks_the_cells_are_about():
    """The geometry the GPU module's docstring promises, by the library's rule
    (isal_hip_crc_geometry / isal_hip_crc64_geometry)."""
    T, tt = fused.TILE, fused.TILES_KNOB
    n = fused.CELL_LEN
    assert n % 16 == 0 and n // T == 5 and 0 < n % T < T - 16 * 16
    assert -(-(n // T + 1) // tt) == 3 and -(-(n // T) // tt) == 3  # CRC32C counts the ragged tile, CRC64 does not
    assert fused.STRIPES * 3 == 9  # odd: the last NV = 2 workgroup has one item
    (a, ta), (b, tb), (c, tc) = fused.EDGE_LENS
    assert (a // T, a % T, ta) == (4, 48 * 16, tt) and -(-(a // T + 1) // tt) == 3  # ragged tile alone
    assert (b // T, b % T, tb) == (4, 0, tt)
    assert c == n and tc is None
    assert fused.GUARD >= 64 and fused.GUARD % 16 == 0
