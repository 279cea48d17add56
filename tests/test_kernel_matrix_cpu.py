"""CPU tier: the kernel matrix is complete, checked without a GPU.

tests/test_kernel_matrix_gpu.py declares, as plain data (CELLS), the template
arguments of every instantiation of the repair, ragged, scrub and overwrite
kernels, and launches every declared cell. Here the declared set is held equal
to the set the ec_kernels code object was built with, read from its kernel
descriptors (*.kd): a new load-group candidate, row count or flag with no cell
fails, and so does a cell that names a kernel that is not built. Only kernel
names are examined, no instructions.
"""
import os
import re

import pytest

from test_kernel_matrix_gpu import CELLS, ENC_REMAINDER, HAND_WRITTEN, REMAINDER_ROWS, VERIFY_REMAINDER, enc_block
from test_kernel_objects_cpu import BUILD, LLVM, _device_kernels, _run

EC_OBJECT = os.path.join(BUILD, "ec_kernels.o")

INT = r"Li(\d+)E"
POLICY = rf"NS_6EncPolI{INT}{INT}{INT}{INT}EE"  # EncPol<U, LD, ST, ORDER>
# family -> its template argument list in the Itanium mangling; the groups of
# CELL[family] are the ones a cell is made of, the rest is the policy's tail
MANGLED = {
    "ec_repair_v16": rf"I{INT}{POLICY}{INT}E",
    "ec_encode_rag": rf"I{INT}{POLICY}{INT}E",
    "ec_repair_rag": rf"I{INT}{POLICY}{INT}E",
    "ec_verify_rag": rf"I{INT}{POLICY}E",
    "ec_locate_rag": rf"I{INT}{POLICY}E",
    "ec_verify_v16": rf"I{INT}{POLICY}{INT}E",
    "ec_locate_v16": rf"I{INT}{POLICY}{INT}E",
    "ec_overwrite_v16": rf"I{INT}Lb([01])E{INT}E",
}
CELL = {f: (0, 1, 5) for f in MANGLED}  # P, U, then B or FL behind the policy
CELL.update({"ec_verify_rag": (0, 1), "ec_locate_rag": (0, 1), "ec_overwrite_v16": (0, 1, 2)})
EXPECTED = {"ec_repair_v16": 48, "ec_encode_rag": 48, "ec_repair_rag": 48, "ec_verify_rag": 32, "ec_locate_rag": 28,
            "ec_verify_v16": 64, "ec_locate_v16": 56, "ec_overwrite_v16": 16}


def built_cells(kernels, mangled=None, cell=None):
    """family -> [(cell, policy tail)] for every kernel name of the families,
    cell as CELLS spells it. A name of a family that the pattern does not
    match is an error: it would be an instantiation this module cannot see.
    mangled and cell: another matrix's families (test_encode_matrix_cpu.py)
    in place of this module's MANGLED and CELL."""
    mangled, cell = mangled or MANGLED, cell or CELL
    out = {f: [] for f in mangled}
    for name in sorted(kernels):
        for family, args in mangled.items():
            m = re.search(rf"\d+{family}I", name)
            if not m:
                continue
            m = re.search(rf"{len(family)}{family}{args}Ev", name)
            assert m, f"{name}: template arguments of {family} not understood"
            g = [int(x) for x in m.groups()]
            out[family].append((tuple(g[i] for i in cell[family]), tuple(x for i, x in enumerate(g)
                                                                       if i not in cell[family])))
    return out


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    if not os.path.exists(EC_OBJECT) or not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")):
        pytest.skip("kernel objects not built here (make -C isa-l_amd)")
    d = tmp_path_factory.mktemp("matrix")
    fb, co = d / "ec_kernels.fatbin", d / "ec_kernels.co"
    _run(f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", EC_OBJECT, str(d / "ec_kernels.tmp.o"))
    _run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fb}",
         "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}")
    return built_cells(_device_kernels(str(co)))


@pytest.mark.parametrize("family", sorted(MANGLED))
def test_built_instantiations_equal_the_declared_cells(built, family):
    cells = {c for c, _ in built[family]}
    declared = CELLS[family]
    assert cells - declared == set(), f"{family}: built with no cell in the matrix: {sorted(cells - declared)}"
    assert declared - cells == set(), f"{family}: cells that name no built kernel: {sorted(declared - cells)}"
    assert len(cells) == EXPECTED[family], (family, len(cells))
    # ec_verify_v16 is also launched by the drop-in and kernel-argument forms,
    # with the batch form's template arguments: a set, not a count. Elsewhere
    # one kernel per cell: a second policy behind a cell would have no cell.
    tails = {t for _, t in built[family]}
    assert len(tails) <= 1, f"{family}: more than one load/store/order policy built: {sorted(tails)}"
    if family != "ec_verify_v16":
        assert len(built[family]) == len(cells), (family, len(built[family]), len(cells))


def test_the_name_patterns_read_template_arguments():
    """The parser itself, on names spelled the way the compiler spells them."""
    names = {"_ZN12_GLOBAL__N_113ec_repair_v16ILi7ENS_6EncPolILi4ELi2ELi2ELi2EEELi256EEEvPKmiPKjS6_jiiijj",
             "_ZN12_GLOBAL__N_113ec_verify_ragILi3ENS_6EncPolILi6ELi2ELi2ELi0EEEEEvPKmiPK15HIP_vector_typeIjLj2EEPKiPKjiiijPy",
             "_ZN12_GLOBAL__N_113ec_locate_v16ILi8ENS_6EncPolILi10ELi2ELi2ELi0EEELi1EEEvPKmiPKjiijjyjPKhPj",
             "_ZN12_GLOBAL__N_116ec_overwrite_v16ILi1ELb1ELi128EEEvPKmiPKjS4_iiijj",
             "_ZN12_GLOBAL__N_113ec_encode_v16ILi1ENS_6EncPolILi4ELi2ELi2ELi2EEELi0ELi128EEEvPKmiiiPKjiijjyj"}
    got = built_cells(names)
    assert got["ec_repair_v16"] == [((7, 4, 256), (2, 2, 2))]
    assert got["ec_verify_rag"] == [((3, 6), (2, 2, 0))]
    assert got["ec_locate_v16"] == [((8, 10, 1), (2, 2, 0))]
    assert got["ec_overwrite_v16"] == [((1, 1, 128), ())]
    assert sum(len(v) for v in got.values()) == 4
    with pytest.raises(AssertionError, match="not understood"):
        built_cells({"_ZN12_GLOBAL__N_113ec_verify_ragILi3ELb1ENS_6EncPolILi6ELi2ELi2ELi0EEEEEvPKm"})


def test_the_tables_are_consistent():
    """Every written-out body and every remainder cell is a declared cell, and
    a remainder k does leave a remainder."""
    for family, cells in HAND_WRITTEN.items():
        assert cells <= CELLS[family], family
        for k, _, U in ENC_REMAINDER:
            assert k % U and {(P, U, enc_block(P)) for P in REMAINDER_ROWS} <= CELLS[family]
    assert any(U == 4 and 7 in REMAINDER_ROWS for _, _, U in ENC_REMAINDER)  # the written-out <7, 4> bodies
    for k, _, U in VERIFY_REMAINDER:
        assert k % U and {(P, U) for P in REMAINDER_ROWS} <= CELLS["ec_verify_rag"]
