"""CPU tier: the ragged overwrite's kernels in the built code object, checked
without a GPU.

tests/test_overwrite_ragged_matrix_gpu.py declares, as plain data (CELLS), the
template arguments of every ec_overwrite_rag instantiation and launches every
declared cell. Here the declared set is held equal to the set the ec_kernels
code object was built with, read from its kernel descriptors (*.kd): exactly
16 kernels, P 1..8 x COMMIT 0/1 at 128 lanes. Only kernel names are examined,
no instructions.
"""
import os
import re

import pytest

from test_kernel_objects_cpu import BUILD, LLVM, _device_kernels, _run
from test_overwrite_ragged_matrix_gpu import CELLS

EC_OBJECT = os.path.join(BUILD, "ec_kernels.o")
FAMILY = "ec_overwrite_rag"
ARGS = r"ILi(\d+)ELb([01])ELi(\d+)EEEv"  # <P, COMMIT, B>, the end of the nested name, void


def built_cells(kernels):
    """(P, COMMIT, B) of every kernel name of the family. A name of the family
    that the pattern does not match is an error: it would be an instantiation
    this module cannot see."""
    out = []
    for name in sorted(kernels):
        if not re.search(rf"\d+{FAMILY}I", name):
            continue
        m = re.search(rf"{len(FAMILY)}{FAMILY}{ARGS}", name)
        assert m, f"{name}: template arguments of {FAMILY} not understood"
        out.append(tuple(int(x) for x in m.groups()))
    return out


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    if not os.path.exists(EC_OBJECT) or not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")):
        pytest.skip("kernel objects not built here (make -C isa-l_amd)")
    d = tmp_path_factory.mktemp("owrag")
    fb, co = d / "ec_kernels.fatbin", d / "ec_kernels.co"
    _run(f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", EC_OBJECT, str(d / "ec_kernels.tmp.o"))
    _run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fb}",
         "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}")
    return built_cells(_device_kernels(str(co)))


def test_built_ragged_overwrite_kernels_equal_the_declared_cells(built):
    cells = set(built)
    assert cells - CELLS == set(), f"built with no cell in the matrix: {sorted(cells - CELLS)}"
    assert CELLS - cells == set(), f"cells that name no built kernel: {sorted(CELLS - cells)}"
    assert len(built) == len(cells) == 16, (len(built), len(cells))
    assert cells == {(P, C, 128) for P in range(1, 9) for C in (0, 1)}


def test_the_name_pattern_reads_template_arguments():
    """The parser itself, on names spelled the way the compiler spells them;
    the uniform family's names are not this family's."""
    names = {"_ZN12_GLOBAL__N_116ec_overwrite_ragILi4ELb1ELi128EEEvPKmiPK15HIP_vector_typeIjLj2EEPKiS8_PKjSA_iij",
             "_ZN12_GLOBAL__N_116ec_overwrite_v16ILi1ELb1ELi128EEEvPKmiPKjS4_iiijj"}
    assert built_cells(names) == [(4, 1, 128)]
    with pytest.raises(AssertionError, match="not understood"):
        built_cells({"_ZN12_GLOBAL__N_116ec_overwrite_ragILi4ELi2ELb1ELi128EEEvPKm"})
