"""CPU tier: the encode, update and drop-in kernel matrix is complete, checked
without a GPU.

tests/test_encode_matrix_gpu.py declares, as plain data (CELLS), the template
arguments of every instantiation of the twelve kernels behind
isal_hip_batch_encode, isal_hip_batch_update and the drop-in calls on device
shards, and launches every declared cell that its REACH table reaches. Here
the declared set is held equal to the set the ec_kernels code object was built
with, read from its kernel descriptors (*.kd): a new load-group candidate, row
count or coefficient form with no cell fails, and so does a cell that names a
kernel that is not built. Only kernel names are examined, no instructions.

The counts (EXPECTED, written from the built object, and the products of the
launchers' template argument ranges): ec_encode_v16 8 P x 6 U x 4 FL = 192;
ec_encode_glds 4 P x 2 FL = 8; ec_encode_ldsx 5; ec_encode_karg 8 x 6 x 2 =
96; ec_verify_karg 8 x 4 x 2 = 64; ec_encode_karg_ldsx 2; the six families
with P alone 8 each. 415 in all.

The reach table is checked in pure Python: every cell is reached or declared
unreachable, a restatement of the library's dispatch (kernel_of,
karg_kernel_of) leads from every REACH entry to its cell, every knob of an
entry is needed (without it the restated rule goes elsewhere), every
remainder k leaves a remainder, and every kernel-argument cell keeps the two
limits of the argument block.
"""
import os

import pytest

import test_encode_matrix_gpu as enc
from test_encode_matrix_gpu import (B1, CELLS, GLDS, KARG, KARG4, KARG_LDSX, LDSX, REACH, UNREACHABLE, UPD_B1, UPD_KARG,
                                    UPD_V16, V16, VER_B1, VER_KARG)
from test_kernel_matrix_cpu import INT, POLICY, built_cells
from test_kernel_objects_cpu import BUILD, LLVM, _device_kernels, _run

EC_OBJECT = os.path.join(BUILD, "ec_kernels.o")

# family -> its template argument list in the Itanium mangling
MANGLED = {
    V16: rf"I{INT}{POLICY}{INT}{INT}E",  # P, EncPol<U, LD, ST, ORDER>, FL, B
    GLDS: rf"I{INT}{INT}{INT}E",  # P, R, FL
    LDSX: rf"I{INT}{INT}E",  # P, U
    B1: rf"I{INT}E",
    UPD_V16: rf"I{INT}{INT}E",  # P, B
    UPD_B1: rf"I{INT}E",
    KARG: rf"I{INT}{POLICY}{INT}E",  # P, EncPol<U, LD, ST, ORDER>, FL
    KARG4: rf"I{INT}E",
    KARG_LDSX: rf"I{INT}E",
    UPD_KARG: rf"I{INT}E",
    VER_KARG: rf"I{INT}{POLICY}{INT}E",
    VER_B1: rf"I{INT}E",
}
# the groups a cell is made of, in CELLS' order; the rest is the policy's tail
CELL = {V16: (0, 1, 5, 6), GLDS: (0, 1, 2), LDSX: (0, 1), B1: (0,), UPD_V16: (0, 1), UPD_B1: (0,), KARG: (0, 1, 5),
        KARG4: (0,), KARG_LDSX: (0,), UPD_KARG: (0,), VER_KARG: (0, 1, 5), VER_B1: (0,)}
# the one load/store/order policy of a family: kBufNT = 2, kBufSC1NT = 3
POLICY_TAIL = {V16: (2, 2, 2), KARG: (2, 3, 2), VER_KARG: (2, 2, 0)}
EXPECTED = {V16: 192, GLDS: 8, LDSX: 5, B1: 8, UPD_V16: 8, UPD_B1: 8, KARG: 96, KARG4: 8, KARG_LDSX: 2, UPD_KARG: 8,
            VER_KARG: 64, VER_B1: 8}
# the launchers' template argument ranges (ec_kernels.hip)
PRODUCT = {V16: 8 * 6 * 4, GLDS: 4 * 2, LDSX: 5, B1: 8, UPD_V16: 8, UPD_B1: 8, KARG: 8 * 6 * 2, KARG4: 8,
           KARG_LDSX: 2, UPD_KARG: 8, VER_KARG: 8 * 4 * 2, VER_B1: 8}


def _built_cells(kernels):
    return built_cells(kernels, MANGLED, CELL)


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    if not os.path.exists(EC_OBJECT) or not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")):
        pytest.skip("kernel objects not built here (make -C isa-l_amd)")
    d = tmp_path_factory.mktemp("encode_matrix")
    fb, co = d / "ec_kernels.fatbin", d / "ec_kernels.co"
    _run(f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", EC_OBJECT, str(d / "ec_kernels.tmp.o"))
    _run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fb}",
         "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}")
    return _built_cells(_device_kernels(str(co)))


@pytest.mark.parametrize("family", sorted(MANGLED))
def test_built_instantiations_equal_the_declared_cells(built, family):
    cells = {c for c, _ in built[family]}
    declared = CELLS[family]
    assert cells - declared == set(), f"{family}: built with no cell in the matrix: {sorted(cells - declared)}"
    assert declared - cells == set(), f"{family}: cells that name no built kernel: {sorted(declared - cells)}"
    assert len(cells) == EXPECTED[family], (family, len(cells))
    # one kernel per cell: a second memory policy behind a cell would be an
    # instantiation with no cell
    assert len(built[family]) == len(cells), (family, len(built[family]), len(cells))
    tails = {t for _, t in built[family]}
    assert tails == {POLICY_TAIL.get(family, ())}, f"{family}: load/store/order policies built: {sorted(tails)}"


def test_the_declared_counts():
    assert set(CELLS) == set(MANGLED) == set(REACH) == set(UNREACHABLE)
    assert {f: len(c) for f, c in CELLS.items()} == EXPECTED == PRODUCT
    assert sum(EXPECTED.values()) == 415
    for family, cells in CELLS.items():
        rows = {V16: enc.ROWS, GLDS: enc.GLDS_ROWS, LDSX: enc.LDSX_ROWS, KARG_LDSX: enc.KARG_LDSX_ROWS}
        assert {c[0] for c in cells} == set(rows.get(family, enc.ROWS)), family
    for family, groups in ((V16, enc.ENC_GROUPS), (KARG, enc.ENC_GROUPS), (VER_KARG, enc.VERIFY_GROUPS)):
        assert {c[1] for c in CELLS[family]} == set(groups), family
    assert {c[3] for c in CELLS[V16] if c[0] <= 2} == {128} and {c[3] for c in CELLS[V16] if c[0] > 2} == {256}


def test_the_name_patterns_read_template_arguments():
    """The parser itself, on names spelled the way the compiler spells them."""
    names = {"_ZN12_GLOBAL__N_113ec_encode_v16ILi3ENS_6EncPolILi6ELi2ELi2ELi2EEELi1ELi256EEEvPKmiiiPKjiijjyj",
             "_ZN12_GLOBAL__N_114ec_encode_gldsILi6ELi4ELi2EEEvPKmiiiPKjiijjyj",
             "_ZN12_GLOBAL__N_114ec_encode_ldsxILi5ELi2EEEvPKmiiiPKjS2_iijj",
             "_ZN12_GLOBAL__N_112ec_encode_b1ILi8EEEvPKmiiiPKjiijj",
             "_ZN12_GLOBAL__N_113ec_update_v16ILi6ELi128EEEvPKmiiiPKjijj",
             "_ZN12_GLOBAL__N_112ec_update_b1ILi4EEEvPKmiiiPKjijj",
             "_ZN12_GLOBAL__N_114ec_encode_kargILi7ENS_6EncPolILi8ELi2ELi3ELi2EEELi0EEEv13isal_hip_karg14isal_hip_kdoneiijyj",
             "_ZN12_GLOBAL__N_115ec_encode_karg4ILi5EEEv13isal_hip_karg14isal_hip_kdoneii",
             "_ZN12_GLOBAL__N_119ec_encode_karg_ldsxILi7EEEv13isal_hip_karg14isal_hip_kdonePKmiij",
             "_ZN12_GLOBAL__N_114ec_update_kargILi4EEEv13isal_hip_karg14isal_hip_kdoneij",
             "_ZN12_GLOBAL__N_114ec_verify_kargILi2ENS_6EncPolILi4ELi2ELi2ELi0EEELi1EEEv13isal_hip_karg14isal_hip_kdoneiijyj",
             "_ZN12_GLOBAL__N_112ec_verify_b1ILi7EEEvPKmiiiPKjiijjPyix",
             "_ZN12_GLOBAL__N_113ec_verify_v16ILi7ENS_6EncPolILi4ELi2ELi2ELi0EEELi1EEEvPKmiiiPKjiijjPyixyjS7_"}
    got = _built_cells(names)
    assert got == {V16: [((3, 6, 1, 256), (2, 2, 2))], GLDS: [((6, 4, 2), ())], LDSX: [((5, 2), ())],
                   B1: [((8,), ())], UPD_V16: [((6, 128), ())], UPD_B1: [((4,), ())],
                   KARG: [((7, 8, 0), (2, 3, 2))], KARG4: [((5,), ())], KARG_LDSX: [((7,), ())],
                   UPD_KARG: [((4,), ())], VER_KARG: [((2, 4, 1), (2, 2, 0))], VER_B1: [((7,), ())]}
    for family, cells in got.items():  # the neighbouring matrix's ec_verify_v16 is ignored here
        assert cells[0][0] in CELLS[family], family
    with pytest.raises(AssertionError, match="not understood"):  # a template argument more
        _built_cells({"_ZN12_GLOBAL__N_114ec_encode_ldsxILi5ELi2ELi1EEEvPKmiiiPKjS2_iijj"})
    with pytest.raises(AssertionError, match="not understood"):  # the policy spelled out of place
        _built_cells({"_ZN12_GLOBAL__N_114ec_encode_kargILi7ELi8ELi0EEEv13isal_hip_karg14isal_hip_kdoneiijyj"})


@pytest.mark.parametrize("family", sorted(MANGLED))
def test_every_cell_is_reached_or_declared_unreachable(family):
    """REACH covers CELLS - UNREACHABLE exactly, the restated dispatch leads
    from each entry to its cell, and no knob of an entry is idle."""
    assert UNREACHABLE[family] <= CELLS[family]
    assert set(REACH[family]) == CELLS[family] - UNREACHABLE[family]
    assert not set(REACH[family]) & UNREACHABLE[family]
    for cell, r in REACH[family].items():
        assert r.rows == cell[0] and r.form in (enc.GENERAL, enc.MIX) and r.align in (enc.ALIGNED, enc.BYTES), cell
        assert 1 <= r.k <= 64 and (r.form == enc.GENERAL or r.k >= 3), cell
        assert (r.align == enc.BYTES) == (family in (B1, UPD_B1, VER_B1)), cell
        if family in (V16, GLDS, LDSX):
            assert r.entry == "batch_encode" and enc.batch_kernels(r) == [(family, cell)], (cell, r)
            for knob in r.env:
                less = r._replace(env={n: v for n, v in r.env.items() if n != knob})
                assert enc.batch_kernels(less) != [(family, cell)], (cell, "idle knob", knob)
        elif family in (KARG, KARG4, KARG_LDSX):
            assert r.entry == "ec_encode_data" and enc.karg_kernel_of(r) == (family, cell), (cell, r)
            for knob in r.env:
                less = r._replace(env={n: v for n, v in r.env.items() if n != knob})
                assert enc.karg_kernel_of(less) != (family, cell), (cell, "idle knob", knob)
        elif family in (VER_KARG, VER_B1):
            assert r.entry == ("xor_check", "pq_check")[cell[0] - 1] and cell[0] in enc.RAID_ROWS, cell
            assert not r.env or (family == VER_KARG and cell[2] == enc.LUT and r.env == {"ISAL_HIP_ENC_XOR": "0"})
            if family == VER_KARG:
                assert enc.verify_group(r.k) == cell[1] == r.k, cell
        else:
            assert r.entry == {B1: "batch_encode", UPD_V16: "batch_update", UPD_B1: "batch_update",
                               UPD_KARG: "ec_encode_data_update"}[family] and not r.env, cell
        if r.entry in ("ec_encode_data", "xor_check", "pq_check") and r.align == enc.ALIGNED:
            assert enc.karg_fits(r.k, r.rows), cell  # else the call leaves the kernel-argument route
        if family in (V16, KARG) and "ISAL_HIP_ENC_GROUP" not in r.env:
            assert r.k == cell[1], cell  # k = U, the library's own rule


def test_the_unreachable_cells_are_the_ones_the_code_rules_out():
    """ec_encode_karg<8, 12, FL> is reached at k = 11 with the group forced
    (5 * 12 * 8 table words do not fit); the verify kernels of 3..8 rows have
    no caller (xor_check: 1 row, pq_check: 2)."""
    assert not enc.karg_fits(12, 8) and enc.karg_fits(11, 8)
    for FL in enc.KARG_FORMS:
        r = REACH[KARG][(8, 12, FL)]
        assert (r.k, r.env.get("ISAL_HIP_ENC_GROUP")) == (11, "12")
    assert [k for k in range(1, 33) if enc.enc_group(k, 0, {}) == 12 and enc.karg_fits(k, 8)] == []
    assert {f for f, c in UNREACHABLE.items() if c} == {VER_KARG, VER_B1}
    assert UNREACHABLE[VER_KARG] == {c for c in CELLS[VER_KARG] if c[0] >= 3} and len(UNREACHABLE[VER_KARG]) == 48
    assert UNREACHABLE[VER_B1] == {(P,) for P in range(3, 9)}


def test_remainder_and_extra_cells_are_consistent():
    """Every remainder k leaves a remainder of its group and is reached by the
    restated rule; the kernel-argument ones keep the two limits."""
    assert enc.REMAINDER_ROWS == (2, 4, 7)
    assert {U for _, _, U in enc.REMAINDER} == set(enc.ENC_GROUPS)
    for k, env, U in enc.REMAINDER:
        assert k % U and enc.enc_group(k, 0, env) == U
        for FL in enc.V16_FORMS:
            for P in enc.REMAINDER_ROWS:
                cell = (P, U, FL, enc.enc_block(P))
                assert cell in CELLS[V16] and enc.batch_kernels(enc.reach_v16(cell, k, env)) == [(V16, cell)], cell
        for FL in enc.KARG_FORMS:
            for P in enc.karg_remainder_rows(k):
                r = enc.reach_karg((P, U, FL), k, env)
                assert enc.karg_fits(r.k, r.rows) and enc.karg_kernel_of(r) == (KARG, (P, U, FL)), (k, P, FL)
    for k, env, U in enc.VERIFY_REMAINDER:
        assert k % U and enc.verify_group(k) == U and not env and enc.karg_fits(k, 2)
    for k in enc.GLDS_K:
        assert k % enc.GLDS_RING == 1  # a partial last round that is a single source
        for cell in CELLS[GLDS]:
            assert enc.batch_kernels(enc.reach_glds(cell, k)) == [(GLDS, cell)]
    assert 9 // enc.GLDS_RING == 2 and 13 // enc.GLDS_RING == 3
    for k in enc.LDSX_K:
        assert k % enc.LDSX_GROUP == 1
        for cell in CELLS[LDSX]:
            assert enc.batch_kernels(enc.reach_ldsx(cell, k)) == [(LDSX, cell)]
        for cell in CELLS[KARG_LDSX]:
            assert enc.karg_kernel_of(REACH[KARG_LDSX][cell]._replace(k=k)) == (KARG_LDSX, cell)
    for U in enc.ENC_GROUPS:  # the second pass: <8, U, FL, 256> then <3, U, 0, 256>
        first, second = enc.batch_kernels(enc.second_pass_reach(U))
        assert first[0] == second[0] == V16 and first[1][:2] == (8, U) and second[1] == (3, U, enc.LUT, 256)
        assert first[1] in CELLS[V16] and second[1] in CELLS[V16]
    assert {enc.second_pass_reach(U).form for U in enc.ENC_GROUPS} == {enc.GENERAL, enc.MIX}


def test_the_shapes_have_the_tiles_the_cells_are_about():
    for family, cells in CELLS.items():
        for cell in cells:
            n, T = enc.length_of(family, cell), enc.tile_of(family, cell)
            if family in (B1, UPD_B1, VER_B1):
                assert n == 2 * 256 + 37
            elif family == KARG4:
                assert n == 3 * 1024 + 7
            else:
                assert n == enc._uniform_len(T) and n // T == 2 and (n % T) // 16 == 3 and n % 16 == 7
                assert T == (2048 if family == UPD_V16 or (family == V16 and cell[0] <= 2) else 4096)
    assert enc.GUARD >= 64 and enc.GUARD % 16 == 0
    assert enc.name_of(V16, (4, 10, 1, 256)) == ["ec_encode_v16<4, EncPol<10, 2, 2, 2>, 1, 256>"]
    assert enc.name_of(KARG, (4, 10, 1)) == ["ec_encode_karg<4>", "ec_encode_karg<4, EncPol<10, 2, 3, 2>, 1>"]
    assert enc.name_of(UPD_V16, (6, 128)) == ["ec_update_v16<6, 128>"] and enc.name_of(B1, (3,)) == ["ec_encode_b1<3>"]
