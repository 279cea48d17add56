"""GPU tier: every (rows, load group) instantiation of the repair, ragged,
scrub and overwrite kernels, launched once and compared with the oracle.

Each of these kernels is compiled per pass width P (1..8) and per load group
U, and a few instantiations keep a written-out copy of the shared tile body
(ec_kernels.hip, `if constexpr ((P == 7 && Pol::U == 4) || ...)`): every one is
its own register allocation and its own wrapper code (item and pattern lookup,
bounds against the stripe's own length, dst0 offsets). CELLS declares, as plain
data, the template arguments of every instantiation; tests/
test_kernel_matrix_cpu.py holds CELLS equal to what the code object was built
with, and the tests below launch every cell of CELLS through the public
objects. So: built set == declared set == launched-and-checked set.

The checkers are those of the neighbouring GPU modules (their Stripes helpers,
imported): oracle.ec_encode_data per stripe, ecutil.decode_matrix for repairs,
never the engine's own output. Every shard is followed by at least 64 guard
bytes, outputs are pre-filled with a poison byte, and the whole allocation is
compared with the host image after the run.

A cell is reached through the library's own rule: the k that enc_group /
verify_group map to U (k = U), with no knob set. The one exception is U = 10
with P >= 6, where k = 10 loads in fives unless ISAL_HIP_ENC_WIDE5=0. The
remainder cells (ENC_REMAINDER, VERIFY_REMAINDER) add a k that leaves a remainder group, at
P = 2, 4 and 7: both tile sizes, and the written-out body where U = 4. The
verify and locate kernels take their group from verify_group, which does not
read ISAL_HIP_ENC_GROUP, so the k = 20 cell exists for the encode-like families
only; ec_overwrite_v16 has no load group over k, so it has no remainder cells.

The encode family itself is covered elsewhere: the batch encode and update
kernels (ec_encode_v16, ec_encode_glds, ec_encode_ldsx, ec_encode_b1,
ec_update_v16, ec_update_b1) and the drop-in kernels on device shards
(ec_encode_karg, ec_encode_karg4, ec_encode_karg_ldsx, ec_update_karg,
ec_verify_karg, ec_verify_b1) have their own matrix of the same build in
tests/test_encode_matrix_{cpu,gpu}.py, and the fused encode + checksum kernels
in tests/test_fused_crc_matrix_{cpu,gpu}.py.

Each cell proves which kernel ran: under ISAL_HIP_LOG=2 the library's
`isal_hip: kernel NAME<...>` lines must name exactly the cell's instantiation,
and kernel_launches() must grow by the expected count.

Shapes: T is the cell's tile (2 KiB for passes of 1-2 rows of the encode-like
families and always for the overwrite, 4 KiB otherwise). Uniform families run
3 stripes of 2T + 3*16 + 7 bytes (two full tiles, a partial tile of vector
lanes and a byte tail: 9 work items), ragged families the 7 lengths of
test_ragged_gpu.lens7(T) in a fixed shuffled order.
"""
import math
import random

import numpy as np
import pytest
import torch

import test_overwrite_gpu as ow_mod
import test_ragged_gpu as rag_mod
import test_repair_gpu as rep_mod
import test_repair_ragged_gpu as reprag_mod
import test_scrub_gpu as scrub_mod
import test_scrub_ragged_gpu as scrubrag_mod
from test_scrub_cpu import CLEAN as SCRUB_CLEAN

pytestmark = pytest.mark.gpu

# ---- the declared cells (plain data; importable without a GPU) ---------------

ROWS = tuple(range(1, 9))
LOCATE_ROWS = tuple(range(2, 9))  # a single row names no shard
ENC_GROUPS = (12, 10, 8, 6, 5, 4)  # enc_group's candidates
VERIFY_GROUPS = (10, 8, 6, 4)  # verify_group's candidates
FORMS = (0, 1)  # FL: kEncLUT (lookups), kEncXor (the 0/1 form)
OVERWRITE_BLOCK = 128
OVERWRITE_NW = (1, 2, 3)


def enc_block(P):
    """Lanes per workgroup of the encode-like families: 2 KiB tiles for
    passes of 1-2 rows, 4 KiB tiles otherwise."""
    return 128 if P <= 2 else 256


# family -> the template arguments of every instantiation, as the launch log
# prints them: (P, U, B), (P, U), (P, U, FL) or (P, COMMIT, B)
CELLS = {
    "ec_repair_v16": {(P, U, enc_block(P)) for P in ROWS for U in ENC_GROUPS},
    "ec_encode_rag": {(P, U, enc_block(P)) for P in ROWS for U in ENC_GROUPS},
    "ec_repair_rag": {(P, U, enc_block(P)) for P in ROWS for U in ENC_GROUPS},
    "ec_verify_rag": {(P, U) for P in ROWS for U in VERIFY_GROUPS},
    "ec_locate_rag": {(P, U) for P in LOCATE_ROWS for U in VERIFY_GROUPS},
    "ec_verify_v16": {(P, U, FL) for P in ROWS for U in VERIFY_GROUPS for FL in FORMS},
    "ec_locate_v16": {(P, U, FL) for P in LOCATE_ROWS for U in VERIFY_GROUPS for FL in FORMS},
    "ec_overwrite_v16": {(P, C, OVERWRITE_BLOCK) for P in ROWS for C in (0, 1)},
}

# The instantiations that keep encode_tile's body written out (ec_kernels.hip)
HAND_WRITTEN = {
    "ec_repair_v16": {(7, 4, 256), (3, 10, 256)},
    "ec_encode_rag": {(7, 4, 256), (4, 8, 256)},
    "ec_repair_rag": {(7, 4, 256), (4, 8, 256)},
}

# Remainder cells: (k, knobs, the U the library's rule gives)
REMAINDER_ROWS = (2, 4, 7)
ENC_REMAINDER = [(7, {}, 4),  # groups of 4, remainder 3
                 (13, {}, 4),  # remainder 1
                 (3, {}, 4),  # k < U: every source in the remainder loop
                 (20, {"ISAL_HIP_ENC_GROUP": "12"}, 12)]  # one full group, remainder 8
VERIFY_REMAINDER = ENC_REMAINDER[:3]  # verify_group does not read ISAL_HIP_ENC_GROUP

KNOBS = ("ISAL_HIP_ENC_WIDE5", "ISAL_HIP_ENC_GROUP", "ISAL_HIP_ENC_XOR")


def enc_knobs(P, U):
    """k = U reaches U by enc_group's own rule, but k = 10 loads in fives from
    6 rows on unless ISAL_HIP_ENC_WIDE5=0."""
    return {"ISAL_HIP_ENC_WIDE5": "0"} if U == 10 and P >= 6 else {}


def _column(family, U, extra=()):
    """The cells of `family` with load group U (and the given last arguments), by P."""
    return sorted(c for c in CELLS[family] if c[1] == U and c[2:] == tuple(extra))


# ---- running one cell ---------------------------------------------------------

@pytest.fixture(autouse=True)
def _reload_knobs_after(engine):
    """Knobs are read once by the library: every test leaves it re-synced with
    os.environ."""
    yield
    engine.reload_config()


def _knobs(engine, monkeypatch, env):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("ISAL_HIP_LOG", "2")
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    engine.reload_config()


def _name(family, cell):
    return f"{family}<{', '.join(str(x) for x in cell)}>"


class Launches:
    """What one step of a cell launched: the kernel lines of the log and the
    growth of kernel_launches() must both say `count` launches of `name`.
    `name` may also be the list of the step's kernel lines, in order, where
    they differ (passes of different widths, test_encode_matrix_gpu.py)."""

    def __init__(self, engine, capfd, name):
        self.engine, self.capfd, self.name = engine, capfd, name

    def __call__(self, step, count=1):
        torch.cuda.synchronize()
        self.capfd.readouterr()
        before = self.engine.kernel_launches()
        out = step()
        torch.cuda.synchronize()
        grew = self.engine.kernel_launches() - before
        err = self.capfd.readouterr().err
        named = [line.split("kernel ", 1)[1] for line in err.splitlines() if line.startswith("isal_hip: kernel ")]
        want = [self.name] * count if isinstance(self.name, str) else list(self.name)
        assert named == want, (self.name, named)
        assert grew == count, (self.name, grew)
        return out


def _uniform_len(T):
    return 2 * T + 3 * 16 + 7


def _ragged_lens(T, seed=1):
    return rag_mod.shuffled(rag_mod.lens7(T), seed)


def _patterns(m, count, n, seed):
    """n erasure patterns of `count` of m shards: distinct ones, taken in turn
    again where fewer than n exist."""
    rng, out = random.Random(seed), []
    while len(out) < min(n, math.comb(m, count)):
        p = tuple(sorted(rng.sample(range(m), count)))
        if p not in out:
            out.append(p)
    return [out[i % len(out)] for i in range(n)]


def _cauchy(oracle, k, m):
    return oracle.gf_gen_cauchy1_matrix(m, k)


# ---- the encode-like families: ec_repair_v16, ec_encode_rag, ec_repair_rag ----

def _repair_cell(engine, oracle, gpu, capfd, k, cell):
    """3 stripes, each with its own pattern of P of k + P + 1 shards."""
    P, _, B = cell
    m, n = k + P + 1, _uniform_len(B * 16)
    a = _cauchy(oracle, k, m)
    pats = _patterns(m, P, 3, 1000 * k + P)
    st = rep_mod.Stripes(oracle, gpu, a, k, m, n, pats, 500 + 10 * k + P)
    assert st.S == 3 and st.S * ((n + B * 16 - 1) // (B * 16)) == 9
    r = engine.Repair(n, k, m, a, P, st.S, st.errs(k + P), st.shards)
    try:
        assert r.npatterns() == 3
        Launches(engine, capfd, _name("ec_repair_v16", cell))(lambda: r.run(0))
        st.check(_name("ec_repair_v16", cell))
    finally:
        r.close()


def _encode_rag_cell(engine, oracle, gpu, capfd, k, cell):
    P, _, B = cell
    lens = _ragged_lens(B * 16)
    st = rag_mod.Stripes(gpu, "cauchy", k, P, lens, 600 + 10 * k + P)
    rg = engine.Ragged(k, P, st.tbls, lens, st.data, st.coding)
    try:
        Launches(engine, capfd, _name("ec_encode_rag", cell))(lambda: rg.encode(0))
        st.same(_name("ec_encode_rag", cell), st.want)
    finally:
        rg.close()


def _repair_rag_cell(engine, oracle, gpu, capfd, k, cell):
    """One class of count P: 7 stripes of 7 lengths, each with its own pattern."""
    P, _, B = cell
    m = k + P + 1
    a = _cauchy(oracle, k, m)
    lens = _ragged_lens(B * 16)
    pats = _patterns(m, P, len(lens), 2000 * k + P)
    st = reprag_mod.RaggedStripes(oracle, gpu, a, k, m, lens, pats, 700 + 10 * k + P)
    assert st.launches(engine) == 1
    r = engine.Repair.ragged(k, m, a, st.lens, st.errs(k + P), st.shards)
    try:
        Launches(engine, capfd, _name("ec_repair_rag", cell))(lambda: r.run(0))
        st.check(_name("ec_repair_rag", cell))
    finally:
        r.close()


ENC_FAMILIES = {"ec_repair_v16": _repair_cell, "ec_encode_rag": _encode_rag_cell, "ec_repair_rag": _repair_rag_cell}


@pytest.mark.parametrize("U", ENC_GROUPS)
@pytest.mark.parametrize("family", sorted(ENC_FAMILIES))
def test_encode_like_family_every_rows_of_a_load_group(engine, oracle, gpu, monkeypatch, capfd, family, U):
    cells = [c for c in sorted(CELLS[family]) if c[1] == U]
    assert [c[0] for c in cells] == list(ROWS)
    for cell in cells:
        _knobs(engine, monkeypatch, enc_knobs(cell[0], U))
        ENC_FAMILIES[family](engine, oracle, gpu, capfd, U, cell)


@pytest.mark.parametrize("k,env,U", ENC_REMAINDER)
@pytest.mark.parametrize("family", sorted(ENC_FAMILIES))
def test_encode_like_family_remainder_groups(engine, oracle, gpu, monkeypatch, capfd, family, k, env, U):
    assert k % U
    for P in REMAINDER_ROWS:
        cell = (P, U, enc_block(P))
        assert cell in CELLS[family]
        _knobs(engine, monkeypatch, env)
        ENC_FAMILIES[family](engine, oracle, gpu, capfd, k, cell)


# ---- verify and locate ---------------------------------------------------------

def _flips(k, P, T, long_, second, parity):
    """(stripe, shard, column): the last byte of the byte tail of the longest
    stripe in the last data shard, the first byte of a second tile in data
    shard 0, a byte of the last parity row."""
    n = _uniform_len(T)
    return [(long_, k - 1, n - 1), (second, 0, T), (parity, k + P - 1, T + 16 * 3 + 2)]


def _verify_cell(engine, oracle, gpu, capfd, name, kind, k, P, lens, make, stripes):
    """Clean, then one flipped byte in three places in turn: the words are the
    model's (column << 8 | row), nothing is written to the shards."""
    T = 4096
    st = rag_mod.Stripes(gpu, kind, k, P, lens, 800 + 10 * k + P, encoded=True)
    run = Launches(engine, capfd, name)
    obj = make(st)
    try:
        assert run(lambda: rag_mod._check(engine, st, obj)) == [rag_mod.CLEAN] * st.S
        for s, shard, col in _flips(k, P, T, *stripes):
            assert st.lens[s] == _uniform_len(T)
            st.flip(s, shard, col)
            want = st.model_bad(oracle)
            assert [x for x in range(st.S) if want[x] != rag_mod.CLEAN] == [s], (s, shard, col, want)
            assert run(lambda: rag_mod._check(engine, st, obj)) == want, (name, s, shard, col)
            st.restore()
    finally:
        obj.close()


def _verify_rag_cell(engine, oracle, gpu, capfd, k, cell):
    P, _ = cell
    lens = _ragged_lens(4096)
    long_ = lens.index(_uniform_len(4096))
    _verify_cell(engine, oracle, gpu, capfd, _name("ec_verify_rag", cell), "cauchy", k, P, lens,
                 lambda st: engine.Ragged(k, P, st.tbls, lens, st.data, st.coding), (long_, long_, long_))


def _verify_v16_cell(engine, oracle, gpu, capfd, k, cell):
    """isal_hip_batch_check over 3 stripes; the Reed-Solomon matrix has an all-
    ones row 0 and column 0, so ISAL_HIP_ENC_XOR alone chooses the form."""
    P, _, _ = cell
    n = _uniform_len(4096)
    _verify_cell(engine, oracle, gpu, capfd, _name("ec_verify_v16", cell), "rs", k, P, [n] * 3,
                 lambda st: engine.Batch(n, k, P, st.tbls, st.S, st.data, st.coding), (1, 0, 2))


def _locate_cell(engine, oracle, gpu, capfd, name, st, sc, mod, k, P, stripes):
    """Clean, then one flipped byte in three places in turn: the verdict names
    the flipped shard (and is the model's), nothing is written to the shards."""
    T = 4096
    assert engine.scrub_ambiguity(k, P, st.tbls) is None, (name, "the scrub refuses this matrix")
    run = Launches(engine, capfd, name)
    try:
        assert run(lambda: mod._run(engine, st, sc)) == [SCRUB_CLEAN] * st.S
        for s, shard, col in _flips(k, P, T, *stripes):
            st.flip(s, shard, col)
            expect = [SCRUB_CLEAN] * st.S
            expect[s] = shard
            assert st.want() == expect, ("the model disagrees with the case", s, shard, col)
            assert run(lambda: mod._run(engine, st, sc)) == expect, (name, s, shard, col)
            st.restore()
    finally:
        sc.close()


def _locate_rag_cell(engine, oracle, gpu, capfd, k, cell):
    P, _ = cell
    lens = _ragged_lens(4096)
    long_ = lens.index(_uniform_len(4096))
    st = scrubrag_mod.Stripes(oracle, gpu, "cauchy", k, P, lens, 900 + 10 * k + P)
    sc = engine.Scrub.ragged(k, P, st.tbls, lens, st.data, st.coding)
    _locate_cell(engine, oracle, gpu, capfd, _name("ec_locate_rag", cell), st, sc, scrubrag_mod, k, P,
                 (long_, long_, long_))


def _locate_v16_cell(engine, oracle, gpu, capfd, k, cell):
    P, _, _ = cell
    n = _uniform_len(4096)
    st = scrub_mod.Stripes(oracle, gpu, "rs", k, P, n, 3, 950 + 10 * k + P)
    sc = engine.Scrub(n, k, P, st.tbls, st.S, st.data, st.coding)
    _locate_cell(engine, oracle, gpu, capfd, _name("ec_locate_v16", cell), st, sc, scrub_mod, k, P, (1, 0, 2))


RAG_CHECKS = {"ec_verify_rag": _verify_rag_cell, "ec_locate_rag": _locate_rag_cell}
V16_CHECKS = {"ec_verify_v16": _verify_v16_cell, "ec_locate_v16": _locate_v16_cell}


def _rows_of(family):
    return sorted({c[0] for c in CELLS[family]})


@pytest.mark.parametrize("U", VERIFY_GROUPS)
@pytest.mark.parametrize("family", sorted(RAG_CHECKS))
def test_ragged_check_family_every_rows_of_a_load_group(engine, oracle, gpu, monkeypatch, capfd, family, U):
    cells = _column(family, U)
    assert [c[0] for c in cells] == _rows_of(family)
    _knobs(engine, monkeypatch, {})
    for cell in cells:
        RAG_CHECKS[family](engine, oracle, gpu, capfd, U, cell)


@pytest.mark.parametrize("k,env,U", VERIFY_REMAINDER)
@pytest.mark.parametrize("family", sorted(RAG_CHECKS))
def test_ragged_check_family_remainder_groups(engine, oracle, gpu, monkeypatch, capfd, family, k, env, U):
    assert k % U
    _knobs(engine, monkeypatch, env)
    for P in REMAINDER_ROWS:
        assert (P, U) in CELLS[family]
        RAG_CHECKS[family](engine, oracle, gpu, capfd, k, (P, U))


@pytest.mark.parametrize("FL", FORMS)
@pytest.mark.parametrize("U", VERIFY_GROUPS)
@pytest.mark.parametrize("family", sorted(V16_CHECKS))
def test_batch_check_family_every_rows_of_a_load_group(engine, oracle, gpu, monkeypatch, capfd, family, U, FL):
    cells = _column(family, U, (FL,))
    assert [c[0] for c in cells] == _rows_of(family)
    _knobs(engine, monkeypatch, {"ISAL_HIP_ENC_XOR": str(FL)})
    for cell in cells:
        V16_CHECKS[family](engine, oracle, gpu, capfd, U, cell)


@pytest.mark.parametrize("FL", FORMS)
@pytest.mark.parametrize("k,env,U", VERIFY_REMAINDER)
@pytest.mark.parametrize("family", sorted(V16_CHECKS))
def test_batch_check_family_remainder_groups(engine, oracle, gpu, monkeypatch, capfd, family, k, env, U, FL):
    assert k % U
    _knobs(engine, monkeypatch, {**env, "ISAL_HIP_ENC_XOR": str(FL)})
    for P in REMAINDER_ROWS:
        assert (P, U, FL) in CELLS[family]
        V16_CHECKS[family](engine, oracle, gpu, capfd, k, (P, U, FL))


# ---- ec_overwrite_v16 -----------------------------------------------------------

@pytest.mark.parametrize("nw", OVERWRITE_NW)
@pytest.mark.parametrize("commit", [0, 1])
def test_overwrite_every_rows(engine, oracle, gpu, monkeypatch, capfd, commit, nw):
    """Parity == a fresh oracle encode of the new data; with COMMIT old == new
    afterwards, without it a second run restores the parity."""
    k, T = 6, OVERWRITE_BLOCK * 16
    cells = sorted(c for c in CELLS["ec_overwrite_v16"] if c[1] == commit)
    assert [c[0] for c in cells] == list(ROWS)
    _knobs(engine, monkeypatch, {})
    for cell in cells:
        P = cell[0]
        name = _name("ec_overwrite_v16", cell)
        sets = ow_mod._seeded_sets(k, nw, 3, 100 * P + 10 * nw + commit)
        w = ow_mod.Writes(oracle, gpu, "cauchy", k, P, _uniform_len(T), sets, 40 + P)
        run = Launches(engine, capfd, name)
        ow = w.overwrite(engine)
        try:
            run(lambda: ow.run(commit=bool(commit)))
            if commit:
                got = w.check(w.committed, name)
                for r in range(w.S * nw):  # old == new
                    s, i = divmod(r, nw)
                    assert np.array_equal(got[s * w.m + sets[s][i]], got[w.new0 + r]), (name, s, i)
            else:
                w.check(w.parity_only, name)
                run(lambda: ow.run(commit=False))
                w.check(w.before, name + " second run")
        finally:
            ow.close()
