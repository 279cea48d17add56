"""GPU tier: every instantiation of the encode, update and drop-in kernels,
launched once and compared with the oracle.

The kernels behind isal_hip_batch_encode, isal_hip_batch_update and the drop-in
ec_encode_data, ec_encode_data_update, xor_check and pq_check on device shards
are compiled per pass width P (1..8) and, the vector forms, per load group U
and coefficient form FL (ec_kernels.hip). Every instantiation is its own
register allocation and schedule. CELLS declares, as plain data, the template
arguments of every one, spelled as the launch log prints them (ISAL_HIP_LOG=2):

    ec_encode_v16<P, EncPol<U, 2, 2, 2>, FL, B>   192 = 8 P x 6 U x 4 FL
    ec_encode_glds<P, 4, FL>                        8 = P 5..8 x {Lds, Xor|Lds}
    ec_encode_ldsx<P, 2>                            5 = P 4..8
    ec_encode_b1<P>, ec_update_v16<P, 128>, ec_update_b1<P>         8 each
    ec_encode_karg<P, EncPol<U, 2, 3, 2>, FL>      96 = 8 P x 6 U x {LUT, Xor}
    ec_encode_karg4<P>, ec_update_karg<P>           8 each
    ec_encode_karg_ldsx<P>                          2 = P 7, 8
    ec_verify_karg<P, U, FL>                       64 = 8 P x 4 U x {LUT, Xor}
    ec_verify_b1<P>                                 8

tests/test_encode_matrix_cpu.py holds CELLS equal to what ec_kernels.o was
built with; the tests below launch every cell of CELLS minus UNREACHABLE. So:
built set == declared set == launched-and-checked set, and a cell is launched
or listed with the code's reason, nothing else.

Reaching a cell (REACH: cell -> Reach(entry, k, rows, form, align, env)). The
library's own rule is used wherever one leads to the cell: k = U (enc_group,
verify_group), B follows P, and the Xor forms take a coefficient matrix whose
row 0 and column 0 are a 0/1 mix (test_gpu_parity._coef_01 "mask", with a one
and a zero planted in each), the LUT forms one with no 0/1 entry. A knob is
set only where the rule does not lead to the cell (kernel_of / karg_kernel_of
restate the rule; the CPU tier checks each knob is needed, the launch log here
decides):
  * ISAL_HIP_ENC_GLDS=0 for ec_encode_v16 at P >= 5: those passes stage their
    sources through the LDS-DMA ring (enc_glds);
  * ISAL_HIP_ENC_LDSX=0 for ec_encode_v16, ec_encode_glds and ec_encode_karg
    at P >= 7: those passes take the LDS product tables (enc_ldsx,
    isal_hip_karg_ldsx); ISAL_HIP_ENC_LDSX=1 for ec_encode_ldsx<4..6, 2>, which
    the rule picks from k = 16 (P >= 5) or never (P = 4);
  * ISAL_HIP_ENC_LDS=1 or =0 for the Lds forms enc_lds does not pick (it picks
    Lds when more than 4 rows are looked up and P <= 6, or U = 5 at P >= 7);
  * ISAL_HIP_ENC_WIDE5=0 for U = 10 at P >= 6 (k = 10 loads in fives there);
  * ISAL_HIP_ENC_GROUP=12 at k = 11 for ec_encode_karg<8, 12, FL>: the
    kernel-argument block holds 5 * k * rows <= 448 table words, so no k = 12
    at 8 rows; every source then goes through the remainder loop;
  * ISAL_HIP_KARG_NARROW=1 for ec_encode_karg4 (the rule picks it under 12
    calls in flight);
  * ISAL_HIP_ENC_XOR=0 for the LUT forms of ec_verify_karg: xor_check and
    pq_check build their own coefficients, which are all 0/1 in row 0 and
    column 0.

UNREACHABLE: the verify kernels of 3..8 rows. The only callers of the drop-in
verify are xor_check (one parity row) and pq_check (two), isal_hip_raid.c
raid_run; isal_hip_run is not exported.

Shapes. The 16-byte-lane families run 3 stripes (the drop-in calls one) of
_uniform_len(T) = 2T + 3 * 16 + 7 bytes, T the cell's tile: two full tiles, a
partial tile of vector lanes and a byte tail. T = 2 KiB for P <= 2 of
ec_encode_v16 and for ec_update_v16, 4 KiB otherwise. The byte-lane kernels
(*_b1) run shards that start 1..15 bytes past a 16-byte boundary, each at
another offset, of two 256-byte tiles plus 37 bytes. ec_encode_karg4 runs
three 1 KiB blocks plus 7 bytes. Remainder cells (ENC_REMAINDER of the
neighbouring matrix, and k = U + 3 with the group forced for the other U) run
at P = 2, 4 and 7 of every FL; ec_encode_glds adds k = 9 (a partial last ring
round) and k = 13 (a single last source), ec_encode_ldsx and
ec_encode_karg_ldsx k = 9 (odd) and k = 1 (below the load pair). A second pass
runs at rows = 8 + 3: one batch encode per load group, and a batch update at
vec_i = 0, a middle source and k - 1 (the table offset vec_i * P * kTbl is
taken per pass, and the passes differ in P).

Layout and reference: one pool per cell, every shard followed by at least 64
guard bytes with 64 more in front of the first; parity (old parity of an
update: seeded bytes) and guards are pre-filled, and after the run the *whole
pool* is compared with a host image of the sources, the oracle's parity
(oracle.encode; an update: old parity XOR the oracle's encode of that one
source) and untouched poison. Equality is exact. The verify cells run on a
clean stripe and on one with a flipped byte in the byte tail of the last
parity row; both results equal oracle.raid's, and the pool is unchanged.

Proof of which kernel ran (Launches of test_kernel_matrix_gpu): the step's
`isal_hip: kernel` lines are exactly the cell's, in order, and
kernel_launches() grows by the passes. A drop-in ec_encode_karg launch prints
two lines, `ec_encode_karg<P>` and the instantiation's.
"""
import collections

import numpy as np
import pytest
import torch

from ecutil import fill_bytes
from test_gpu_parity import _coef_01, _raid_fn, _vp
from test_kernel_matrix_gpu import (ENC_GROUPS, ENC_REMAINDER, REMAINDER_ROWS, ROWS, VERIFY_GROUPS, VERIFY_REMAINDER,
                                    Launches, _knobs, _reload_knobs_after, _uniform_len, enc_block)  # noqa: F401

pytestmark = pytest.mark.gpu

# ---- the declared cells (plain data; importable without a GPU) ---------------

# FL as the log prints it
LUT = 0  # ec_device.h: enum : int { kEncLUT = 0, ... }: every product looked up
XOR = 1  # ec_device.h: kEncXor = 1: row 0 and column 0 are XORs
LDS = 2  # ec_device.h: kEncLds = 2 (a bit, with either): low table halves from LDS
XOR_LDS = XOR | LDS  # 3
V16_FORMS = (LUT, XOR, LDS, XOR_LDS)
KARG_FORMS = (LUT, XOR)

V16, GLDS, LDSX, B1 = "ec_encode_v16", "ec_encode_glds", "ec_encode_ldsx", "ec_encode_b1"
UPD_V16, UPD_B1 = "ec_update_v16", "ec_update_b1"
KARG, KARG4, KARG_LDSX, UPD_KARG = "ec_encode_karg", "ec_encode_karg4", "ec_encode_karg_ldsx", "ec_update_karg"
VER_KARG, VER_B1 = "ec_verify_karg", "ec_verify_b1"

GLDS_ROWS = (5, 6, 7, 8)  # launch_glds_r: P >= 5
GLDS_RING = 4  # kGldsRing
LDSX_ROWS = (4, 5, 6, 7, 8)  # kLdsxRows = 4
LDSX_GROUP = 2  # kLdsxGroup
KARG_LDSX_ROWS = (7, 8)  # isal_hip_launch_encode_karg's switch
UPD_BLOCK = 128  # kUpdBlock

# family -> the template arguments of every instantiation, as the log prints them
CELLS = {
    V16: {(P, U, FL, enc_block(P)) for P in ROWS for U in ENC_GROUPS for FL in V16_FORMS},
    GLDS: {(P, GLDS_RING, FL) for P in GLDS_ROWS for FL in (LDS, XOR_LDS)},
    LDSX: {(P, LDSX_GROUP) for P in LDSX_ROWS},
    B1: {(P,) for P in ROWS},
    UPD_V16: {(P, UPD_BLOCK) for P in ROWS},
    UPD_B1: {(P,) for P in ROWS},
    KARG: {(P, U, FL) for P in ROWS for U in ENC_GROUPS for FL in KARG_FORMS},
    KARG4: {(P,) for P in ROWS},
    KARG_LDSX: {(P,) for P in KARG_LDSX_ROWS},
    UPD_KARG: {(P,) for P in ROWS},
    VER_KARG: {(P, U, FL) for P in ROWS for U in VERIFY_GROUPS for FL in KARG_FORMS},
    VER_B1: {(P,) for P in ROWS},
}

# Built cells no public call launches. isal_hip_raid.c raid_run is the only
# caller of the drop-in verify (OP_VERIFY), with rows = 1 (xor_check) and
# rows = 2 (pq_check); isal_hip_run is not exported (exports.map).
RAID_ROWS = (1, 2)
UNREACHABLE = {f: set() for f in CELLS}
UNREACHABLE[VER_KARG] = {c for c in CELLS[VER_KARG] if c[0] not in RAID_ROWS}
UNREACHABLE[VER_B1] = {c for c in CELLS[VER_B1] if c[0] not in RAID_ROWS}

GENERAL, MIX = "general", "mix"  # the coefficients: no 0/1 entry / row 0 and column 0 a 0/1 mix
ALIGNED, BYTES = "aligned", "bytes"  # shards on 16-byte boundaries / 1..15 bytes past one

# entry: batch_encode, batch_update, ec_encode_data, ec_encode_data_update, xor_check, pq_check
Reach = collections.namedtuple("Reach", "entry k rows form align env")

# the kernel-argument block (isal_hip_internal.h): pointers and table words
KARG_PTRS, KARG_TBL, TBL_DWORDS = 32, 448, 5


def karg_fits(k, rows):
    return k + rows <= KARG_PTRS and TBL_DWORDS * k * rows <= KARG_TBL


def name_of(family, cell):
    """The kernel lines one launch of the cell prints, in order."""
    if family == V16:
        return ["%s<%d, EncPol<%d, 2, 2, 2>, %d, %d>" % ((family,) + cell)]
    if family == KARG:  # kBufNT = 2 loads, kBufSC1NT = 3 stores
        return ["%s<%d>" % (family, cell[0]), "%s<%d, EncPol<%d, 2, 3, 2>, %d>" % ((family,) + cell)]
    return [f"{family}<{', '.join(str(x) for x in cell)}>"]


# ---- the library's rule, restated (ec_kernels.hip) ----------------------------

def enc_group(k, P, env):
    """enc_group / enc_wide5; P = 0 for the kernel-argument launch."""
    if int(env.get("ISAL_HIP_ENC_GROUP", 0)) in ENC_GROUPS:
        return int(env["ISAL_HIP_ENC_GROUP"])
    if P >= 6 and k >= 10 and k % 5 == 0 and env.get("ISAL_HIP_ENC_WIDE5") != "0":
        return 5
    return next((u for u in ENC_GROUPS if k >= u and k % u == 0), 4)


def verify_group(k):
    return next((u for u in VERIFY_GROUPS if k >= u and k % u == 0), 4)


def _forced(env, name, rule):
    return env[name] == "1" if env.get(name) in ("0", "1") else rule


def kernel_of(P, k, x, env, tables):
    """(family, cell) of one pass of a batch encode over aligned shards:
    encode_pass. x: the pass has its 0/1 form; tables: the batch holds the LDS
    product tables (k <= 64, rows >= 4)."""
    if tables and P >= LDSX_ROWS[0] and _forced(env, "ISAL_HIP_ENC_LDSX", P >= 7 or (P >= 5 and k >= 16)):
        return LDSX, (P, LDSX_GROUP)
    if P >= GLDS_ROWS[0] and env.get("ISAL_HIP_ENC_GLDS") != "0":
        return GLDS, (P, GLDS_RING, LDS | x)
    U = enc_group(k, P, env)
    lds = _forced(env, "ISAL_HIP_ENC_LDS",
                  P - x > 4 and (P <= 6 or (U == 5 and env.get("ISAL_HIP_ENC_WIDE5") != "0")))
    return V16, (P, U, (LDS if lds else LUT) | x, enc_block(P))


def has_form(k, form, env):
    """pass_mask: isal_hip_enc_masks finds the 0/1 form (k <= 64) and
    ISAL_HIP_ENC_XOR does not turn it off."""
    return int(form == MIX and k <= 64 and env.get("ISAL_HIP_ENC_XOR") != "0")


def batch_kernels(r):
    """[(family, cell)] of the passes of a batch encode; only pass 0 of the
    MIX coefficients has a 0/1 row."""
    out = []
    for r0 in range(0, r.rows, 8):
        x = has_form(r.k, r.form, r.env) if r0 == 0 else 0
        out.append(kernel_of(min(8, r.rows - r0), r.k, x, r.env, r.k <= 64 and r.rows >= 4))
    return out


def karg_kernel_of(r):
    """(family, cell) of a drop-in encode on aligned device shards, one call in
    flight: isal_hip_launch_encode_karg."""
    assert karg_fits(r.k, r.rows) and r.rows <= 8
    if _forced(r.env, "ISAL_HIP_KARG_NARROW", False):
        return KARG4, (r.rows,)
    if r.rows >= 7 and r.k <= 12 and r.env.get("ISAL_HIP_ENC_LDSX") != "0":
        return KARG_LDSX, (r.rows,)
    return KARG, (r.rows, enc_group(r.k, 0, r.env), has_form(r.k, r.form, r.env))


# ---- REACH ---------------------------------------------------------------------

def _form(FL):
    return MIX if FL & XOR else GENERAL


def reach_v16(cell, k=None, env=()):
    """k = U and the form's coefficients; then the knobs in front of the
    cell, each only where the rule goes elsewhere (module docstring)."""
    P, U, FL, _ = cell
    k, env = k or U, dict(env)
    if P >= 5:
        env["ISAL_HIP_ENC_GLDS"] = "0"  # else the LDS-DMA ring
    if P >= 7:
        env["ISAL_HIP_ENC_LDSX"] = "0"  # else the LDS product tables
    if U == 10 and P >= 6 and k % 5 == 0:
        env["ISAL_HIP_ENC_WIDE5"] = "0"  # else k = 10 loads in fives
    if kernel_of(P, k, FL & XOR, env, P >= 4)[1][2] != FL:
        env["ISAL_HIP_ENC_LDS"] = str(int(bool(FL & LDS)))  # the Lds form enc_lds does not pick
    return Reach("batch_encode", k, P, _form(FL), ALIGNED, env)


def reach_glds(cell, k=8):
    """k = 8: two full rounds of the ring of 4."""
    P, _, FL = cell
    return Reach("batch_encode", k, P, _form(FL), ALIGNED, {"ISAL_HIP_ENC_LDSX": "0"} if P >= 7 else {})


def reach_ldsx(cell, k=10):
    P, _ = cell
    return Reach("batch_encode", k, P, GENERAL, ALIGNED, {} if P >= 7 else {"ISAL_HIP_ENC_LDSX": "1"})


def reach_karg(cell, k=None, env=()):
    P, U, FL = cell
    k, env = k or U, dict(env)
    if not karg_fits(k, P):  # <8, 12, FL>: 5 * 12 * 8 = 480 table words
        k, env["ISAL_HIP_ENC_GROUP"] = U - 1, str(U)
    if P >= 7 and k <= 12:
        env["ISAL_HIP_ENC_LDSX"] = "0"  # else ec_encode_karg_ldsx
    return Reach("ec_encode_data", k, P, _form(FL), ALIGNED, env)


def reach_verify_karg(cell, k=None):
    P, U, FL = cell
    return Reach("xor_check" if P == 1 else "pq_check", k or U, P, MIX, ALIGNED,
                 {} if FL & XOR else {"ISAL_HIP_ENC_XOR": "0"})


K_PLAIN = 5  # the source count of the families with no load group over k
REACH = {
    V16: {c: reach_v16(c) for c in CELLS[V16]},
    GLDS: {c: reach_glds(c) for c in CELLS[GLDS]},
    LDSX: {c: reach_ldsx(c) for c in CELLS[LDSX]},
    B1: {c: Reach("batch_encode", K_PLAIN, c[0], GENERAL, BYTES, {}) for c in CELLS[B1]},
    UPD_V16: {c: Reach("batch_update", K_PLAIN, c[0], GENERAL, ALIGNED, {}) for c in CELLS[UPD_V16]},
    UPD_B1: {c: Reach("batch_update", K_PLAIN, c[0], GENERAL, BYTES, {}) for c in CELLS[UPD_B1]},
    KARG: {c: reach_karg(c) for c in CELLS[KARG]},
    KARG4: {c: Reach("ec_encode_data", K_PLAIN, c[0], GENERAL, ALIGNED, {"ISAL_HIP_KARG_NARROW": "1"})
            for c in CELLS[KARG4]},
    KARG_LDSX: {c: Reach("ec_encode_data", 10, c[0], GENERAL, ALIGNED, {}) for c in CELLS[KARG_LDSX]},
    UPD_KARG: {c: Reach("ec_encode_data_update", K_PLAIN, c[0], GENERAL, ALIGNED, {}) for c in CELLS[UPD_KARG]},
    VER_KARG: {c: reach_verify_karg(c) for c in CELLS[VER_KARG] - UNREACHABLE[VER_KARG]},
    VER_B1: {c: Reach("xor_check" if c[0] == 1 else "pq_check", K_PLAIN, c[0], MIX, BYTES, {})
             for c in CELLS[VER_B1] - UNREACHABLE[VER_B1]},
}

# Remainder cells: ENC_REMAINDER, and for the load groups it leaves out k = U + 3
# with the group forced: (k, knobs, U)
REMAINDER = ENC_REMAINDER + [(U + 3, {"ISAL_HIP_ENC_GROUP": str(U)}, U) for U in (10, 8, 6, 5)]
GLDS_K = (9, 13)  # a partial last ring round; a single last source
LDSX_K = (9, 1)  # odd; below the load pair
SECOND_PASS_ROWS = 8 + 3

GUARD = 64
POISON = 0xA5
B1_LEN = 2 * 256 + 37
KARG4_LEN = 3 * 1024 + 7


def tile_of(family, cell):
    if family == UPD_V16 or (family == V16 and cell[0] <= 2):
        return 2048
    return 4096


def length_of(family, cell):
    if family in (B1, UPD_B1, VER_B1):
        return B1_LEN
    return KARG4_LEN if family == KARG4 else _uniform_len(tile_of(family, cell))


def coefficients(k, rows, form, seed):
    """rows x k coefficient bytes: _coef_01's "mask" (row 0 and column 0 random
    0/1, with a one and a zero planted in each where there is room) or "big"
    (every byte >= 2)."""
    c = _coef_01(np.random.default_rng(seed), k, rows, "mask" if form == MIX else "big").reshape(rows, k).copy()
    if form == MIX:
        c[0, 0], c[0, k - 1], c[rows - 1, 0] = 1, 1, 1
        if k >= 3:
            c[0, 1] = 0
        if rows >= 3:
            c[1, 0] = 0
        assert c[0].max() <= 1 and c[:, 0].max() <= 1
    else:
        assert c.min() >= 2
    return c.reshape(-1)


# ---- running one cell ---------------------------------------------------------

MORE_KNOBS = ("ISAL_HIP_ENC_LDS", "ISAL_HIP_ENC_GLDS", "ISAL_HIP_ENC_LDSX", "ISAL_HIP_KARG_NARROW", "ISAL_HIP_KARG",
              "ISAL_HIP_KARG_DONE")


def _set_knobs(engine, monkeypatch, env):
    for name in MORE_KNOBS:
        monkeypatch.delenv(name, raising=False)
    _knobs(engine, monkeypatch, env)


class Pool:
    """S stripes of k + rows shards of n bytes in one device allocation. Shard
    i starts GUARD + i * slot + its offset (0, or 1..15 for BYTES, each shard
    another) into it; at least GUARD bytes follow every shard."""

    def __init__(self, gpu, S, k, rows, n, align, seed, old_parity=False):
        self.S, self.k, self.rows, self.n, self.nsh = S, k, rows, n, k + rows
        self.slot = (n + 15 + 15) // 16 * 16 + GUARD
        self.off = [0 if align == ALIGNED else 1 + (7 * i) % 15 for i in range(S * self.nsh)]
        self.image = np.full(GUARD + S * self.nsh * self.slot, POISON, np.uint8)
        for s in range(S):
            for i in range(self.nsh if old_parity else k):
                self.shard(s, i)[:] = fill_bytes(n, seed + 131 * s + i)
        self.dev = torch.from_numpy(self.image).to(gpu)
        self.base = int(self.dev.data_ptr())
        assert self.base % 16 == 0
        if align == BYTES:
            assert all(1 <= o <= 15 for o in self.off) and len(set(self.off[:self.nsh])) == min(15, self.nsh)

    def at(self, s, i):
        return GUARD + (s * self.nsh + i) * self.slot + self.off[s * self.nsh + i]

    def shard(self, s, i):
        return self.image[self.at(s, i):self.at(s, i) + self.n]

    def ptr(self, s, i):
        return self.base + self.at(s, i)

    def sources(self, s):
        return [self.shard(s, j).copy() for j in range(self.k)]

    def same(self, what):
        """The whole allocation == the host image."""
        got = self.dev.cpu().numpy()
        if not np.array_equal(got, self.image):
            at = int(np.flatnonzero(got != self.image)[0])
            slot, off = divmod(at - GUARD, self.slot) if at >= GUARD else (-1, at)
            where = "the guard in front of the pool" if slot < 0 else (
                f"stripe {slot // self.nsh} shard {slot % self.nsh} byte {off - self.off[slot]} of {self.n}")
            raise AssertionError((what, f"pool byte {at}: {where}: got {int(got[at]):#04x}, "
                                        f"want {int(self.image[at]):#04x}"))


def run_cell(engine, oracle, gpu, monkeypatch, capfd, family, cell, r, names=None, vec_i=None):
    """One call of r.entry: which kernels ran, then the whole pool."""
    n = length_of(family, cell)
    names = names or name_of(family, cell)
    what = f"{names[-1]} {r.entry} k={r.k} rows={r.rows} {r.form} {r.align} len={n} {r.env}"
    _set_knobs(engine, monkeypatch, r.env)
    update = r.entry in ("batch_update", "ec_encode_data_update")
    S = 3 if r.entry.startswith("batch") else 1
    k, rows = r.k, r.rows
    coef = coefficients(k, rows, r.form, 1000 * k + rows)
    tbls = engine.ec_init_tables(k, rows, coef)
    pool = Pool(gpu, S, k, rows, n, r.align, 7919 * k + rows, old_parity=update)
    passes = (rows + 7) // 8
    run = Launches(engine, capfd, names)
    if update:
        vec_i = k // 2 if vec_i is None else vec_i
        column = coef.reshape(rows, k)[:, vec_i].copy()
        for s in range(S):
            delta = oracle.encode(column, 1, rows, [pool.shard(s, vec_i).copy()])
            for l in range(rows):
                pool.shard(s, k + l)[:] ^= delta[l]
    else:
        for s in range(S):
            parity = oracle.encode(coef, k, rows, pool.sources(s))
            for l in range(rows):
                pool.shard(s, k + l)[:] = parity[l]
    if r.entry.startswith("batch"):
        b = engine.Batch(n, k, rows, tbls, S, [pool.ptr(s, j) for s in range(S) for j in range(k)],
                         [pool.ptr(s, k + l) for s in range(S) for l in range(rows)])
        try:
            run((lambda: b.update(vec_i, 0)) if update else (lambda: b.encode(0)), passes)
        finally:
            b.close()
    elif update:
        run(lambda: engine.ec_encode_data_update(n, k, rows, vec_i, tbls, pool.ptr(0, vec_i),
                                                 [pool.ptr(0, k + l) for l in range(rows)]), passes)
    else:
        run(lambda: engine.ec_encode_data(n, k, rows, tbls, [pool.ptr(0, j) for j in range(k)],
                                          [pool.ptr(0, k + l) for l in range(rows)]), passes)
    pool.same(what)


def raid_coefficients(oracle, k, rows):
    """isal_hip_raid.c raid_build: P all ones, Q = 2^j."""
    c = np.ones((rows, k), np.uint8)
    for j in range(1, k if rows == 2 else 0):
        c[1, j] = oracle.gf_mul(int(c[1, j - 1]), 2)
    return c.reshape(-1)


def run_check_cell(engine, oracle, gpu, monkeypatch, capfd, family, cell, r):
    """xor_check / pq_check on one clean stripe, then with one flipped byte in
    the byte tail of the last parity row: both == oracle.raid, nothing written."""
    n, k, rows = length_of(family, cell), r.k, r.rows
    names = name_of(family, cell)
    what = f"{names[0]} {r.entry} k={k} {r.align} len={n} {r.env}"
    _set_knobs(engine, monkeypatch, r.env)
    pool = Pool(gpu, 1, k, rows, n, r.align, 104729 * k + rows)
    parity = oracle.encode(raid_coefficients(oracle, k, rows), k, rows, pool.sources(0))
    for l in range(rows):
        pool.shard(0, k + l)[:] = parity[l]
    pool.dev.copy_(torch.from_numpy(pool.image))
    v = k + rows
    f, ptrs = _raid_fn(engine, r.entry), _vp([pool.ptr(0, i) for i in range(v)])
    run = Launches(engine, capfd, names)
    ref = [pool.shard(0, i).copy() for i in range(v)]
    assert oracle.raid(r.entry, v, n, ref) == 0, what
    assert run(lambda: f(v, n, ptrs)) == 0, what
    col = n - 2  # the byte tail of the ragged last tile
    assert col % 16 and col >= n // 16 * 16 and col // tile_of(family, cell) == n // tile_of(family, cell)
    pool.shard(0, v - 1)[col] ^= 0x40
    pool.dev.copy_(torch.from_numpy(pool.image))
    ref = [pool.shard(0, i).copy() for i in range(v)]
    want = oracle.raid(r.entry, v, n, ref)
    assert want != 0, what
    assert run(lambda: f(v, n, ptrs)) == want, (what, "flipped", col)
    pool.same(what)


def _run_column(engine, oracle, gpu, monkeypatch, capfd, family, cells, reach=None):
    assert cells and not set(cells) & UNREACHABLE[family]
    for cell in cells:
        r = reach(cell) if reach else REACH[family][cell]
        if family in (VER_KARG, VER_B1):
            run_check_cell(engine, oracle, gpu, monkeypatch, capfd, family, cell, r)
        else:
            run_cell(engine, oracle, gpu, monkeypatch, capfd, family, cell, r)


def _column(family, U=None, FL=None):
    """The cells of `family` with load group U and form FL (where it has them), by P."""
    fl = {V16: 2, GLDS: 2, KARG: 2, VER_KARG: 2}.get(family)
    return sorted(c for c in CELLS[family] - UNREACHABLE[family]
                  if (U is None or c[1] == U) and (FL is None or c[fl] == FL))


# ---- batch encode ---------------------------------------------------------------

@pytest.mark.parametrize("FL", V16_FORMS)
@pytest.mark.parametrize("U", ENC_GROUPS)
def test_encode_v16_every_rows_of_a_column(engine, oracle, gpu, monkeypatch, capfd, U, FL):
    cells = _column(V16, U, FL)
    assert [c[0] for c in cells] == list(ROWS)
    _run_column(engine, oracle, gpu, monkeypatch, capfd, V16, cells)


@pytest.mark.parametrize("FL", V16_FORMS)
@pytest.mark.parametrize("k,env,U", REMAINDER)
def test_encode_v16_remainder_groups(engine, oracle, gpu, monkeypatch, capfd, k, env, U, FL):
    assert k % U
    cells = [(P, U, FL, enc_block(P)) for P in REMAINDER_ROWS]
    assert set(cells) <= CELLS[V16]
    _run_column(engine, oracle, gpu, monkeypatch, capfd, V16, cells, lambda c: reach_v16(c, k, env))


def second_pass_reach(U):
    """rows = 8 + 3 at k = U, both passes through ec_encode_v16; the 0/1 mix
    for even U positions, so the first pass runs both of its forms."""
    form = MIX if ENC_GROUPS.index(U) % 2 == 0 else GENERAL
    first = reach_v16((8, U, XOR if form == MIX else LUT, 256))
    env = {n: v for n, v in first.env.items() if n != "ISAL_HIP_ENC_LDS"}
    return Reach("batch_encode", U, SECOND_PASS_ROWS, form, ALIGNED, env)


@pytest.mark.parametrize("U", ENC_GROUPS)
def test_encode_v16_second_pass(engine, oracle, gpu, monkeypatch, capfd, U):
    """The second pass writes rows 8.. (dst0 + r0) from its own tables (kTbl * k * r0)."""
    r = second_pass_reach(U)
    passes = batch_kernels(r)
    assert [f for f, _ in passes] == [V16, V16] and passes[1][1] == (3, U, LUT, 256), passes
    run_cell(engine, oracle, gpu, monkeypatch, capfd, *passes[1], r,
             names=[name_of(f, c)[0] for f, c in passes])


@pytest.mark.parametrize("k", (8,) + GLDS_K)
@pytest.mark.parametrize("FL", (LDS, XOR_LDS))
def test_encode_glds_every_rows(engine, oracle, gpu, monkeypatch, capfd, FL, k):
    cells = _column(GLDS, GLDS_RING, FL)
    assert [c[0] for c in cells] == list(GLDS_ROWS)
    _run_column(engine, oracle, gpu, monkeypatch, capfd, GLDS, cells, lambda c: reach_glds(c, k))


@pytest.mark.parametrize("k", (10,) + LDSX_K)
def test_encode_ldsx_every_rows(engine, oracle, gpu, monkeypatch, capfd, k):
    cells = _column(LDSX)
    assert [c[0] for c in cells] == list(LDSX_ROWS)
    _run_column(engine, oracle, gpu, monkeypatch, capfd, LDSX, cells, lambda c: reach_ldsx(c, k))


@pytest.mark.parametrize("family", [B1, UPD_V16, UPD_B1])
def test_byte_lane_encode_and_batch_update_every_rows(engine, oracle, gpu, monkeypatch, capfd, family):
    cells = _column(family)
    assert [c[0] for c in cells] == list(ROWS)
    _run_column(engine, oracle, gpu, monkeypatch, capfd, family, cells)


@pytest.mark.parametrize("vec_i", [0, K_PLAIN // 2, K_PLAIN - 1])
@pytest.mark.parametrize("family", [UPD_V16, UPD_B1])
def test_batch_update_second_pass(engine, oracle, gpu, monkeypatch, capfd, family, vec_i):
    """rows = 8 + 3: the table offset vec_i * P * kTbl is taken per pass."""
    tail = (UPD_BLOCK,) if family == UPD_V16 else ()
    r = REACH[family][(3,) + tail]._replace(rows=SECOND_PASS_ROWS)
    run_cell(engine, oracle, gpu, monkeypatch, capfd, family, (3,) + tail, r,
             names=name_of(family, (8,) + tail) + name_of(family, (3,) + tail), vec_i=vec_i)


# ---- the drop-in calls on device shards -----------------------------------------

@pytest.mark.parametrize("FL", KARG_FORMS)
@pytest.mark.parametrize("U", ENC_GROUPS)
def test_dropin_encode_karg_every_rows_of_a_column(engine, oracle, gpu, monkeypatch, capfd, U, FL):
    cells = _column(KARG, U, FL)
    assert [c[0] for c in cells] == list(ROWS)
    _run_column(engine, oracle, gpu, monkeypatch, capfd, KARG, cells)


def karg_remainder_rows(k):
    """REMAINDER_ROWS within the kernel-argument limits."""
    return [P for P in REMAINDER_ROWS if karg_fits(k, P)]


@pytest.mark.parametrize("FL", KARG_FORMS)
@pytest.mark.parametrize("k,env,U", [x for x in REMAINDER if len(karg_remainder_rows(x[0])) >= 2])
def test_dropin_encode_karg_remainder_groups(engine, oracle, gpu, monkeypatch, capfd, k, env, U, FL):
    assert k % U
    cells = [(P, U, FL) for P in karg_remainder_rows(k)]
    assert set(cells) <= CELLS[KARG]
    _run_column(engine, oracle, gpu, monkeypatch, capfd, KARG, cells, lambda c: reach_karg(c, k, env))


@pytest.mark.parametrize("family", [KARG4, UPD_KARG])
def test_dropin_narrow_encode_and_update_every_rows(engine, oracle, gpu, monkeypatch, capfd, family):
    cells = _column(family)
    assert [c[0] for c in cells] == list(ROWS)
    _run_column(engine, oracle, gpu, monkeypatch, capfd, family, cells)


@pytest.mark.parametrize("k", (10,) + LDSX_K)
def test_dropin_encode_karg_ldsx(engine, oracle, gpu, monkeypatch, capfd, k):
    cells = _column(KARG_LDSX)
    assert [c[0] for c in cells] == list(KARG_LDSX_ROWS)
    _run_column(engine, oracle, gpu, monkeypatch, capfd, KARG_LDSX, cells,
                lambda c: REACH[KARG_LDSX][c]._replace(k=k))


@pytest.mark.parametrize("FL", KARG_FORMS)
@pytest.mark.parametrize("U", VERIFY_GROUPS)
def test_dropin_check_karg_every_reachable_rows_of_a_column(engine, oracle, gpu, monkeypatch, capfd, U, FL):
    cells = _column(VER_KARG, U, FL)
    assert [c[0] for c in cells] == list(RAID_ROWS)
    _run_column(engine, oracle, gpu, monkeypatch, capfd, VER_KARG, cells)


@pytest.mark.parametrize("FL", KARG_FORMS)
@pytest.mark.parametrize("k,env,U", VERIFY_REMAINDER)
def test_dropin_check_karg_remainder_groups(engine, oracle, gpu, monkeypatch, capfd, k, env, U, FL):
    assert k % U and verify_group(k) == U and not env
    cells = [(P, U, FL) for P in RAID_ROWS]
    assert set(cells) <= CELLS[VER_KARG]
    _run_column(engine, oracle, gpu, monkeypatch, capfd, VER_KARG, cells, lambda c: reach_verify_karg(c, k))


def test_dropin_check_byte_lanes_every_reachable_rows(engine, oracle, gpu, monkeypatch, capfd):
    cells = _column(VER_B1)
    assert [c[0] for c in cells] == list(RAID_ROWS)
    _run_column(engine, oracle, gpu, monkeypatch, capfd, VER_B1, cells)
