"""GPU tier: T10 protection information per sector (include/isal_hip.h
isal_hip_*_sector_t10dif, isal_hip_*_dif_generate, isal_hip_*_dif_verify): the
16-bit guard of every 512 B .. 4 KiB sector of every shard as a word, as the
8-byte tuple with its tags, and compared on the device with stored tuples.

The checker is difutil's restatement of crc16_t10dif (anchored to the
reference by test_dif_cpu.py), never the engine's output. The layout is the
sector checksum tests': every stripe of a case in one device allocation with
guard bytes after every shard (test_ragged_gpu.Stripes), every output inside a
larger device array with sentinels on both sides, and after every call the
whole shard allocation, the sentinels and the launch count are compared.
Lengths are test_sector_crc_gpu's LENS(S) in its three orders.
"""
import ctypes
import functools
import random
import struct

import numpy as np
import pytest
import torch

import difutil
from difutil import APP, CLEAN, GUARD, REF
from test_ragged_gpu import Stripes
from test_sector_crc_gpu import PAD, T, _expect, _HostCase, _nwords, orders

pytestmark = pytest.mark.gpu

_rng = random.Random(1610)
SEED16 = _rng.getrandbits(16) | 1  # random, non-zero
APP_TAG = 0xA5C3
TORCH = {2: torch.int16, 4: torch.int32, 8: torch.int64}
NUMPY = {2: np.uint16, 4: np.uint32, 8: np.uint64}
SENTINEL = {2: 0x7E57, 4: 0x7E57C0DE, 8: 0x7E57C0DE7E57C0DE}
GARBAGE = {2: 0x5A5A, 4: 0x5A5A5A5A, 8: 0x5A5A5A5A5A5A5A5A}


class Out:
    """n elements of w bytes between PAD sentinel elements on each side
    (test_sector_crc_gpu.Words for any width; a tuple is one 8-byte element)."""

    def __init__(self, gpu, n, w):
        self.n, self.w = n, w
        self.dev = torch.empty(n + 2 * PAD, dtype=TORCH[w], device=gpu)
        self.buf = self.dev[PAD:PAD + n]
        self.garbage()

    def _signed(self, x):
        bits = 8 * self.w
        return x - (1 << bits) if x >> (bits - 1) else x

    def garbage(self):
        self.dev.fill_(self._signed(SENTINEL[self.w]))
        self.buf.fill_(self._signed(GARBAGE[self.w]))

    def write(self, values):
        """values: numpy of n elements of the width (or 8n bytes of tuples)."""
        self.buf.copy_(torch.from_numpy(np.ascontiguousarray(values).view(NUMPY[self.w]).view(f"i{self.w}").copy()))

    def read(self, what):
        got = self.dev.cpu().numpy().view(NUMPY[self.w])
        assert (got[:PAD] == SENTINEL[self.w]).all(), f"{what}: an element before the output written"
        assert (got[PAD + self.n:] == SENTINEL[self.w]).all(), f"{what}: an element after the output written"
        return got[PAD:PAD + self.n].copy()

    def read_bytes(self, what):
        return self.read(what).view(np.uint8)


def _run(engine, st, call, launches, what):
    """One call: the launch count and no shard byte written."""
    torch.cuda.synchronize()
    before = engine.kernel_launches()
    call()
    torch.cuda.synchronize()
    assert engine.kernel_launches() - before == launches, what
    st.same(what)


@functools.lru_cache(maxsize=None)
def _guards(k, rows, lens, seed, S, crcseed):
    """The checker's guard of every sector of the encoded case, in the sector
    layout; computed once per case."""
    st = _HostCase(k, rows, lens, seed)
    out = difutil.sector_guards(difutil.shards_of(st, st.want), S, crcseed)
    out.setflags(write=False)
    return out


def _ref0(st, S, wrap=True):
    """Random reference tags per shard; the first shard with two sectors gets
    one whose sector tags wrap past 2^32."""
    rng = np.random.default_rng(1611)
    ref0 = rng.integers(0, 1 << 32, st.S * st.m, dtype=np.uint64).astype(np.uint32)
    if wrap:
        row = next(r for r, ns in enumerate(difutil.sectors_per_shard(st, S)) if ns >= 2)
        ref0[row] = 0xFFFFFFFF
    return ref0


def _dev32(gpu, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).copy()).to(gpu)


# ---- guard words ------------------------------------------------------------------


@pytest.mark.parametrize("order", range(3))
@pytest.mark.parametrize("S,k,rows", [(512, 1, 1), (512, 3, 2), (512, 10, 4), (4096, 1, 1), (4096, 3, 2), (4096, 10, 4),
                                      (1024, 3, 2), (2048, 3, 2)])
def test_ragged_guard_words_match_the_checker_per_sector(engine, gpu, S, k, rows, order):
    """Every word equals crc16_t10dif of its sector's bytes, for seed 0 and a
    random non-zero seed; exactly one launch; sentinels and shards untouched."""
    lens = orders(S)[order]
    seed = 900 + order
    st = Stripes(gpu, "rs", k, rows, lens, seed, encoded=True)
    rg = engine.Ragged(k, rows, st.tbls, lens, st.data, st.coding)
    words = Out(gpu, _nwords(st, S), 2)
    try:
        for crcseed in (0, SEED16):
            what = f"sector {S} seed {crcseed:#x}"
            words.garbage()
            _run(engine, st, lambda: rg.sector_t10dif(S, crcseed, words.buf), 1, what)
            _expect(words.read(what), _guards(k, rows, tuple(lens), seed, S, crcseed), st, S, what)
    finally:
        rg.close()


@pytest.mark.parametrize("S", [512, 1024, 2048, 4096])
@pytest.mark.parametrize("which", range(4))
def test_uniform_guard_words_match_the_checker_and_the_ragged_object(engine, gpu, S, which):
    n = [S - 1, S, T + S + 5, 2 * T + 3 * 16 + 7][which]
    seed = 940 + which
    st = Stripes(gpu, "rs", 3, 2, [n, n, n], seed, encoded=True)
    bt = engine.Batch(n, st.k, st.rows, st.tbls, st.S, st.data, st.coding)
    rg = engine.Ragged(st.k, st.rows, st.tbls, st.lens, st.data, st.coding)
    words = Out(gpu, _nwords(st, S), 2)
    try:
        for crcseed in (0, SEED16):
            want = _guards(st.k, st.rows, tuple(st.lens), seed, S, crcseed)
            got = {}
            for name, obj in (("batch", bt), ("ragged", rg)):
                what = f"sector {S} len {n} seed {crcseed:#x} {name}"
                words.garbage()
                _run(engine, st, lambda: obj.sector_t10dif(S, crcseed, words.buf), 1, what)
                got[name] = words.read(what)
                _expect(got[name], want, st, S, what)
            assert np.array_equal(got["batch"], got["ragged"])
    finally:
        bt.close()
        rg.close()


# ---- generate ---------------------------------------------------------------------


def _case(engine, gpu, S, uniform=False, seed=905):
    lens = [T + S + 5] * 3 if uniform else orders(S)[2]
    st = Stripes(gpu, "rs", 3, 2, lens, seed, encoded=True)
    obj = (engine.Batch(lens[0], 3, 2, st.tbls, st.S, st.data, st.coding) if uniform else
           engine.Ragged(3, 2, st.tbls, lens, st.data, st.coding))
    return st, obj, _guards(3, 2, tuple(lens), seed, S, 0)


@pytest.mark.parametrize("uniform", [False, True], ids=["ragged", "uniform"])
@pytest.mark.parametrize("S", [512, 4096])
def test_generate_writes_the_tuples_byte_for_byte(engine, gpu, S, uniform):
    """struct.pack(">HHI") of the checker's guard, the application tag and the
    reference tag: type 1 with random ref0 (one shard's tags wrap past 2^32),
    type 3, and a NULL ref0 for both; one launch, nothing outside pi."""
    st, obj, _ = _case(engine, gpu, S, uniform)
    nsec = _nwords(st, S)
    pi = Out(gpu, nsec, 8)
    ref0 = _ref0(st, S)
    d_ref0 = _dev32(gpu, ref0)
    try:
        for type_, r0, crcseed in ((1, ref0, 0), (3, ref0, SEED16), (1, None, SEED16), (3, None, 0)):
            what = f"sector {S} type {type_} ref0 {'set' if r0 is not None else 'NULL'}"
            guards = _guards(3, 2, tuple(st.lens), 905, S, crcseed)
            refs = difutil.ref_tags(st, S, type_, r0)
            if type_ == 1 and r0 is not None:
                assert any(a > b for a, b in zip(refs, refs[1:]) if a == 0xFFFFFFFF), "no tag wraps"
            pi.garbage()
            _run(engine, st, lambda: obj.dif_generate(S, pi.buf, type=type_, app_tag=APP_TAG, seed=crcseed,
                                                      ref0=None if r0 is None else d_ref0), 1, what)
            got = pi.read_bytes(what)
            want = difutil.tuples(guards, APP_TAG, refs)
            if not np.array_equal(got, want):
                i = int(np.nonzero(got != want)[0][0]) // 8
                raise AssertionError(f"{what}: tuple {i}: got {bytes(got[8 * i:8 * i + 8]).hex()}, "
                                     f"want {bytes(want[8 * i:8 * i + 8]).hex()}")
    finally:
        obj.close()


# ---- verify -----------------------------------------------------------------------


class Pi:
    """A case with generated tuples on the device: stored (host copy of what pi
    holds), and verify() = one dif_verify against the model of difutil."""

    def __init__(self, engine, gpu, S, uniform, type_=1):
        self.engine, self.gpu, self.S, self.type = engine, gpu, S, type_
        self.st, self.obj, self.guards = _case(engine, gpu, S, uniform)
        st = self.st
        self.ref0 = _ref0(st, S)
        self.d_ref0 = _dev32(gpu, self.ref0)
        self.refs = difutil.ref_tags(st, S, type_, self.ref0)
        self.pi = Out(gpu, _nwords(st, S), 8)
        self.bad = Out(gpu, st.S * st.m, 4)
        self.obj.dif_generate(S, self.pi.buf, type=type_, app_tag=APP_TAG, ref0=self.d_ref0)
        self.stored = self.pi.read_bytes("generate")
        assert np.array_equal(self.stored, difutil.tuples(self.guards, APP_TAG, self.refs))
        self.first = np.concatenate([[0], np.cumsum(difutil.sectors_per_shard(st, S))])

    def sector(self, row, i):
        return int(self.first[row]) + i

    def store(self, row, i, guard=None, app=None, ref=None):
        """Overwrites fields of the stored tuple of sector i of shard `row`."""
        at = 8 * self.sector(row, i)
        g, a, r = struct.unpack(">HHI", bytes(self.stored[at:at + 8]))
        new = struct.pack(">HHI", g if guard is None else guard, a if app is None else app, r if ref is None else ref)
        self.stored[at:at + 8] = np.frombuffer(new, np.uint8)
        self.pi.write(self.stored)

    def current_guards(self):
        return difutil.sector_guards(difutil.shards_of(self.st, self.st.image), self.S, 0)

    def verify(self, what, flags=7):
        self.bad.garbage()
        _run(self.engine, self.st, lambda: self.obj.dif_verify(self.S, self.pi.buf, self.bad.buf, type=self.type, flags=flags,
                                                               app_tag=APP_TAG, ref0=self.d_ref0), 1, what)
        assert np.array_equal(self.pi.read_bytes(what), self.stored), f"{what}: verify wrote pi"
        got = self.bad.read(what)
        model = difutil.verify_words(self.st, self.S, self.current_guards(), APP_TAG, self.refs, self.stored, self.type, flags)
        assert np.array_equal(got, model), (what, [hex(x) for x in got], [hex(x) for x in model])
        return [int(x) for x in got]

    def close(self):
        self.obj.close()


def _rows_with(st, S, nsec):
    """Shards (rows of the pointer table) with at least nsec sectors."""
    return [r for r, ns in enumerate(difutil.sectors_per_shard(st, S)) if ns >= nsec]


@pytest.mark.parametrize("uniform", [False, True], ids=["ragged", "uniform"])
@pytest.mark.parametrize("S", [512, 4096])
def test_verify_names_the_first_failing_sector_and_its_kinds(engine, gpu, S, uniform):
    p = Pi(engine, gpu, S, uniform)
    st = p.st
    nsh = st.S * st.m
    try:
        assert p.verify("after generate") == [CLEAN] * nsh  # a fill plus one launch
        rows = _rows_with(st, S, 2)
        row = rows[len(rows) // 2]
        s, j = divmod(row, st.m)
        n = st.lens[s]
        last = -(-n // S) - 1
        # a flipped data byte in the shard's last (short) sector: GUARD, in that shard's word alone
        st.flip(s, j, n - 1)
        assert p.verify("flipped byte") == [CLEAN] * row + [(last << 3) | GUARD] + [CLEAN] * (nsh - row - 1)
        # ... and CLEAN with CHECK_GUARD cleared
        assert p.verify("flipped byte, guard not checked", flags=APP | REF) == [CLEAN] * nsh
        # a second bad sector before it: the first is named
        st.flip(s, j, 3)
        assert p.verify("two bad sectors")[row] == (0 << 3) | GUARD
        st.restore()
        assert p.verify("restored") == [CLEAN] * nsh
        # stored tags: application tag, reference tag, guard and reference tag in one sector
        other = rows[0] if rows[0] != row else rows[1]
        p.store(row, last, app=APP_TAG ^ 0x0100)
        p.store(other, 1, ref=p.refs[p.sector(other, 1)] ^ 0x00010000)
        got = p.verify("stored tags corrupted")
        assert got[row] == (last << 3) | APP and got[other] == (1 << 3) | REF
        assert sum(x != CLEAN for x in got) == 2
        assert p.verify("only the guard checked", flags=GUARD) == [CLEAN] * nsh
        p.store(other, 1, guard=int(p.guards[p.sector(other, 1)]) ^ 0x8000)
        assert p.verify("guard and reference tag")[other] == (1 << 3) | GUARD | REF
        assert (1 << 3) | GUARD | REF == 13 and GUARD | REF == 5
    finally:
        p.close()


@pytest.mark.parametrize("type_", [1, 3])
def test_the_escape_rule_of_both_types(engine, gpu, type_):
    """Type 1: a stored application tag of 0xFFFF leaves the sector unchecked.
    Type 3: only together with a reference tag of 0xFFFFFFFF; 0xFFFF with any
    other reference tag IS checked."""
    S = 512
    p = Pi(engine, gpu, S, False, type_)
    st = p.st
    nsh = st.S * st.m
    try:
        row = _rows_with(st, S, 3)[1]
        s, j = divmod(row, st.m)
        st.flip(s, j, S + 7)  # sector 1
        assert p.verify("flipped")[row] == (1 << 3) | GUARD
        p.store(row, 1, app=0xFFFF)
        got = p.verify("application tag 0xFFFF")
        if type_ == 1:
            assert got == [CLEAN] * nsh
        else:
            assert got[row] == (1 << 3) | GUARD | APP  # still checked: the reference tag is not all-ones
            assert p.verify("... tags not checked", flags=GUARD)[row] == (1 << 3) | GUARD
            p.store(row, 1, ref=0xFFFFFFFF)
            assert p.verify("application and reference tag all-ones") == [CLEAN] * nsh
        # the escape is per sector: a later bad sector of the shard is still named
        st.flip(s, j, 2 * S + 1)
        assert p.verify("a later sector")[row] == (2 << 3) | GUARD
    finally:
        p.close()


def test_more_work_items_than_resident_workgroups(engine, gpu):
    """32 stripes of 3+2 shards of 17 tiles are 2720 items for at most 2048
    resident workgroups, at 4096: workgroups take a second item and the LDS
    hand-off alternates its slots. Guard words, then a corrupt sector in the
    last tile of the last shard found by verify, on both object kinds."""
    S, n, seed, nstripes = 4096, 16 * T + 37, 970, 32
    st = Stripes(gpu, "rs", 3, 2, [n] * nstripes, seed, encoded=True)
    assert st.S * st.m * -(-n // T) > 2048
    bt = engine.Batch(n, st.k, st.rows, st.tbls, st.S, st.data, st.coding)
    rg = engine.Ragged(st.k, st.rows, st.tbls, st.lens, st.data, st.coding)
    nsh, ns = st.S * st.m, -(-n // S)
    words, pi, bad = Out(gpu, nsh * ns, 2), Out(gpu, nsh * ns, 8), Out(gpu, nsh, 4)
    want = _guards(st.k, st.rows, tuple(st.lens), seed, S, SEED16)
    try:
        for name, obj in (("batch", bt), ("ragged", rg)):
            words.garbage()
            _run(engine, st, lambda: obj.sector_t10dif(S, SEED16, words.buf), 1, name)
            _expect(words.read(name), want, st, S, name)
            pi.garbage()
            _run(engine, st, lambda: obj.dif_generate(S, pi.buf, app_tag=APP_TAG, seed=SEED16), 1, name)
            assert np.array_equal(pi.read_bytes(name), difutil.tuples(want, APP_TAG, difutil.ref_tags(st, S, 1, None)))
            st.flip(st.S - 1, st.m - 1, n - 3)  # the 37-byte sector of the last tile
            st.flip(7, 1, 16 * T - 1)  # the last byte of a whole sector
            bad.garbage()
            _run(engine, st, lambda: obj.dif_verify(S, pi.buf, bad.buf, app_tag=APP_TAG, seed=SEED16), 1, name)
            got = [int(x) for x in bad.read(name)]
            model = [CLEAN] * nsh
            model[nsh - 1] = ((ns - 1) << 3) | GUARD
            model[7 * st.m + 1] = (15 << 3) | GUARD
            assert got == model, name
            st.restore()
    finally:
        bt.close()
        rg.close()


# ---- end to end ---------------------------------------------------------------------


def test_encode_generate_corrupt_verify_repair_verify(engine, oracle, gpu):
    """rs 10+4 ragged: encode, generate; corrupt two shards of one stripe and
    one of another; verify names all three; the erasure lists built from bad
    alone go to isal_hip_repair_create_ragged; after the rebuild verify is
    clean again and every byte equals the original."""
    S, k, rows, seed = 512, 10, 4, 902
    lens = orders(S)[2]
    m = k + rows
    st = Stripes(gpu, "rs", k, rows, lens, seed)  # poisoned parity
    rg = engine.Ragged(k, rows, st.tbls, lens, st.data, st.coding)
    nsh = st.S * m
    pi, bad = Out(gpu, _nwords(st, S), 8), Out(gpu, nsh, 4)
    d_ref0 = _dev32(gpu, _ref0(st, S))
    kw = dict(type=1, app_tag=APP_TAG, ref0=d_ref0)
    rep = None
    try:
        rg.encode(0)
        rg.dif_generate(S, pi.buf, **kw)
        torch.cuda.synchronize()
        st.image = st.want.copy()
        st.same("encoded")
        big = [s for s, n in enumerate(lens) if n >= 2 * T]
        s0, s1 = big[0], big[1]
        hits = {(s0, 2): lens[s0] - 1, (s0, k + 1): T + 5, (s1, 0): 0}
        for (s, j), col in hits.items():
            st.flip(s, j, col)
        rg.dif_verify(S, pi.buf, bad.buf, **kw)
        torch.cuda.synchronize()
        got = [int(x) for x in bad.read("verify")]
        assert {divmod(r, m): w for r, w in enumerate(got) if w != CLEAN} == \
            {sj: ((col // S) << 3) | GUARD for sj, col in hits.items()}
        errs = [[j for j in range(m) if got[s * m + j] != CLEAN] for s in range(st.S)]
        assert sorted(len(e) for e in errs)[-2:] == [1, 2]
        shards = [(st.data[s * k + j] if j < k else st.coding[s * rows + j - k]) for s in range(st.S) for j in range(m)]
        rep = engine.Repair.ragged(k, m, oracle.gf_gen_rs_matrix(m, k), lens, errs, shards)
        rep.run(0)
        rg.dif_verify(S, pi.buf, bad.buf, **kw)
        torch.cuda.synchronize()
        assert (bad.read("verify after repair") == CLEAN).all()
        st.same("after repair", st.want)
    finally:
        rg.close()
        if rep is not None:
            rep.close()


# ---- refusals and ordering ------------------------------------------------------------


def test_refusals_on_live_objects(engine, gpu):
    """Behind a live object: a bad sector, a bad type, bad flags, a misaligned
    pi, NULL outputs, and on the uniform batch a shard 8 bytes off a 16-byte
    boundary; ISAL_HIP_EINVAL, nothing launched, nothing written."""
    k, rows, n, S = 3, 2, 1024, 3
    m = k + rows
    buf = torch.zeros(S * m * (n + 64) + 64, dtype=torch.uint8, device=gpu)
    base = int(buf.data_ptr())
    ptrs = [base + i * (n + 64) for i in range(S * m)]
    a = engine.gf_gen_rs_matrix(m, k)
    tbls = engine.ec_init_tables(k, rows, a[k * k:])

    def split(p):
        return ([p[s * m + j] for s in range(S) for j in range(k)], [p[s * m + k + l] for s in range(S) for l in range(rows)])

    good = engine.Batch(n, k, rows, tbls, S, *split(ptrs))
    rg = engine.Ragged(k, rows, tbls, [n] * S, *split(ptrs))
    off = list(ptrs)
    off[k + 1] += 8  # a source of stripe 1
    unaligned = engine.Batch(n, k, rows, tbls, S, *split(off))
    out = Out(gpu, 2 * S * m, 8)
    L = engine.lib()
    p = ctypes.c_void_p(int(out.buf.data_ptr()))
    odd = ctypes.c_void_p(int(out.buf.data_ptr()) + 4)
    try:
        torch.cuda.synchronize()
        before = engine.kernel_launches()
        d = engine._Dif(1, 7, 0, 0, None)
        for kind, h in (("batch", good._h), ("ragged", rg._h)):
            words, gen, ver = (getattr(L, f"isal_hip_{kind}_{f}") for f in ("sector_t10dif", "dif_generate", "dif_verify"))
            for sector in (0, 256, 768, 8192, -512):
                assert words(h, sector, 0, p, None) == -1
                assert gen(h, sector, ctypes.byref(d), p, None) == -1
                assert ver(h, sector, ctypes.byref(d), p, p, None) == -1
            for type_ in (0, 2, 4):
                t = engine._Dif(type_, 7, 0, 0, None)
                assert gen(h, 512, ctypes.byref(t), p, None) == -1 and ver(h, 512, ctypes.byref(t), p, p, None) == -1
            assert ver(h, 512, ctypes.byref(engine._Dif(1, 8, 0, 0, None)), p, p, None) == -1
            assert gen(h, 512, ctypes.byref(d), odd, None) == -1 and ver(h, 512, ctypes.byref(d), odd, p, None) == -1
            assert words(h, 512, 0, None, None) == -1 and gen(h, 512, None, p, None) == -1
            assert ver(h, 512, ctypes.byref(d), p, None, None) == -1
        assert L.isal_hip_batch_sector_t10dif(unaligned._h, 512, 0, p, None) == -1
        assert L.isal_hip_batch_dif_generate(unaligned._h, 512, ctypes.byref(d), p, None) == -1
        assert L.isal_hip_batch_dif_verify(unaligned._h, 512, ctypes.byref(d), p, p, None) == -1
        with pytest.raises(RuntimeError):
            unaligned.dif_generate(512, out.buf)
        with pytest.raises(RuntimeError):
            good.dif_verify(512, out.buf, out.buf, type=2)
        torch.cuda.synchronize()
        assert engine.kernel_launches() == before
        assert (out.read("refusals") == GARBAGE[8]).all()
    finally:
        good.close()
        rg.close()
        unaligned.close()


def test_all_zero_lengths_enqueue_nothing(engine, gpu):
    k, rows = 3, 2
    st = Stripes(gpu, "rs", k, rows, [0, 0, 0], 7)
    rg = engine.Ragged(k, rows, st.tbls, st.lens, st.data, st.coding)
    bt = engine.Batch(0, k, rows, st.tbls, st.S, st.data, st.coding)
    out, bad = Out(gpu, 16, 8), Out(gpu, st.S * st.m, 4)
    try:
        for obj in (rg, bt):
            _run(engine, st, lambda: obj.sector_t10dif(512, 0, out.buf), 0, "words")
            _run(engine, st, lambda: obj.dif_generate(512, out.buf), 0, "generate")
            _run(engine, st, lambda: obj.dif_verify(512, out.buf, bad.buf), 0, "verify")
            assert (out.read("zero lengths") == GARBAGE[8]).all()
            assert (bad.read("zero lengths") == GARBAGE[4]).all(), "bad written although every length is 0"
    finally:
        rg.close()
        bt.close()


def test_generate_and_verify_are_ordered_behind_encode_on_one_stream(engine, gpu):
    """ragged encode, dif_generate, dif_verify on one non-default stream with
    nothing between them: the parity sectors' tuples are those of the fresh
    parity, and verify, which reads them, is clean."""
    k, rows, S, seed = 3, 2, 512, 902
    lens = orders(S)[2]
    st = Stripes(gpu, "rs", k, rows, lens, seed)  # poisoned parity
    rg = engine.Ragged(k, rows, st.tbls, lens, st.data, st.coding)
    pi, bad = Out(gpu, _nwords(st, S), 8), Out(gpu, st.S * st.m, 4)
    stream = torch.cuda.Stream(device=gpu)
    try:
        torch.cuda.synchronize()
        rg.encode(stream.cuda_stream)
        rg.dif_generate(S, pi.buf, app_tag=APP_TAG, stream=stream.cuda_stream)
        rg.dif_verify(S, pi.buf, bad.buf, app_tag=APP_TAG, stream=stream.cuda_stream)
        stream.synchronize()
        st.same("after encode, generate and verify", st.want)
        want = _guards(k, rows, tuple(lens), seed, S, 0)
        assert np.array_equal(pi.read_bytes("side stream"), difutil.tuples(want, APP_TAG, difutil.ref_tags(st, S, 1, None)))
        assert (bad.read("side stream") == CLEAN).all()
        stale = difutil.sector_guards(difutil.shards_of(st, st.poisoned), S, 0)
        assert (stale != want).sum() > 0.9 * rows * sum(-(-n // S) for n in lens), "the case cannot tell fresh parity from poison"
    finally:
        rg.close()
