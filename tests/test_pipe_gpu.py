"""GPU tier: the host pipeline (isal_hip_pipe_*, isa-l_amd/csrc/isal_hip_pipe.c)
and the multi-device encode (isal_hip_multi_*, isal_hip_multi.c) beyond the one
geometry of test_gpu_parity.py: host shards that are not one contiguous block
(one copy per run of adjacent shards, partial runs, runs of one), lengths that
are no multiple of 16 (byte-lane kernels on misaligned device slots), encode
geometries without LDS product tables and with more rows than one pass, 0/1
coefficient masks, every depth, handle reuse, destroy with work queued, two
pipelines at once, and multi with fewer stripes than slots.

Every case compares every parity byte with oracle.encode of the same sources.
Host shards are carved from one arena per case (pinned or pageable) with 64
guard bytes of 0x5A before, between and after them; parity starts as 0xEE and
every stripe has its own source bytes, so a stale slot or a swapped stripe
cannot compare equal. After the flush the WHOLE arena is compared: every guard
and every source byte must be unchanged.

What this file cannot see is ordering: on a GPU a missing event edge usually
still gives the right bytes. tests/sanitize/pipe_host.c checks the ordering on
a deferred model of HIP streams (and cannot see the kernels).
"""
import threading

import numpy as np
import pytest

from ecutil import fill_bytes

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE, FRESH = 64, 0x5A, 0xEE
PARITY_LAYOUTS = ["block", "gapped", "reversed", "pairs"]
SOURCE_LAYOUTS = PARITY_LAYOUTS + ["aliased"]


@pytest.fixture(autouse=True, scope="module")
def _force_gpu_route(engine):
    """The drop-in calls of this module run the GPU kernels (device shards do
    anyway; the knob keeps the module independent of the library's default)."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("ISAL_HIP_BACKEND", "gpu")
        engine.reload_config()
        yield
    engine.reload_config()


def layout(name, n, length):
    """Offsets of a stripe's n shards from its base, the bytes they span, and
    the runs the layout consists of: lengths, in shards, of the maximal groups
    adjacent in memory AND in index order (what the pipeline may move as one
    copy; tests/sanitize/pipe_host.c asserts the copies against the same runs).

      block     adjacent in index order                      one run of n
      gapped    a guard between any two                      n runs of 1
      reversed  adjacent, at descending addresses            n runs of 1
      pairs     runs of two, a guard between runs            n//2 runs of 2 (+ one of 1)
      aliased   block, but index 2 names shard 0's buffer    {0,1} {2} {3..n-1}; sources only
    """
    if name == "block":
        offs, runs = [i * length for i in range(n)], [n]
    elif name == "gapped":
        offs, runs = [i * (length + GUARD) for i in range(n)], [1] * n
    elif name == "reversed":
        offs, runs = [(n - 1 - i) * length for i in range(n)], [1] * n
    elif name == "pairs":
        offs = [(i // 2) * (2 * length + GUARD) + (i % 2) * length for i in range(n)]
        runs = [2] * (n // 2) + [1] * (n % 2)
    elif name == "aliased":
        assert n >= 4
        offs = [i * length for i in range(n)]
        offs[2] = offs[0]
        runs = [2, 1, n - 3]
    else:
        raise ValueError(name)
    assert sum(runs) == n
    return offs, max(offs) + length, runs


class HostStripes:
    """`stripes` host stripes of k sources and `rows` parity shards of `length`
    bytes inside one arena tensor: [guard][sources][guard][parity] per stripe,
    then a last guard. The first shard sits `misalign` bytes past a 16-byte
    boundary."""

    def __init__(self, stripes, k, rows, length, src_layout="block", par_layout="block", pinned=True, seed=0,
                 misalign=0):
        import torch

        self.stripes, self.k, self.rows, self.length = stripes, k, rows, length
        soffs, sspan, self.src_runs = layout(src_layout, k, length)
        poffs, pspan, self.par_runs = layout(par_layout, rows, length)
        per = GUARD + sspan + GUARD + pspan
        total = stripes * per + GUARD
        self.tensor = torch.empty(total + 32, dtype=torch.uint8)
        if pinned:
            self.tensor = self.tensor.pin_memory()
        start = (-self.tensor.data_ptr()) % 16 + misalign
        self.arena = self.tensor.numpy()[start:start + total]
        self.base = self.tensor.data_ptr() + start
        self.arena[:] = GUARD_BYTE
        self.src_off = [[s * per + GUARD + o for o in soffs] for s in range(stripes)]
        self.par_off = [[s * per + GUARD + sspan + GUARD + o for o in poffs] for s in range(stripes)]
        for s in range(stripes):
            done = set()
            for j, o in enumerate(self.src_off[s]):
                if o not in done:  # an aliased index keeps the bytes of the buffer it names
                    self.arena[o:o + length] = fill_bytes(length, (seed * 1000 + s) * 1000 + j)
                    done.add(o)
            for o in self.par_off[s]:
                self.arena[o:o + length] = FRESH
        self.before = self.arena.copy()

    def data(self, s):
        return [self.base + o for o in self.src_off[s]]

    def coding(self, s):
        return [self.base + o for o in self.par_off[s]]

    def all_data(self):
        return [p for s in range(self.stripes) for p in self.data(s)]

    def all_coding(self):
        return [p for s in range(self.stripes) for p in self.coding(s)]

    def parity(self, s):
        return [self.arena[o:o + self.length].copy() for o in self.par_off[s]]

    def check(self, oracle, coef, what=()):
        """Every parity byte equals the oracle's; every other byte of the arena
        (guards, sources) is what it was before the run."""
        want = self.before.copy()
        for s in range(self.stripes):
            src = [self.before[o:o + self.length] for o in self.src_off[s]]
            par = oracle.encode(coef, self.k, self.rows, src)
            for l, o in enumerate(self.par_off[s]):
                want[o:o + self.length] = par[l]
        if not np.array_equal(self.arena, want):
            i = int(np.flatnonzero(self.arena != want)[0])
            where = "a guard or source byte"
            for s in range(self.stripes):
                for l, o in enumerate(self.par_off[s]):
                    if o <= i < o + self.length:
                        where = f"stripe {s} parity row {l} byte {i - o}"
            raise AssertionError(f"{what}: {where} (arena offset {i}) is {self.arena[i]:#x}, not {want[i]:#x}")


def rs_tables(engine, k, rows):
    a = engine.gf_gen_rs_matrix(k + rows, k)
    return a[k * k:].copy(), engine.ec_init_tables(k, rows, a[k * k:])


def run_pipe(pipe, host, first=0, count=None):
    for s in range(first, first + (host.stripes if count is None else count)):
        pipe.submit(host.data(s), host.coding(s))


# --------------------------------------------------------------------------
# 1. layouts: one copy and one event per run of adjacent shards
# --------------------------------------------------------------------------

@pytest.mark.parametrize("par_layout", PARITY_LAYOUTS)
@pytest.mark.parametrize("src_layout", SOURCE_LAYOUTS)
@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
@pytest.mark.parametrize("mode", ["update", "encode"])
def test_pipe_host_layouts_vs_oracle(engine, oracle, gpu, mode, pinned, src_layout, par_layout):
    k, p, n, depth, ns = 5, 3, 4096 + 16, 2, 5
    coef, tbls = rs_tables(engine, k, p)
    host = HostStripes(ns, k, p, n, src_layout, par_layout, pinned, seed=1)
    pipe = engine.Pipe(n, k, p, tbls, depth=depth, mode=mode)
    run_pipe(pipe, host)
    pipe.flush()
    pipe.close()
    host.check(oracle, coef, (mode, pinned, src_layout, par_layout))


# --------------------------------------------------------------------------
# 2. lengths: len % 16 != 0 puts the slot's shards at d_buf + i*len
#    (misaligned) and runs the byte-lane kernels
# --------------------------------------------------------------------------

@pytest.mark.parametrize("odd_host", [False, True], ids=["aligned", "oddaddr"])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 255, 256, 4080, 4096, 4099, 8192 + 16, 65536 + 48])
@pytest.mark.parametrize("k,p", [(4, 2), (10, 4)])
@pytest.mark.parametrize("mode", ["update", "encode"])
def test_pipe_lengths_vs_oracle(engine, oracle, gpu, mode, k, p, n, odd_host):
    # odd_host with n % 16 == 0: the host shards sit at odd addresses, but the
    # device slot is aligned, so the pipeline still takes its 16-byte kernels
    # and a misaligned HOST buffer must not matter.
    coef, tbls = rs_tables(engine, k, p)
    host = HostStripes(4, k, p, n, "block", "gapped", pinned=True, seed=2, misalign=(1 if k == 4 else 3) * odd_host)
    assert host.base % 16 == ((1 if k == 4 else 3) if odd_host else 0)
    pipe = engine.Pipe(n, k, p, tbls, depth=3, mode=mode)
    run_pipe(pipe, host)
    pipe.flush()
    pipe.close()
    host.check(oracle, coef, (mode, k, p, n, odd_host))


# --------------------------------------------------------------------------
# 3. depth and handle reuse
# --------------------------------------------------------------------------

@pytest.mark.parametrize("which", range(4), ids=["1", "d", "d+1", "3d+1"])
@pytest.mark.parametrize("depth", [1, 2, 3, 4, 9])
@pytest.mark.parametrize("mode", ["update", "encode"])
def test_pipe_depth_and_second_wave_vs_oracle(engine, oracle, gpu, mode, depth, which):
    k, p, n = 4, 2, 4096 + 16
    d = min(depth, 4)  # ISAL_HIP_PIPE_MAX_DEPTH caps 9
    ns = [1, d, d + 1, 3 * d + 1][which]
    coef, tbls = rs_tables(engine, k, p)
    first = HostStripes(ns, k, p, n, "block", "block", pinned=True, seed=3)
    second = HostStripes(d + 2, k, p, n, "block", "block", pinned=True, seed=4)
    pipe = engine.Pipe(n, k, p, tbls, depth=depth, mode=mode)
    run_pipe(pipe, first)
    pipe.flush()
    first.check(oracle, coef, (mode, depth, ns, "first wave"))
    # other stripes into fresh parity buffers: the slot phase goes on mid-cycle
    run_pipe(pipe, second)
    pipe.flush()
    pipe.close()
    second.check(oracle, coef, (mode, depth, ns, "second wave"))
    first.check(oracle, coef, (mode, depth, ns, "first wave after the second"))


@pytest.mark.parametrize("mode", ["update", "encode"])
def test_pipe_flush_with_nothing_queued(engine, oracle, gpu, mode):
    k, p, n = 4, 2, 4096 + 16
    coef, tbls = rs_tables(engine, k, p)
    pipe = engine.Pipe(n, k, p, tbls, depth=3, mode=mode)
    pipe.flush()  # nothing submitted
    pipe.flush()
    host = HostStripes(2, k, p, n, seed=5)
    run_pipe(pipe, host)
    pipe.flush()
    pipe.flush()  # two in a row
    host.check(oracle, coef, (mode, "after the flushes"))
    pipe.close()
    host.check(oracle, coef, (mode, "after close"))


@pytest.mark.parametrize("ns", [1, 3, 7])
@pytest.mark.parametrize("mode", ["update", "encode"])
def test_pipe_close_without_flush_drains(engine, oracle, gpu, mode, ns):
    """isal_hip_pipe_destroy with work queued: the parity is there once it returns."""
    k, p, n = 4, 2, 4096 + 16
    coef, tbls = rs_tables(engine, k, p)
    host = HostStripes(ns, k, p, n, "gapped", "gapped", pinned=True, seed=6)
    pipe = engine.Pipe(n, k, p, tbls, depth=3, mode=mode)
    run_pipe(pipe, host)
    pipe.close()
    host.check(oracle, coef, (mode, ns))


# --------------------------------------------------------------------------
# 4. geometries: without LDS product tables (k > 64, rows < 4), one row, one
#    source, more rows than one pass (R = rows per pass)
# --------------------------------------------------------------------------

GEOMETRIES = [(1, 1), (2, 1), (1, 4), (10, 3), (10, 4), (64, 4), (65, 4), (20, 8), (10, "R+1"), (10, "2R+1")]


@pytest.mark.parametrize("n", [4096 + 16, 4099])
@pytest.mark.parametrize("k,rows", GEOMETRIES, ids=[f"k{k}-rows{r}" for k, r in GEOMETRIES])
@pytest.mark.parametrize("mode", ["update", "encode"])
def test_pipe_geometries_vs_oracle(engine, oracle, gpu, mode, k, rows, n):
    R = engine.max_rows_per_pass()
    rows = {"R+1": R + 1, "2R+1": 2 * R + 1}.get(rows, rows)
    ns = 3
    coef, tbls = rs_tables(engine, k, rows)
    host = HostStripes(ns, k, rows, n, "block", "block", pinned=True, seed=7)
    pipe = engine.Pipe(n, k, rows, tbls, depth=2, mode=mode)
    launches = engine.kernel_launches()
    run_pipe(pipe, host)
    pipe.flush()
    assert engine.kernel_launches() >= launches + ns
    pipe.close()
    host.check(oracle, coef, (mode, k, rows, n))


# --------------------------------------------------------------------------
# 5. coefficients: the encode launch gets isal_hip_enc_masks of the tables
#    (0/1 first row and first column of a pass become XORs)
# --------------------------------------------------------------------------

def _matrices(oracle, k, rows):
    rnd = fill_bytes(k * rows, 0xC0EF).reshape(rows, k).copy()
    rnd[rnd < 2] = 7  # no accidental 0 or 1
    rs = oracle.gf_gen_rs_matrix(k + rows, k)[k * k:].reshape(rows, k).copy()
    cauchy = oracle.gf_gen_cauchy1_matrix(k + rows, k)[k * k:].reshape(rows, k).copy()
    ones_row = rnd.copy()
    ones_row[0, :] = 1
    ones_row[:, 0] = [1, 0, 1, 0][:rows]  # and a 0/1 first column: the masks apply
    zero_row = rnd.copy()
    zero_row[2, :] = 0
    zero_row0 = rnd.copy()
    zero_row0[0, :] = 0
    zero_row0[:, 0] = 0
    zero_col = rnd.copy()
    zero_col[:, 0] = 0
    zero_col[0, :] = [0, 1, 0, 1, 1, 0][:k]  # and a 0/1 first row: the masks apply
    zero_col_plain = rnd.copy()
    zero_col_plain[:, 3] = 0
    copies = np.zeros((rows, k), np.uint8)
    for l in range(rows):
        copies[l, (2 * l + 1) % k] = 1  # parity l = a copy of source (2l+1) % k
    return {"rs": rs, "cauchy": cauchy, "ones_row": ones_row, "zero_row": zero_row, "zero_row0": zero_row0,
            "zero_col0": zero_col, "zero_col3": zero_col_plain, "copies": copies}


@pytest.mark.parametrize("name", ["rs", "cauchy", "ones_row", "zero_row", "zero_row0", "zero_col0", "zero_col3",
                                  "copies"])
def test_pipe_coefficient_masks_vs_oracle(engine, oracle, gpu, name):
    k, rows, n, ns = 6, 4, 4096 + 16, 3
    coef = np.ascontiguousarray(_matrices(oracle, k, rows)[name].reshape(-1))
    tbls = engine.ec_init_tables(k, rows, coef)
    got = {}
    for mode in ("update", "encode"):
        host = HostStripes(ns, k, rows, n, "block", "block", pinned=True, seed=8)
        pipe = engine.Pipe(n, k, rows, tbls, depth=2, mode=mode)
        run_pipe(pipe, host)
        pipe.flush()
        pipe.close()
        host.check(oracle, coef, (name, mode))
        got[mode] = [host.parity(s) for s in range(ns)]
    for s in range(ns):
        for l in range(rows):
            assert np.array_equal(got["update"][s][l], got["encode"][s][l]), (name, s, l)
    if name == "copies":
        src = [host.before[o:o + n] for o in host.src_off[0]]
        for l in range(rows):
            assert np.array_equal(got["encode"][0][l], src[(2 * l + 1) % k]), l


# --------------------------------------------------------------------------
# 6. concurrency
# --------------------------------------------------------------------------

def _in_threads(fns):
    errs = []

    def run(f):
        try:
            f()
        except BaseException as e:  # noqa: BLE001 - reported by the caller's assert
            errs.append(e)

    ts = [threading.Thread(target=run, args=(f,)) for f in fns]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs


def test_two_pipes_from_two_threads(engine, oracle, gpu):
    """Two pipelines of different geometry driven at once (ctypes releases the
    GIL inside submit and flush); each == oracle."""
    geo = [(5, 3, 4096 + 16, "update", 2), (10, 4, 4099, "encode", 3)]
    jobs = []
    for i, (k, p, n, mode, depth) in enumerate(geo):
        coef, tbls = rs_tables(engine, k, p)
        host = HostStripes(9, k, p, n, "pairs", "gapped", pinned=True, seed=10 + i)
        jobs.append((coef, host, engine.Pipe(n, k, p, tbls, depth=depth, mode=mode)))
    start = threading.Barrier(2)

    def drive(host, pipe):
        start.wait()
        run_pipe(pipe, host)
        pipe.flush()

    _in_threads([lambda h=host, q=pipe: drive(h, q) for _, host, pipe in jobs])
    for (coef, host, pipe), g in zip(jobs, geo):
        pipe.close()
        host.check(oracle, coef, g)


@pytest.mark.parametrize("mode", ["update", "encode"])
def test_pipe_submits_alternate_with_dropin_calls(engine, oracle, gpu, mode):
    """pipe.submit and drop-in ec_encode_data on device shards, turn by turn
    from one thread: the pipeline's streams and the drop-in's do not disturb
    each other."""
    import torch

    k, p, n, ns = 5, 3, 4096 + 16, 7
    coef, tbls = rs_tables(engine, k, p)
    host = HostStripes(ns, k, p, n, "gapped", "pairs", pinned=True, seed=12)
    dk, dp, dn = 10, 4, 8192 + 16
    dcoef, dtbls = rs_tables(engine, dk, dp)
    dsrc_h = np.stack([np.stack([fill_bytes(dn, 77000 + 100 * s + j) for j in range(dk)]) for s in range(ns)])
    dsrc = torch.from_numpy(dsrc_h).to(gpu)
    dpar = torch.full((ns, dp, dn), FRESH, dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    pipe = engine.Pipe(n, k, p, tbls, depth=2, mode=mode)
    for s in range(ns):
        pipe.submit(host.data(s), host.coding(s))
        engine.ec_encode_data(dn, dk, dp, dtbls, [dsrc[s, j] for j in range(dk)], [dpar[s, l] for l in range(dp)])
    pipe.flush()
    pipe.close()
    host.check(oracle, coef, mode)
    got = dpar.cpu().numpy()
    for s in range(ns):
        want = oracle.encode(dcoef, dk, dp, [dsrc_h[s, j] for j in range(dk)])
        for l in range(dp):
            assert np.array_equal(got[s, l], want[l]), (mode, s, l)


# --------------------------------------------------------------------------
# 7. multi: fewer stripes than slots and than devices, handle reuse, two callers
# --------------------------------------------------------------------------

@pytest.mark.parametrize("n", [4096 + 16, 4099])
@pytest.mark.parametrize("ns", [1, 2, 3, 9])  # 3 = depth + 1
@pytest.mark.parametrize("ndev", [1, 0])
def test_multi_encode_few_stripes_and_reuse_vs_oracle(engine, oracle, gpu, ndev, ns, n):
    import torch

    k, p, depth = 10, 4, 2
    coef, tbls = rs_tables(engine, k, p)
    m = engine.Multi(n, k, p, tbls, ndev=ndev, depth=depth)
    assert m.ndev == (ndev or torch.cuda.device_count())
    first = HostStripes(ns, k, p, n, "gapped", "pairs", pinned=True, seed=13)
    launches = engine.kernel_launches()
    m.encode(ns, first.all_data(), first.all_coding())
    assert engine.kernel_launches() >= launches + ns
    first.check(oracle, coef, (ndev, ns, n, "first call"))
    # the same handle again, other data
    second = HostStripes(ns, k, p, n, "gapped", "pairs", pinned=True, seed=14)
    m.encode(ns, second.all_data(), second.all_coding())
    m.close()
    second.check(oracle, coef, (ndev, ns, n, "second call"))
    first.check(oracle, coef, (ndev, ns, n, "first call after the second"))


def test_multi_encode_two_callers_on_one_handle(engine, oracle, gpu):
    """Two threads call encode on one handle with disjoint buffers: the handle's
    mutex serialises them; both results are right."""
    k, p, n, depth = 10, 4, 4096 + 16, 2
    coef, tbls = rs_tables(engine, k, p)
    m = engine.Multi(n, k, p, tbls, ndev=0, depth=depth)
    hosts = [HostStripes(5, k, p, n, "gapped", "pairs", pinned=True, seed=15),
             HostStripes(4, k, p, n, "pairs", "gapped", pinned=True, seed=16)]
    start = threading.Barrier(2)

    def call(h):
        start.wait()
        m.encode(h.stripes, h.all_data(), h.all_coding())

    _in_threads([lambda h=h: call(h) for h in hosts])
    m.close()
    for i, h in enumerate(hosts):
        h.check(oracle, coef, ("caller", i))
