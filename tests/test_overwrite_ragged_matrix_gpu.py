"""GPU tier: every instantiation of ec_overwrite_rag, launched once and
compared with the oracle.

The kernel is compiled per pass width P (1..8) and per COMMIT (0, 1) at 128
lanes: 16 instantiations, each its own register allocation.
tests/test_overwrite_ragged_objects_cpu.py holds CELLS equal to what the code
object was built with; the test below launches every cell of CELLS through the
public object, as tests/test_kernel_matrix_gpu.py does for the other families.

Each cell proves which kernel ran: under ISAL_HIP_LOG=2 the library's
`isal_hip: kernel NAME<...>` line must name exactly the cell's instantiation,
once, and kernel_launches() must grow by 1.

Shape: k = 6, the seven lengths of test_ragged_gpu.lens7(2048) (a stripe of no
byte, a byte tail, one vector, one tile, a tile and a vector, two tiles with
vector lanes and a tail, one byte), the counts cycling through 1, 2, 3: the
pair group alone, the single group alone, and both.
"""
import numpy as np
import pytest

import test_overwrite_ragged_gpu as owrag_mod
import test_ragged_gpu as rag_mod
from test_kernel_matrix_gpu import Launches, _knobs

pytestmark = pytest.mark.gpu

ROWS = tuple(range(1, 9))
BLOCK = 128
# the template arguments of every instantiation, as the launch log prints them
CELLS = {(P, C, BLOCK) for P in ROWS for C in (0, 1)}


@pytest.fixture(autouse=True)
def _reload_knobs_after(engine):
    """Knobs are read once by the library: every test leaves it re-synced with
    os.environ."""
    yield
    engine.reload_config()


@pytest.mark.parametrize("commit", [0, 1])
def test_ragged_overwrite_every_rows(engine, oracle, gpu, monkeypatch, capfd, commit):
    """Parity == a fresh oracle encode of the new data; with COMMIT old == new
    afterwards, without it a second run restores the image."""
    k = 6
    cells = sorted(c for c in CELLS if c[1] == commit)
    assert [c[0] for c in cells] == list(ROWS)
    _knobs(engine, monkeypatch, {})
    lens = rag_mod.lens7(BLOCK * 16)
    counts = [1 + s % 3 for s in range(len(lens))]
    assert set(counts) == {1, 2, 3}
    for cell in cells:
        P = cell[0]
        name = f"ec_overwrite_rag<{', '.join(str(x) for x in cell)}>"
        sets = owrag_mod._sets(k, counts, 100 * P + commit)
        w = owrag_mod.RaggedWrites(oracle, gpu, "cauchy", k, P, lens, sets, 60 + P)
        assert w.max_nw == 3 and w.live == 6
        run = Launches(engine, capfd, name)
        ow = w.overwrite(engine)
        try:
            run(lambda: ow.run(commit=bool(commit)))
            if commit:
                got = w.check(w.committed, name)
                for s, ix in enumerate(sets):  # old == new
                    for i, j in enumerate(ix):
                        assert np.array_equal(got[s * w.m + j], got[w.new0 + s * w.max_nw + i]), (name, s, i)
            else:
                w.check(w.parity_only, name)
                run(lambda: ow.run(commit=False))
                w.check(w.before, name + " second run")
        finally:
            ow.close()
