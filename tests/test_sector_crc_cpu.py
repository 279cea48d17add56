"""CPU tier: sector checksums (include/isal_hip.h isal_hip_*_sector_crc*) — what
needs no GPU: the offsets arithmetic against a Python restatement, and every
refusal that a host without a GPU can reach (a NULL handle, bad arguments; an
object cannot be created here, so the checks behind a live handle are the GPU
tier's)."""
import ctypes

import numpy as np
import pytest

LENS = [0, 1, 511, 512, 513, 4095, 4096, 4097, 0, 8192 + 23]
SECTORS = [512, 1024, 2048, 4096]
BAD_SECTORS = [0, 256, 768, 8192]


def _offsets(L, lens, sector, first=True, n=None):
    ln = (ctypes.c_int * max(1, len(lens)))(*lens)
    out = (ctypes.c_longlong * max(1, len(lens)))(*([-7] * max(1, len(lens))))
    total = L.isal_hip_ragged_sector_offsets(len(lens) if n is None else n, ln, sector, out if first else None)
    return int(total), list(out)[:len(lens)]


@pytest.mark.parametrize("sector", SECTORS)
def test_sector_offsets_match_a_restatement(engine, sector):
    L = engine.lib()
    want, at = [], 0
    for n in LENS:
        want.append(at)
        at += -(-n // sector)
    total, first = _offsets(L, LENS, sector)
    assert (total, first) == (at, want)
    assert _offsets(L, LENS, sector, first=False)[0] == at  # first may be NULL
    f, t = engine.ragged_sector_offsets(LENS, sector)
    assert f.dtype == np.int64 and list(f) == want and t == at
    assert _offsets(L, [0, 0], sector) == (0, [0, 0])
    assert _offsets(L, [2**31 - 1] * 3, sector)[0] == 3 * -(-(2**31 - 1) // sector)  # no 32-bit overflow


def test_sector_offsets_refuse_what_the_contract_excludes(engine):
    L = engine.lib()
    assert L.isal_hip_ragged_sector_offsets(3, None, 512, None) == -1
    for n in (0, -1):
        assert _offsets(L, LENS, 512, n=n)[0] == -1
    assert _offsets(L, [4096, -1, 5], 512)[0] == -1
    for sector in BAD_SECTORS + [-512, 513, 4095]:
        total, first = _offsets(L, LENS, sector)
        assert total == -1 and first == [-7] * len(LENS), sector  # nothing written either
    with pytest.raises(ValueError):
        engine.ragged_sector_offsets(LENS, 768)


def test_sector_calls_refuse_bad_arguments_without_a_gpu(engine):
    """ISAL_HIP_EINVAL (-1) before any HIP call: a NULL object, with good and
    with bad other arguments, for all four launch functions; no launch counted."""
    L = engine.lib()
    word = ctypes.c_ulonglong(0)
    crc = ctypes.cast(ctypes.pointer(word), ctypes.c_void_p)
    before = engine.kernel_launches()
    for fn in (L.isal_hip_batch_sector_crc, L.isal_hip_ragged_sector_crc):
        for sector in SECTORS + BAD_SECTORS:
            assert fn(None, sector, 0x1234, crc, None) == -1
            assert fn(None, sector, 0x1234, None, None) == -1
    for fn in (L.isal_hip_batch_sector_crc64, L.isal_hip_ragged_sector_crc64):
        for variant in (-1, 0, 6, 7, 8, 1 << 20):
            for sector in SECTORS + BAD_SECTORS:
                assert fn(None, variant, sector, 0x1234, crc, None) == -1
                assert fn(None, variant, sector, 0x1234, None, None) == -1
    assert engine.kernel_launches() == before and word.value == 0
