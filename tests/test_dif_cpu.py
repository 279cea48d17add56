"""CPU tier: T10 protection information (include/isal_hip.h
isal_hip_*_sector_t10dif, isal_hip_*_dif_generate, isal_hip_*_dif_verify)
without a GPU.

The checker of both tiers (difutil.py: crc16_t10dif restated from 0x8BB7)
against the fixture recorded from the reference's crc16_t10dif_base; the
refusals a host without a GPU can reach, through the raw library and through
the Python wrappers; the two refusals that depend on the object (more than 2^30
work items, unaligned uniform shards), which are decided from the object's
host fields before any HIP call, through tests/host_tables/dif_limit_check.c on
hand-filled objects (the GPU tier repeats the unaligned one on a live object);
and tests/host_tables/crc16_sector_check.c, which emulates every lane of the
sector pass on the engine's own table image, compiled plain and with ASan +
UBSan.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import difutil
import ecutil

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "isa-l_amd", "csrc")
EINVAL = -1
SECTORS = [512, 1024, 2048, 4096]
BAD_SECTORS = [0, 256, 768, 8192, -512]
KINDS = ("batch", "ragged")
SYMBOLS = [f"isal_hip_{k}_{f}" for k in KINDS for f in ("sector_t10dif", "dif_generate", "dif_verify")]


def test_the_checker_gives_the_check_value():
    assert difutil.crc16(b"123456789") == 0xD0DB
    assert difutil.golden()["check"] == 0xD0DB


def test_the_checker_equals_the_reference_fixture():
    g = difutil.golden()
    cases = g["cases"]
    assert {c["len"] for c in cases} == {0, 1, 15, 16, 17, 511, 512, 4095, 4096, 4097}
    assert {c["fill"] for c in cases} == {"0x00", "0x8a", "lcg"}
    assert len({c["seed"] for c in cases}) == 3 and 0 in {c["seed"] for c in cases}
    assert len(cases) == 10 * 3 * 3
    for c in cases:
        data = difutil.golden_input(c["fill"], c["len"])
        assert difutil.crc16(data, c["seed"]) == c["crc"], c
    # the vectorised form over many sectors at once, short last sector included
    data = difutil.golden_input("lcg", 4097)
    by = {(c["len"], c["seed"]): c["crc"] for c in cases if c["fill"] == "lcg"}
    got = difutil.sector_guards([data[:4097], data[:511], data[:0], data[:17]], 4096, 0x1D0F)
    assert [int(x) for x in got] == [by[4096, 0x1D0F], difutil.crc16(data[4096:4097], 0x1D0F), by[511, 0x1D0F],
                                     by[17, 0x1D0F]]


def test_dif_symbols_are_exported_declared_and_wrapped(engine):
    header = open(os.path.join(ROOT, "include", "isal_hip.h")).read()
    exports = open(os.path.join(CSRC, "exports.map")).read()
    for name in SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), name
        assert re.search(rf"\b{name};", exports), name
        assert getattr(engine.lib(), name).argtypes is not None, name
    for cls in (engine.Batch, engine.Ragged):
        assert callable(cls.sector_t10dif) and callable(cls.dif_generate) and callable(cls.dif_verify)
    assert (engine.DIF_TYPE1, engine.DIF_TYPE3, engine.DIF_CLEAN) == (1, 3, 0xFFFFFFFF)
    assert (engine.DIF_CHECK_GUARD, engine.DIF_CHECK_APP, engine.DIF_CHECK_REF) == (1, 2, 4)
    for define in ("ISAL_HIP_DIF_TYPE1 1", "ISAL_HIP_DIF_TYPE3 3", "ISAL_HIP_DIF_CHECK_GUARD 1u",
                   "ISAL_HIP_DIF_CHECK_APP   2u", "ISAL_HIP_DIF_CHECK_REF   4u", "ISAL_HIP_DIF_CLEAN 0xffffffffu"):
        assert f"#define {define}" in header, define
    # the two items this closes left the sector checksums' out-of-scope sentence
    doc = " ".join(header.replace(" * ", " ").split())
    assert "CRC16 T10-DIF, the 16-bit NVMe guard (a new polynomial" not in doc
    assert "crc16_t10dif[_copy][_base]" in doc and "interleaved data + PI" in doc


def _dif(engine, type_=1, flags=7):
    return engine._Dif(type_, flags, 0x1234, 0, None)


def test_dif_calls_refuse_bad_arguments_without_a_gpu(engine):
    """ISAL_HIP_EINVAL (-1) before any HIP call and before the object is
    touched: a NULL object with good and with bad arguments, and behind a
    handle that is never dereferenced a NULL d, crc, pi or bad, a bad sector, a
    bad type, flags outside the three bits and a misaligned pi; no launch."""
    L = engine.lib()
    buf = (ctypes.c_ulonglong * 4)()
    out = ctypes.c_void_p(ctypes.addressof(buf))
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    fake = ctypes.c_void_p(0x2000)  # never dereferenced
    before = engine.kernel_launches()
    for kind in KINDS:
        words = getattr(L, f"isal_hip_{kind}_sector_t10dif")
        gen = getattr(L, f"isal_hip_{kind}_dif_generate")
        ver = getattr(L, f"isal_hip_{kind}_dif_verify")
        d = _dif(engine)
        for sector in SECTORS + BAD_SECTORS:
            assert words(None, sector, 0, out, None) == EINVAL
            assert words(None, sector, 0, None, None) == EINVAL
            assert gen(None, sector, ctypes.byref(d), out, None) == EINVAL
            assert ver(None, sector, ctypes.byref(d), out, out, None) == EINVAL
        for sector in BAD_SECTORS:
            assert words(fake, sector, 0, out, None) == EINVAL
            assert gen(fake, sector, ctypes.byref(d), out, None) == EINVAL
            assert ver(fake, sector, ctypes.byref(d), out, out, None) == EINVAL
        assert words(fake, 512, 0, None, None) == EINVAL
        assert gen(fake, 512, None, out, None) == EINVAL and ver(fake, 512, None, out, out, None) == EINVAL
        assert gen(fake, 512, ctypes.byref(d), None, None) == EINVAL
        assert ver(fake, 512, ctypes.byref(d), None, out, None) == EINVAL
        assert ver(fake, 512, ctypes.byref(d), out, None, None) == EINVAL
        for off in (1, 2, 4, 7):
            p = ctypes.c_void_p(ctypes.addressof(buf) + off)
            assert gen(fake, 512, ctypes.byref(d), p, None) == EINVAL
            assert ver(fake, 512, ctypes.byref(d), p, out, None) == EINVAL
        for type_ in (0, 2, 4, -1):
            t = _dif(engine, type_=type_)
            assert gen(fake, 512, ctypes.byref(t), out, None) == EINVAL
            assert ver(fake, 512, ctypes.byref(t), out, out, None) == EINVAL
        for flags in (8, 15, 0x80000001):
            f = _dif(engine, flags=flags)
            assert ver(fake, 512, ctypes.byref(f), out, out, None) == EINVAL
    del odd
    assert engine.kernel_launches() == before and not any(buf)


@pytest.mark.parametrize("cls", ["Batch", "Ragged"])
def test_dif_wrappers_raise_on_refusals_without_a_gpu(engine, cls):
    """The Python methods pass the refusals on as RuntimeError: a closed object
    (NULL handle), and behind a handle that is never dereferenced a bad
    sector, a bad type, bad flags and a misaligned pi."""
    buf = np.zeros(8, np.uint64)
    obj = getattr(engine, cls).__new__(getattr(engine, cls))
    try:
        for h in (None, 0x2000):
            obj._h = h
            calls = [lambda: obj.sector_t10dif(768, 0, buf), lambda: obj.dif_generate(256, buf),
                     lambda: obj.dif_verify(8192, buf, buf)]
            if h is None:
                calls += [lambda: obj.sector_t10dif(512, 0, buf), lambda: obj.dif_generate(512, buf),
                          lambda: obj.dif_verify(512, buf, buf)]
            else:
                calls += [lambda: obj.dif_generate(512, buf, type=2), lambda: obj.dif_verify(512, buf, buf, type=0),
                          lambda: obj.dif_verify(512, buf, buf, flags=8),
                          lambda: obj.dif_generate(512, buf.ctypes.data + 4),
                          lambda: obj.dif_verify(512, buf.ctypes.data + 2, buf)]
            for call in calls:
                with pytest.raises(RuntimeError, match=r"failed \(-1\)"):
                    call()
    finally:
        obj._h = None  # nothing for close() to destroy
    assert not buf.any()


@pytest.mark.parametrize("san", [False, True], ids=["plain", "asan-ubsan"])
def test_crc16_sector_image_and_lane_algebra(tmp_path, san):
    """Every lane of the sector pass emulated on isal_hip_crc16_sector_image,
    all four sector sizes, against a bytewise CRC; as a plain program and as a
    stand-alone one under ASan + UBSan."""
    src = os.path.join(HERE, "host_tables", "crc16_sector_check.c")
    exe = tmp_path / "crc16_sector_check"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if san else ["-O2"]
    r = subprocess.run(["gcc", *flags, "-Wall", "-I", CSRC, "-o", str(exe), src, "-lpthread"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout and "FAIL" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_work_item_limit_and_alignment_refusals_on_hand_filled_objects(engine, tmp_path):
    """More than 2^30 work items (uniform and ragged) and unaligned uniform
    shards: ISAL_HIP_EINVAL from all six calls (and the sector checksums'
    five), nothing written, no launch counted."""
    src = os.path.join(HERE, "host_tables", "dif_limit_check.c")
    exe = tmp_path / "dif_limit_check"
    libdir = os.path.dirname(os.path.abspath(ecutil.ENGINE_LIB))
    r = subprocess.run(["gcc", "-O1", "-g", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-o", str(exe), src,
                        "-L", libdir, "-lisal_hip", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout and "FAIL" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
