"""CPU tier: the ragged checksum (include/isal_hip.h isal_hip_ragged_crc,
isal_hip_ragged_encode_crc) without a GPU.

The symbols are exported, declared and wrapped; NULL arguments are refused
before any HIP call; and tests/host_tables/crc32c_ragged_check.c pins the
length-independent host image (crc_host.c isal_hip_crc32c_ragged_image) and
the algebra of both kernels: it emulates every lane of the pass and of the
combine from that image for tt = 2 and tt = 64 over the GPU test's lengths,
200 seeded random lengths and three init values, compares with the bytewise
CRC, and compares every derived constant with the uniform batch's per-length
plan word for word.
"""
import ctypes
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "isa-l_amd", "csrc")
EINVAL = -1
SYMBOLS = ["isal_hip_ragged_crc", "isal_hip_ragged_encode_crc"]


def test_ragged_crc_symbols_are_exported_declared_and_wrapped(engine):
    header = open(os.path.join(ROOT, "include", "isal_hip.h")).read()
    exports = open(os.path.join(CSRC, "exports.map")).read()
    for name in SYMBOLS:
        assert re.search(rf"\bint {name}\(isal_hip_ragged \*r, unsigned int init, unsigned int \*crc,\s*void \*stream\);",
                         header), name
        assert re.search(rf"\b{name};", exports), name
        assert getattr(engine.lib(), name).argtypes is not None, name
    assert callable(engine.Ragged.crc) and callable(engine.Ragged.encode_crc)
    # the header states the launch count, the memory, the zero-length rule and what stays out
    doc = header[header.index("isal_hip_ragged_crc: the isal_hip_batch_crc contract"):header.index("typedef struct isal_hip_ragged ")]
    for phrase in ["2 kernel launches", "45 KiB", "length 0", "words are init", "NOT fused",
                   "one-pass fused encode + checksum, CRC64"]:
        assert phrase in " ".join(doc.replace(" * ", " ").split()), phrase


def test_ragged_crc_rejects_null_arguments_without_gpu(engine):
    L = engine.lib()
    words = ctypes.c_void_p(0x1000)  # never dereferenced
    fake = ctypes.c_void_p(0x2000)
    for name in SYMBOLS:
        fn = getattr(L, name)
        assert fn(None, 0, words, None) == EINVAL
        assert fn(None, 0xFFFFFFFF, None, None) == EINVAL
        assert fn(fake, 7, None, None) == EINVAL  # NULL crc: refused before the object is touched


def test_ragged_crc_host_image_and_kernel_algebra(tmp_path):
    src = os.path.join(HERE, "host_tables", "crc32c_ragged_check.c")
    exe = tmp_path / "crc32c_ragged_check"
    r = subprocess.run(["gcc", "-O2", "-Wall", "-I", CSRC, "-o", str(exe), src, "-lpthread"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout and "FAIL" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
