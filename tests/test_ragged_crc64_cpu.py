"""CPU tier: the ragged CRC64 checksum (include/isal_hip.h isal_hip_ragged_crc64,
isal_hip_ragged_encode_crc64) without a GPU.

The symbols are exported, declared and wrapped; NULL arguments and variants
outside [0, 8) are refused before any HIP call and before the handle is
touched; and tests/host_tables/crc64_ragged_check.c pins, for all eight
flavours, the quotient-ring arithmetic (crc64_host.c isal_hip_crc64_mulmod,
isal_hip_crc64_xpow8n) against the matrix form, the length-independent host
image (isal_hip_crc64_ragged_image) and the algebra of both kernels: it
emulates every lane of the pass and of the combine from that image for tt = 2
and tt = 128 over the GPU test's lengths, 200 seeded random lengths and three
init values, compares with a bytewise CRC, and compares every derived constant
with the uniform batch's per-length maps on the 64 basis values. The same
program runs once more as a stand-alone ASan + UBSan executable.
"""
import ctypes
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "isa-l_amd", "csrc")
CHECK = os.path.join(HERE, "host_tables", "crc64_ragged_check.c")
EINVAL = -1
NVARIANTS = 8
SYMBOLS = ["isal_hip_ragged_crc64", "isal_hip_ragged_encode_crc64"]


def test_ragged_crc64_symbols_are_exported_declared_and_wrapped(engine):
    header = open(os.path.join(ROOT, "include", "isal_hip.h")).read()
    exports = open(os.path.join(CSRC, "exports.map")).read()
    for name in SYMBOLS:
        assert re.search(rf"\bint {name}\(isal_hip_ragged \*r, int variant, unsigned long long init,\s*"
                         rf"unsigned long long \*crc, void \*stream\);", header), name
        assert re.search(rf"\b{name};", exports), name
        assert getattr(engine.lib(), name).argtypes is not None, name
    assert callable(engine.Ragged.crc64) and callable(engine.Ragged.encode_crc64)
    assert len(engine.CRC64_VARIANTS) == NVARIANTS
    # the header states the launch count, both sizes as formulas, the zero-length rule and what stays out
    doc = header[header.index("isal_hip_ragged_crc64: isal_hip_ragged_crc for the eight"):
                 header.index("typedef struct isal_hip_ragged ")]
    doc = " ".join(doc.replace(" * ", " ").split())
    for phrase in ["2 kernel launches", "8*(11104 + tt + 1) bytes", "2 KiB per block of every shard", "length 0",
                   "words are init", "independent of what isal_hip_ragged_crc keeps", "Not a fused pass",
                   "CRC64 fused into the encode"]:
        assert phrase in doc, phrase


def test_ragged_crc64_header_states_the_image_size_the_host_builds(tmp_path):
    """The formula in the header is the size function's (crc64_host.c)."""
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "isal_hip_internal.h"\n'
                   'int main(void) { printf("%zu %zu\\n", isal_hip_crc64_ragged_image_entries(0), '
                   'isal_hip_crc64_ragged_image_entries(128)); return 0; }\n')
    exe = tmp_path / "size"
    r = subprocess.run(["gcc", "-O1", "-I", CSRC, "-o", str(exe), str(src), os.path.join(CSRC, "crc64_host.c"),
                        "-lpthread"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.split()
    assert [int(x) for x in out] == [11104 + 0 + 1, 11104 + 128 + 1]


def test_ragged_crc64_rejects_bad_arguments_without_gpu(engine):
    L = engine.lib()
    words = ctypes.c_void_p(0x1000)  # never dereferenced
    fake = ctypes.c_void_p(0x2000)   # never dereferenced either: every refusal below comes first
    for name in SYMBOLS:
        fn = getattr(L, name)
        assert fn(None, 0, 0, words, None) == EINVAL
        assert fn(None, 6, 0xFFFFFFFFFFFFFFFF, None, None) == EINVAL
        assert fn(fake, 7, 7, None, None) == EINVAL  # NULL crc
        for variant in (-1, NVARIANTS, 1 << 20):
            assert fn(fake, variant, 0, words, None) == EINVAL, variant


def _build(exe, flags):
    return subprocess.run(["gcc", *flags, "-Wall", "-I", CSRC, "-o", str(exe), CHECK, "-lpthread"],
                          capture_output=True, text=True, timeout=300)


def _run_check(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout and "FAIL" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_ragged_crc64_ring_host_image_and_kernel_algebra(tmp_path):
    exe = tmp_path / "crc64_ragged_check"
    r = _build(exe, ["-O2"])
    assert r.returncode == 0, r.stderr[-3000:]
    _run_check(exe)


def test_ragged_crc64_host_check_under_asan_and_ubsan(tmp_path):
    """The same stand-alone program with the sanitizers compiled in (nothing is
    loaded into Python)."""
    exe = tmp_path / "crc64_ragged_check_san"
    r = _build(exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0 and re.search(r"cannot find.*(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("the sanitizer runtimes do not link here")
    assert r.returncode == 0, r.stderr[-3000:]
    _run_check(exe)
