"""isal_amd — Python mirror of the reference erasure-code API over libisal_hip.so.

The product is the C-ABI library ``isa-l_amd/lib/libisal_hip.so`` (headers in
``include/``). This module binds it with ctypes, keeping the reference's
function names, argument order and meaning (reference include/erasure_code.h,
include/gf_vect_mul.h), so tests and the benchmark read like the reference's
own C tests. Buffers may be numpy uint8 arrays (host memory), torch tensors
(host or device; their storage address is passed), or raw integer addresses.

There is no Python fallback: every data-path call goes through the library
(a missing library raises immediately). The library itself routes each
drop-in call (include/isal_hip.h "routing"): device-resident shards and large
host calls to the GPU kernels, small host calls to its CPU route;
ISAL_HIP_BACKEND=gpu forces the kernels.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence

import numpy as np

__all__ = [
    "LIB_PATH", "lib", "gf_mul", "gf_inv", "gf_gen_rs_matrix", "gf_gen_cauchy1_matrix",
    "gf_invert_matrix", "gf_vect_mul_init", "ec_init_tables", "ec_encode_data",
    "ec_encode_data_base", "ec_encode_data_update", "ec_encode_data_update_base",
    "gf_vect_dot_prod", "gf_vect_dot_prod_base", "gf_vect_mad", "gf_vect_mad_base",
    "gf_vect_mul", "gf_vect_mul_base", "Batch", "Repair", "decode_matrix", "ESINGULAR", "Scrub", "scrub_ambiguity",
    "locate_syndrome", "SCRUB_CLEAN", "SCRUB_MULTI", "Ragged", "ragged_items", "ragged_sector_offsets", "Pipe", "kernel_launches", "max_rows_per_pass",
    "version", "addr", "cpu_calls", "fallbacks", "reload_config", "Multi", "partition",
    "route_device", "contexts_created", "selftest_kernels", "crc32_iscsi", "crc64", "CRC64_VARIANTS", "slow_waits",
    "DIF_TYPE1", "DIF_TYPE3", "DIF_CHECK_GUARD", "DIF_CHECK_APP", "DIF_CHECK_REF", "DIF_CHECK_ALL", "DIF_CLEAN",
]

LIB_PATH = os.environ.get(
    "ISAL_HIP_LIB",
    os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "lib", "libisal_hip.so"),
)

_u8p = ctypes.POINTER(ctypes.c_ubyte)
_u8pp = ctypes.POINTER(_u8p)
_lib = None


# Variant numbers of isal_hip_batch_crc64 (ISAL_HIP_CRC64_*): the crc64_*
# functions of the reference's include/crc64.h, in its order.
CRC64_VARIANTS = ("ecma_refl", "ecma_norm", "iso_refl", "iso_norm",
                  "jones_refl", "jones_norm", "rocksoft_refl", "rocksoft_norm")


def _one_hip_runtime() -> None:
    """A process must hold exactly ONE HIP runtime. PyTorch-ROCm ships its own
    libamdhip64.so.7; if libisal_hip.so were loaded first it would bind
    /opt/rocm's copy, torch would then load a second one, and whichever
    initialises second sees no device. Loading torch first makes the engine's
    NEEDED libamdhip64.so.7 resolve to the runtime torch already holds (same
    SONAME), so device pointers and streams are shared. Set ISAL_AMD_NO_TORCH=1
    in processes that never use torch."""
    if os.environ.get("ISAL_AMD_NO_TORCH"):
        return
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def lib() -> ctypes.CDLL:
    """Load libisal_hip.so (raises if it has not been built: no silent fallback)."""
    global _lib
    if _lib is None:
        path = os.path.abspath(LIB_PATH)
        if not os.path.exists(path):
            raise RuntimeError(f"libisal_hip.so not built at {path}: run `make -C isa-l_amd`")
        _one_hip_runtime()
        L = ctypes.CDLL(path)
        i, v = ctypes.c_int, None
        sig = {
            "gf_mul": (ctypes.c_ubyte, [ctypes.c_ubyte, ctypes.c_ubyte]),
            "gf_inv": (ctypes.c_ubyte, [ctypes.c_ubyte]),
            "gf_gen_rs_matrix": (v, [_u8p, i, i]),
            "gf_gen_cauchy1_matrix": (v, [_u8p, i, i]),
            "gf_invert_matrix": (i, [_u8p, _u8p, i]),
            "gf_vect_mul_init": (v, [ctypes.c_ubyte, _u8p]),
            "gf_vect_mul_init_base": (v, [ctypes.c_ubyte, _u8p]),
            "ec_init_tables": (v, [i, i, _u8p, _u8p]),
            "ec_init_tables_base": (v, [i, i, _u8p, _u8p]),
            "ec_encode_data": (v, [i, i, i, _u8p, _u8pp, _u8pp]),
            "ec_encode_data_base": (v, [i, i, i, _u8p, _u8pp, _u8pp]),
            "ec_encode_data_update": (v, [i, i, i, i, _u8p, _u8p, _u8pp]),
            "ec_encode_data_update_base": (v, [i, i, i, i, _u8p, _u8p, _u8pp]),
            "gf_vect_dot_prod": (v, [i, i, _u8p, _u8pp, _u8p]),
            "gf_vect_dot_prod_base": (v, [i, i, _u8p, _u8pp, _u8p]),
            "gf_vect_mad": (v, [i, i, i, _u8p, _u8p, _u8p]),
            "gf_vect_mad_base": (v, [i, i, i, _u8p, _u8p, _u8p]),
            "gf_vect_mul": (i, [i, _u8p, ctypes.c_void_p, ctypes.c_void_p]),
            "gf_vect_mul_base": (i, [i, _u8p, _u8p, _u8p]),
            "isal_get_version": (ctypes.c_uint, []),
            "isal_get_version_str": (ctypes.c_char_p, []),
            "isal_hip_batch_create": (i, [ctypes.POINTER(ctypes.c_void_p), i, i, i, _u8p, i, _u8pp, _u8pp]),
            "isal_hip_batch_set_tables": (i, [ctypes.c_void_p, _u8p]),
            "isal_hip_batch_encode": (i, [ctypes.c_void_p, ctypes.c_void_p]),
            "isal_hip_batch_update": (i, [ctypes.c_void_p, i, ctypes.c_void_p]),
            "isal_hip_batch_destroy": (i, [ctypes.c_void_p]),
            "isal_hip_batch_encode_crc": (i, [ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p]),
            "isal_hip_batch_crc": (i, [ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p]),
            "isal_hip_batch_crc64": (i, [ctypes.c_void_p, i, ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_void_p]),
            "isal_hip_batch_encode_crc64": (i, [ctypes.c_void_p, i, ctypes.c_ulonglong, ctypes.c_void_p,
                                                ctypes.c_void_p]),
            "isal_hip_decode_matrix": (i, [i, i, _u8p, i, _u8p, _u8p, _u8p]),
            "isal_hip_repair_create": (i, [ctypes.POINTER(ctypes.c_void_p), i, i, i, _u8p, i, i, _u8p, _u8pp,
                                           ctypes.POINTER(ctypes.c_int)]),
            "isal_hip_repair_create_ragged": (i, [ctypes.POINTER(ctypes.c_void_p), i, i, _u8p, i,
                                                  ctypes.POINTER(ctypes.c_int), i, _u8p, _u8p, _u8pp,
                                                  ctypes.POINTER(ctypes.c_int)]),
            "isal_hip_repair_run": (i, [ctypes.c_void_p, ctypes.c_void_p]),
            "isal_hip_repair_npatterns": (i, [ctypes.c_void_p]),
            "isal_hip_repair_destroy": (i, [ctypes.c_void_p]),
            "isal_hip_overwrite_create": (i, [ctypes.POINTER(ctypes.c_void_p), i, i, i, _u8p, i, i, _u8p, _u8pp, _u8pp,
                                              _u8pp, ctypes.POINTER(ctypes.c_int)]),
            "isal_hip_overwrite_create_ragged": (i, [ctypes.POINTER(ctypes.c_void_p), i, i, _u8p, i,
                                                     ctypes.POINTER(ctypes.c_int), i, ctypes.POINTER(ctypes.c_int),
                                                     _u8p, _u8pp, _u8pp, _u8pp, ctypes.POINTER(ctypes.c_int)]),
            "isal_hip_overwrite_run": (i, [ctypes.c_void_p, i, ctypes.c_void_p]),
            "isal_hip_overwrite_destroy": (i, [ctypes.c_void_p]),
            "isal_hip_scrub_ambiguity": (i, [i, i, _u8p, ctypes.POINTER(ctypes.c_int)]),
            "isal_hip_locate_syndrome": (i, [i, i, _u8p, _u8p]),
            "isal_hip_scrub_create": (i, [ctypes.POINTER(ctypes.c_void_p), i, i, i, _u8p, i, _u8pp, _u8pp,
                                          ctypes.POINTER(ctypes.c_int)]),
            "isal_hip_scrub_create_ragged": (i, [ctypes.POINTER(ctypes.c_void_p), i, i, _u8p, i,
                                                 ctypes.POINTER(ctypes.c_int), _u8pp, _u8pp,
                                                 ctypes.POINTER(ctypes.c_int)]),
            "isal_hip_scrub_run": (i, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
            "isal_hip_scrub_destroy": (i, [ctypes.c_void_p]),
            "isal_hip_ragged_items": (ctypes.c_longlong, [i, ctypes.POINTER(ctypes.c_int), i,
                                                          ctypes.POINTER(ctypes.c_uint)]),
            "isal_hip_ragged_create": (i, [ctypes.POINTER(ctypes.c_void_p), i, i, _u8p, i, ctypes.POINTER(ctypes.c_int),
                                           _u8pp, _u8pp, ctypes.POINTER(ctypes.c_int)]),
            "isal_hip_ragged_encode": (i, [ctypes.c_void_p, ctypes.c_void_p]),
            "isal_hip_ragged_check": (i, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
            "isal_hip_ragged_crc": (i, [ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p]),
            "isal_hip_ragged_encode_crc": (i, [ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p]),
            "isal_hip_ragged_crc64": (i, [ctypes.c_void_p, i, ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_void_p]),
            "isal_hip_ragged_encode_crc64": (i, [ctypes.c_void_p, i, ctypes.c_ulonglong, ctypes.c_void_p,
                                                 ctypes.c_void_p]),
            "isal_hip_ragged_destroy": (i, [ctypes.c_void_p]),
            "isal_hip_batch_sector_crc": (i, [ctypes.c_void_p, i, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p]),
            "isal_hip_batch_sector_crc64": (i, [ctypes.c_void_p, i, i, ctypes.c_ulonglong, ctypes.c_void_p,
                                                ctypes.c_void_p]),
            "isal_hip_ragged_sector_offsets": (ctypes.c_longlong, [i, ctypes.POINTER(ctypes.c_int), i,
                                                                   ctypes.POINTER(ctypes.c_longlong)]),
            "isal_hip_ragged_sector_crc": (i, [ctypes.c_void_p, i, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p]),
            "isal_hip_ragged_sector_crc64": (i, [ctypes.c_void_p, i, i, ctypes.c_ulonglong, ctypes.c_void_p,
                                                 ctypes.c_void_p]),
            "isal_hip_batch_sector_t10dif": (i, [ctypes.c_void_p, i, ctypes.c_ushort, ctypes.c_void_p, ctypes.c_void_p]),
            "isal_hip_ragged_sector_t10dif": (i, [ctypes.c_void_p, i, ctypes.c_ushort, ctypes.c_void_p, ctypes.c_void_p]),
            "isal_hip_batch_dif_generate": (i, [ctypes.c_void_p, i, ctypes.POINTER(_Dif), ctypes.c_void_p, ctypes.c_void_p]),
            "isal_hip_ragged_dif_generate": (i, [ctypes.c_void_p, i, ctypes.POINTER(_Dif), ctypes.c_void_p, ctypes.c_void_p]),
            "isal_hip_batch_dif_verify": (i, [ctypes.c_void_p, i, ctypes.POINTER(_Dif), ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p]),
            "isal_hip_ragged_dif_verify": (i, [ctypes.c_void_p, i, ctypes.POINTER(_Dif), ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p]),
            "isal_hip_pipe_create": (i, [ctypes.POINTER(ctypes.c_void_p), i, i, i, _u8p, i, i]),
            "isal_hip_pipe_submit": (i, [ctypes.c_void_p, _u8pp, _u8pp]),
            "isal_hip_pipe_flush": (i, [ctypes.c_void_p]),
            "isal_hip_pipe_destroy": (i, [ctypes.c_void_p]),
            "isal_hip_kernel_launches": (ctypes.c_ulonglong, []),
            "isal_hip_cpu_calls": (ctypes.c_ulonglong, []),
            "isal_hip_multi_create": (i, [ctypes.POINTER(ctypes.c_void_p), i, i, i, i, _u8p, i]),
            "isal_hip_multi_ndev": (i, [ctypes.c_void_p]),
            "isal_hip_multi_encode": (i, [ctypes.c_void_p, ctypes.c_longlong, _u8pp, _u8pp]),
            "isal_hip_multi_destroy": (i, [ctypes.c_void_p]),
            "isal_hip_multi_partition": (None, [ctypes.c_longlong, i, i, ctypes.POINTER(ctypes.c_longlong),
                                                ctypes.POINTER(ctypes.c_longlong)]),
            "isal_hip_multi_numa_node": (i, [ctypes.c_void_p, i]),
            "isal_hip_multi_worker_cpus": (i, [ctypes.c_void_p, i]),
            "isal_hip_pci_numa_node": (i, [ctypes.c_char_p, ctypes.c_char_p]),
            "isal_hip_numa_node_cpus": (i, [ctypes.c_char_p, i, ctypes.POINTER(ctypes.c_int), i]),
            "isal_hip_fallbacks": (ctypes.c_ulonglong, []),
            "isal_hip_config_reload": (None, []),
            "isal_hip_max_rows_per_pass": (i, []),
            "isal_hip_target": (ctypes.c_char_p, []),
            "isal_hip_route_device": (i, [i, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), i,
                                          ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
            "isal_hip_contexts_created": (ctypes.c_ulonglong, []),
            "isal_hip_slow_waits": (ctypes.c_ulonglong, []),
            "isal_hip_selftest_kernels": (i, [ctypes.POINTER(ctypes.c_int)]),
            "crc32_iscsi": (ctypes.c_uint, [ctypes.c_void_p, i, ctypes.c_uint]),
            "crc32_iscsi_base": (ctypes.c_uint, [ctypes.c_void_p, i, ctypes.c_uint]),
        }
        for v in CRC64_VARIANTS:
            for suffix in ("", "_base"):
                sig[f"crc64_{v}{suffix}"] = (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64])
        for name, (res, args) in sig.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


# ---------------------------------------------------------------------------
# buffer plumbing
# ---------------------------------------------------------------------------

# T10 protection information (isal_hip.h ISAL_HIP_DIF_*)
DIF_TYPE1, DIF_TYPE3 = 1, 3
DIF_CHECK_GUARD, DIF_CHECK_APP, DIF_CHECK_REF, DIF_CHECK_ALL = 1, 2, 4, 7
DIF_CLEAN = 0xFFFFFFFF


class _Dif(ctypes.Structure):
    """isal_hip_dif"""
    _fields_ = [("type", ctypes.c_int), ("flags", ctypes.c_uint), ("app_tag", ctypes.c_ushort),
                ("seed", ctypes.c_ushort), ("ref0", ctypes.c_void_p)]


def _sector_t10dif(kind: str, h, sector: int, seed: int, crc, stream: int) -> None:
    name = f"isal_hip_{kind}_sector_t10dif"
    rc = getattr(lib(), name)(h, sector, seed & 0xFFFF, ctypes.c_void_p(addr(crc)), ctypes.c_void_p(stream))
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc})")


def _dif(kind: str, what: str, h, sector: int, pi, bad, type: int, flags: int, app_tag: int, seed: int, ref0,
         stream: int) -> None:
    d = _Dif(type, flags, app_tag & 0xFFFF, seed & 0xFFFF, None if ref0 is None else addr(ref0))
    name = f"isal_hip_{kind}_dif_{what}"
    tail = (ctypes.c_void_p(addr(bad)),) if what == "verify" else ()
    rc = getattr(lib(), name)(h, sector, ctypes.byref(d), ctypes.c_void_p(addr(pi)), *tail, ctypes.c_void_p(stream))
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc})")


def addr(buf) -> int:
    """Address of a byte buffer: numpy array, torch tensor, ctypes buffer or int."""
    if isinstance(buf, int):
        return buf
    if isinstance(buf, np.ndarray):
        if not buf.flags["C_CONTIGUOUS"]:
            raise ValueError("buffer must be C-contiguous")
        return buf.ctypes.data
    if hasattr(buf, "data_ptr"):  # torch.Tensor
        if not buf.is_contiguous():
            raise ValueError("tensor must be contiguous")
        return int(buf.data_ptr())
    if isinstance(buf, (ctypes.Array, bytearray)):
        return ctypes.addressof(ctypes.c_char.from_buffer(buf))
    raise TypeError(f"unsupported buffer type {type(buf)!r}")


def _p(buf) -> _u8p:
    return ctypes.cast(ctypes.c_void_p(addr(buf)), _u8p)


def _pp(bufs: Sequence) -> ctypes.Array:
    arr = (_u8p * max(1, len(bufs)))()
    for j, b in enumerate(bufs):
        arr[j] = _p(b)
    return arr


def _u8(a) -> np.ndarray:
    a = np.ascontiguousarray(np.frombuffer(bytes(a), dtype=np.uint8) if isinstance(a, (bytes, bytearray)) else a,
                             dtype=np.uint8)
    return a


# ---------------------------------------------------------------------------
# host-side GF math (reference ec_base.c:37-280 semantics)
# ---------------------------------------------------------------------------

def gf_mul(a: int, b: int) -> int:
    return int(lib().gf_mul(a & 0xFF, b & 0xFF))


def gf_inv(a: int) -> int:
    return int(lib().gf_inv(a & 0xFF))


def gf_gen_rs_matrix(m: int, k: int) -> np.ndarray:
    a = np.zeros(m * k, dtype=np.uint8)
    lib().gf_gen_rs_matrix(_p(a), m, k)
    return a


def gf_gen_cauchy1_matrix(m: int, k: int) -> np.ndarray:
    a = np.zeros(m * k, dtype=np.uint8)
    lib().gf_gen_cauchy1_matrix(_p(a), m, k)
    return a


def gf_invert_matrix(mat, n: int):
    """Returns (ret, inverse, destroyed_input) like the C call (input is copied first)."""
    inp = _u8(mat).copy()
    out = np.zeros(n * n, dtype=np.uint8)
    ret = lib().gf_invert_matrix(_p(inp), _p(out), n)
    return int(ret), out, inp


def gf_vect_mul_init(c: int) -> np.ndarray:
    t = np.zeros(32, dtype=np.uint8)
    lib().gf_vect_mul_init(c & 0xFF, _p(t))
    return t


def ec_init_tables(k: int, rows: int, a) -> np.ndarray:
    a = _u8(a)
    t = np.zeros(max(1, 32 * k * rows), dtype=np.uint8)
    lib().ec_init_tables(k, rows, _p(a), _p(t))
    return t


# ---------------------------------------------------------------------------
# data path (GPU) — same argument order as the C API
# ---------------------------------------------------------------------------

def ec_encode_data(len_: int, k: int, rows: int, gftbls, data: Sequence, coding: Sequence) -> None:
    lib().ec_encode_data(len_, k, rows, _p(gftbls), _pp(data), _pp(coding))


def ec_encode_data_base(len_: int, k: int, rows: int, gftbls, data: Sequence, coding: Sequence) -> None:
    lib().ec_encode_data_base(len_, k, rows, _p(gftbls), _pp(data), _pp(coding))


def ec_encode_data_update(len_: int, k: int, rows: int, vec_i: int, gftbls, data, coding: Sequence) -> None:
    lib().ec_encode_data_update(len_, k, rows, vec_i, _p(gftbls), _p(data), _pp(coding))


def ec_encode_data_update_base(len_: int, k: int, rows: int, vec_i: int, gftbls, data, coding: Sequence) -> None:
    lib().ec_encode_data_update_base(len_, k, rows, vec_i, _p(gftbls), _p(data), _pp(coding))


def gf_vect_dot_prod(len_: int, vlen: int, gftbls, src: Sequence, dest) -> None:
    lib().gf_vect_dot_prod(len_, vlen, _p(gftbls), _pp(src), _p(dest))


def gf_vect_dot_prod_base(len_: int, vlen: int, gftbls, src: Sequence, dest) -> None:
    lib().gf_vect_dot_prod_base(len_, vlen, _p(gftbls), _pp(src), _p(dest))


def gf_vect_mad(len_: int, vec: int, vec_i: int, gftbls, src, dest) -> None:
    lib().gf_vect_mad(len_, vec, vec_i, _p(gftbls), _p(src), _p(dest))


def gf_vect_mad_base(len_: int, vec: int, vec_i: int, gftbls, src, dest) -> None:
    lib().gf_vect_mad_base(len_, vec, vec_i, _p(gftbls), _p(src), _p(dest))


def gf_vect_mul(len_: int, gftbl, src, dest) -> int:
    return int(lib().gf_vect_mul(len_, _p(gftbl), ctypes.c_void_p(addr(src)), ctypes.c_void_p(addr(dest))))


def gf_vect_mul_base(len_: int, gftbl, src, dest) -> int:
    return int(lib().gf_vect_mul_base(len_, _p(gftbl), _p(src), _p(dest)))


# ---------------------------------------------------------------------------
# batched extension (include/isal_hip.h)
# ---------------------------------------------------------------------------

class Batch:
    """nstripes stripes sharing one coefficient matrix; shards are device buffers.

    data[s*k + j] / coding[s*rows + l] are addresses (or tensors) of stripe s.
    encode()/update() only enqueue on `stream` (a hipStream_t as int; 0 = default).
    """

    def __init__(self, len_: int, k: int, rows: int, gftbls, nstripes: int,
                 data: Sequence, coding: Sequence):
        self.len, self.k, self.rows, self.nstripes = len_, k, rows, nstripes
        if len(data) != nstripes * k or len(coding) != nstripes * rows:
            raise ValueError("pointer lists must hold nstripes*k and nstripes*rows entries")
        h = ctypes.c_void_p()
        rc = lib().isal_hip_batch_create(ctypes.byref(h), len_, k, rows, _p(gftbls), nstripes,
                                         _pp(data), _pp(coding))
        if rc != 0:
            raise RuntimeError(f"isal_hip_batch_create failed ({rc})")
        self._h = h

    def set_tables(self, gftbls) -> None:
        rc = lib().isal_hip_batch_set_tables(self._h, _p(gftbls))
        if rc != 0:
            raise RuntimeError(f"isal_hip_batch_set_tables failed ({rc})")

    def encode(self, stream: int = 0) -> None:
        rc = lib().isal_hip_batch_encode(self._h, ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"isal_hip_batch_encode failed ({rc})")

    def update(self, vec_i: int, stream: int = 0) -> None:
        rc = lib().isal_hip_batch_update(self._h, vec_i, ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"isal_hip_batch_update failed ({rc})")

    def check(self, bad, stream: int = 0) -> None:
        """Verify every stripe (isal_hip_batch_check): the DEVICE buffer bad
        (nstripes uint64) gets ~0 for a consistent stripe, else its first
        mismatch as column << 8 | row."""
        rc = lib().isal_hip_batch_check(self._h, ctypes.c_void_p(addr(bad)), ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"isal_hip_batch_check failed ({rc})")

    def encode_crc(self, init: int, crc, stream: int = 0) -> None:
        """encode() plus crc32_iscsi(shard, len, init) of every source and parity
        shard into the DEVICE buffer crc (nstripes*(k+rows) uint32, stripe-major,
        sources then parity)."""
        rc = lib().isal_hip_batch_encode_crc(self._h, init & 0xFFFFFFFF, ctypes.c_void_p(addr(crc)),
                                             ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"isal_hip_batch_encode_crc failed ({rc})")

    def crc(self, init: int, crc, stream: int = 0) -> None:
        """crc32_iscsi of every shard (no encoding), layout as encode_crc()."""
        rc = lib().isal_hip_batch_crc(self._h, init & 0xFFFFFFFF, ctypes.c_void_p(addr(crc)),
                                      ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"isal_hip_batch_crc failed ({rc})")

    def crc64(self, variant: int, init: int, crc, stream: int = 0) -> None:
        """crc64_<variant>(init, shard, len) of every shard into the DEVICE buffer
        crc (nstripes*(k+rows) 64-bit words, layout as encode_crc()); variant =
        CRC64_VARIANTS.index(name), the order of the reference's crc64.h."""
        rc = lib().isal_hip_batch_crc64(self._h, variant, init & 0xFFFFFFFFFFFFFFFF,
                                        ctypes.c_void_p(addr(crc)), ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"isal_hip_batch_crc64 failed ({rc})")

    def encode_crc64(self, variant: int, init: int, crc, stream: int = 0) -> None:
        """encode() plus crc64_<variant>(init, shard, len) of every source and
        parity shard, layout as crc64(); one pass over HBM where the shape allows."""
        rc = lib().isal_hip_batch_encode_crc64(self._h, variant, init & 0xFFFFFFFFFFFFFFFF,
                                               ctypes.c_void_p(addr(crc)), ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"isal_hip_batch_encode_crc64 failed ({rc})")

    def sector_crc(self, sector: int, init: int, crc, stream: int = 0) -> None:
        """crc32_iscsi(sector bytes, n, init) of every `sector` bytes (512, 1024,
        2048 or 4096; the last sector of a shard may be short) of every shard
        into the DEVICE buffer crc: nstripes*(k+rows)*ns uint32 with ns =
        ceil(len / sector), word (s*(k+rows) + j)*ns + i for sector i of shard
        j of stripe s. One launch (isal_hip_batch_sector_crc)."""
        rc = lib().isal_hip_batch_sector_crc(self._h, sector, init & 0xFFFFFFFF, ctypes.c_void_p(addr(crc)),
                                             ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"isal_hip_batch_sector_crc failed ({rc})")

    def sector_crc64(self, variant: int, sector: int, init: int, crc, stream: int = 0) -> None:
        """crc64_<variant>(init, sector bytes, n) of every sector, 64-bit words
        laid out as sector_crc()'s; variant as for crc64()."""
        rc = lib().isal_hip_batch_sector_crc64(self._h, variant, sector, init & 0xFFFFFFFFFFFFFFFF,
                                               ctypes.c_void_p(addr(crc)), ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"isal_hip_batch_sector_crc64 failed ({rc})")

    def sector_t10dif(self, sector: int, seed: int, crc, stream: int = 0) -> None:
        """crc16_t10dif(seed, sector bytes, n), the T10 / NVMe 16-bit guard, of
        every sector into the DEVICE buffer crc: uint16 words laid out as
        sector_crc()'s. One launch (isal_hip_batch_sector_t10dif)."""
        _sector_t10dif("batch", self._h, sector, seed, crc, stream)

    def dif_generate(self, sector: int, pi, type: int = DIF_TYPE1, app_tag: int = 0, seed: int = 0, ref0=None,
                     stream: int = 0) -> None:
        """The 8-byte T10 tuple (guard, application tag, reference tag, each
        big-endian) of every sector into the DEVICE buffer pi (8-byte aligned,
        8 bytes per sector in sector_crc()'s order). ref0: DEVICE uint32 per
        shard (None: 0); DIF_TYPE1 adds the sector's index, DIF_TYPE3 does
        not. One launch (isal_hip_batch_dif_generate)."""
        _dif("batch", "generate", self._h, sector, pi, None, type, 0, app_tag, seed, ref0, stream)

    def dif_verify(self, sector: int, pi, bad, type: int = DIF_TYPE1, flags: int = DIF_CHECK_ALL, app_tag: int = 0,
                   seed: int = 0, ref0=None, stream: int = 0) -> None:
        """Compares every sector with its stored tuple in pi, in the fields
        `flags` names: the DEVICE uint32 bad[s*(k+rows) + j] becomes DIF_CLEAN,
        or (i << 3) | kinds for the first failing sector i of the shard. A
        fill of bad and one launch (isal_hip_batch_dif_verify)."""
        _dif("batch", "verify", self._h, sector, pi, bad, type, flags, app_tag, seed, ref0, stream)

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().isal_hip_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


ESINGULAR = -5  # ISAL_HIP_ESINGULAR


def decode_matrix(a, k: int, errs: Sequence[int]):
    """isal_hip_decode_matrix (host arithmetic, no GPU): (ret, c, survivors) for
    the m x k encode matrix a and the erased shard indices errs. c is
    len(errs) x k, row i rebuilding shard errs[i] from the survivors (the first
    k non-erased indices); ret is 0, ESINGULAR or -1 (bad arguments)."""
    a = _u8(a)
    m = a.size // k
    e = np.array(list(errs), dtype=np.uint8)
    c = np.zeros(max(1, e.size * k), dtype=np.uint8)
    surv = np.zeros(max(1, k), dtype=np.uint8)
    ret = lib().isal_hip_decode_matrix(k, m, _p(a), int(e.size), _p(e), _p(c), _p(surv))
    return int(ret), c[:e.size * k], [int(x) for x in surv[:k]]


class Repair:
    """nstripes stripes of one geometry, each with its own nerrs erased shards,
    rebuilt by one launch per pass (include/isal_hip.h repair batch).

    shards[s*m + i] is the address (or tensor) of shard i of stripe s, every
    one a 16-byte aligned device buffer; errs[s*nerrs + i] the erased indices
    of stripe s. run() only enqueues on `stream` and may be repeated."""

    def __init__(self, len_: int, k: int, m: int, a, nerrs: int, nstripes: int, errs: Sequence[int],
                 shards: Sequence):
        if len(errs) != nstripes * nerrs or len(shards) != nstripes * m:
            raise ValueError("errs must hold nstripes*nerrs entries and shards nstripes*m")
        e = np.array(list(errs), dtype=np.uint8)
        h, bad = ctypes.c_void_p(), ctypes.c_int(-1)
        rc = lib().isal_hip_repair_create(ctypes.byref(h), len_, k, m, _p(_u8(a)), nerrs, nstripes, _p(e),
                                          _pp(shards), ctypes.byref(bad))
        if rc != 0:
            raise RuntimeError(f"isal_hip_repair_create failed ({rc}, stripe {bad.value})")
        self.len, self.k, self.m, self.nerrs, self.nstripes = len_, k, m, nerrs, nstripes
        self._h = h

    @classmethod
    def ragged(cls, k: int, m: int, a, lens: Sequence[int], errs: Sequence[Sequence[int]],
               shards: Sequence) -> "Repair":
        """isal_hip_repair_create_ragged: stripe s has shards of lens[s] bytes and
        lost the shards errs[s] (any number from none to m - k of them, its own
        count); shards as for Repair()."""
        nstripes = len(lens)
        if len(errs) != nstripes or len(shards) != nstripes * m:
            raise ValueError("errs must hold one index sequence per stripe and shards nstripes*m")
        ln = np.ascontiguousarray(np.array(list(lens), dtype=np.int64).astype(np.intc))
        max_errs = max([len(e) for e in errs], default=0)
        n = np.array([len(e) for e in errs], dtype=np.uint8)
        e = np.zeros(max(1, nstripes * max_errs), dtype=np.uint8)
        for s, row in enumerate(errs):
            e[s * max_errs:s * max_errs + len(row)] = list(row)
        h, bad = ctypes.c_void_p(), ctypes.c_int(-1)
        rc = lib().isal_hip_repair_create_ragged(ctypes.byref(h), k, m, _p(_u8(a)), nstripes,
                                                 ln.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), max_errs, _p(n),
                                                 _p(e), _pp(shards), ctypes.byref(bad))
        if rc != 0:
            raise RuntimeError(f"isal_hip_repair_create_ragged failed ({rc}, stripe {bad.value})")
        self = cls.__new__(cls)
        self.len, self.k, self.m, self.nerrs, self.nstripes = None, k, m, max_errs, nstripes
        self.lens = [int(x) for x in ln]
        self._h = h
        return self

    def run(self, stream: int = 0) -> None:
        rc = lib().isal_hip_repair_run(self._h, ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"isal_hip_repair_run failed ({rc})")

    def npatterns(self) -> int:
        """Distinct erasure patterns among the stripes."""
        return int(lib().isal_hip_repair_npatterns(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().isal_hip_repair_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


OVERWRITE_COMMIT = 1  # ISAL_HIP_OVERWRITE_COMMIT


class Overwrite:
    """nstripes encoded stripes of one geometry, each with its own nw rewritten
    data shards, whose deltas are folded into the parity by one launch per pass
    (include/isal_hip.h overwrite batch).

    idx[s*nw + i] is the data-shard index slot i of stripe s rewrites;
    old_data / new_data[s*nw + i] and coding[s*rows + l] are addresses (or
    tensors) of 16-byte aligned device buffers. run() only enqueues on
    `stream`; commit=True also stores new over old in the same pass."""

    def __init__(self, len_: int, k: int, rows: int, gftbls, nw: int, nstripes: int, idx: Sequence[int],
                 old_data: Sequence, new_data: Sequence, coding: Sequence):
        if (len(idx) != nstripes * nw or len(old_data) != nstripes * nw or len(new_data) != nstripes * nw
                or len(coding) != nstripes * rows):
            raise ValueError("idx, old_data and new_data must hold nstripes*nw entries and coding nstripes*rows")
        ix = np.array(list(idx), dtype=np.uint8)
        h, bad = ctypes.c_void_p(), ctypes.c_int(-1)
        rc = lib().isal_hip_overwrite_create(ctypes.byref(h), len_, k, rows, _p(gftbls), nw, nstripes, _p(ix),
                                             _pp(old_data), _pp(new_data), _pp(coding), ctypes.byref(bad))
        if rc != 0:
            raise RuntimeError(f"isal_hip_overwrite_create failed ({rc}, stripe {bad.value})")
        self.len, self.k, self.rows, self.nw, self.nstripes = len_, k, rows, nw, nstripes
        self._h = h

    @classmethod
    def ragged(cls, k: int, rows: int, gftbls, lens: Sequence[int], idx: Sequence[Sequence[int]],
               old_data: Sequence[Sequence], new_data: Sequence[Sequence], coding: Sequence, *,
               max_nw: Optional[int] = None, pad_idx: int = 0, pad_ptr=0) -> "Overwrite":
        """isal_hip_overwrite_create_ragged: stripe s rewrites lens[s] bytes of
        the data shards idx[s] (any number from none to k of them, its own
        count), from old_data[s][i] to new_data[s][i]; coding as for
        Overwrite(). The rows are padded to the stride max_nw (default: the
        longest idx[s], at least 1) with pad_idx and pad_ptr, which the library
        ignores. One launch per pass serves every mix of lengths and counts."""
        nstripes = len(lens)
        if (len(idx) != nstripes or len(old_data) != nstripes or len(new_data) != nstripes
                or len(coding) != nstripes * rows):
            raise ValueError("idx, old_data and new_data must hold one sequence per stripe and coding nstripes*rows")
        if any(len(old_data[s]) != len(idx[s]) or len(new_data[s]) != len(idx[s]) for s in range(nstripes)):
            raise ValueError("old_data[s] and new_data[s] must hold one entry per index of idx[s]")
        if max_nw is None:
            max_nw = max([len(x) for x in idx] + [1])
        if any(len(x) > max_nw for x in idx):
            raise ValueError("a stripe has more than max_nw slots")
        ln = np.ascontiguousarray(np.array(list(lens), dtype=np.int64).astype(np.intc))
        n = np.ascontiguousarray(np.array([len(x) for x in idx], dtype=np.intc))
        ix = np.full(max(1, nstripes * max_nw), pad_idx, dtype=np.uint8)
        old, new = [pad_ptr] * (nstripes * max_nw), [pad_ptr] * (nstripes * max_nw)
        for s, row in enumerate(idx):
            ix[s * max_nw:s * max_nw + len(row)] = list(row)
            old[s * max_nw:s * max_nw + len(row)] = list(old_data[s])
            new[s * max_nw:s * max_nw + len(row)] = list(new_data[s])
        h, bad = ctypes.c_void_p(), ctypes.c_int(-1)
        ip = ctypes.POINTER(ctypes.c_int)
        rc = lib().isal_hip_overwrite_create_ragged(ctypes.byref(h), k, rows, _p(gftbls), nstripes,
                                                    ln.ctypes.data_as(ip), max_nw, n.ctypes.data_as(ip), _p(ix),
                                                    _pp(old), _pp(new), _pp(coding), ctypes.byref(bad))
        if rc != 0:
            raise RuntimeError(f"isal_hip_overwrite_create_ragged failed ({rc}, stripe {bad.value})")
        self = cls.__new__(cls)
        self.len, self.k, self.rows, self.nw, self.nstripes = None, k, rows, max_nw, nstripes
        self.lens, self.nws = [int(x) for x in ln], [int(x) for x in n]
        self._h = h
        return self

    def run(self, commit: bool = False, stream: int = 0) -> None:
        rc = lib().isal_hip_overwrite_run(self._h, OVERWRITE_COMMIT if commit else 0, ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"isal_hip_overwrite_run failed ({rc})")

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().isal_hip_overwrite_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SCRUB_CLEAN = 0xFFFFFFFF  # ISAL_HIP_SCRUB_CLEAN
SCRUB_MULTI = 0xFFFFFFFE  # ISAL_HIP_SCRUB_MULTI


def scrub_ambiguity(k: int, rows: int, gftbls):
    """isal_hip_scrub_ambiguity (host arithmetic, no GPU): None when no two of
    the k + rows columns of [C | I] are proportional and none is zero, else
    the first offending pair (a, b) of shard indices ((j, j): a zero column)."""
    g = _u8(gftbls)
    if k < 1 or rows < 1 or g.size < 32 * k * rows:
        raise ValueError("gftbls must hold 32*k*rows bytes")
    pair = (ctypes.c_int * 2)(-1, -1)
    rc = lib().isal_hip_scrub_ambiguity(k, rows, _p(g), pair)
    if rc == 0:
        return None
    if rc != ESINGULAR:
        raise ValueError(f"isal_hip_scrub_ambiguity failed ({rc})")
    return int(pair[0]), int(pair[1])


def locate_syndrome(k: int, rows: int, gftbls, syndrome) -> int:
    """isal_hip_locate_syndrome (host arithmetic, no GPU): the shard index the
    rows-byte syndrome (stored ^ recomputed parity of one byte column) names,
    SCRUB_MULTI when it names nothing, SCRUB_CLEAN when it is all zero."""
    g, e = _u8(gftbls), _u8(syndrome)
    if k < 1 or rows < 1 or k + rows > 256 or g.size < 32 * k * rows or e.size != rows:
        raise ValueError("gftbls must hold 32*k*rows bytes and syndrome rows bytes, k + rows <= 256")
    return int(lib().isal_hip_locate_syndrome(k, rows, _p(g), _p(e))) & 0xFFFFFFFF


class Scrub:
    """nstripes encoded stripes of one geometry, verified by one launch that
    names, for every inconsistent stripe, the one shard that explains its
    mismatches (include/isal_hip.h scrub batch).

    data[s*k + j] / coding[s*rows + l] are addresses (or tensors) of 16-byte
    aligned device buffers, as for Batch. run() only enqueues on `stream`:
    the DEVICE buffer verdict (nstripes uint32) gets SCRUB_CLEAN, a shard index
    (j < k: data shard j, k + l: parity row l) or SCRUB_MULTI per stripe. An
    index is the only single-shard explanation, not a proof: confirm it with
    fragment checksums where they exist, then rebuild with Repair(nerrs=1)."""

    def __init__(self, len_: int, k: int, rows: int, gftbls, nstripes: int, data: Sequence, coding: Sequence):
        if len(data) != nstripes * k or len(coding) != nstripes * rows:
            raise ValueError("pointer lists must hold nstripes*k and nstripes*rows entries")
        h, bad = ctypes.c_void_p(), ctypes.c_int(-1)
        rc = lib().isal_hip_scrub_create(ctypes.byref(h), len_, k, rows, _p(gftbls), nstripes, _pp(data),
                                         _pp(coding), ctypes.byref(bad))
        if rc != 0:
            raise RuntimeError(f"isal_hip_scrub_create failed ({rc}, stripe {bad.value})")
        self.len, self.k, self.rows, self.nstripes = len_, k, rows, nstripes
        self._h = h

    @classmethod
    def ragged(cls, k: int, rows: int, gftbls, lens: Sequence[int], data: Sequence, coding: Sequence) -> "Scrub":
        """isal_hip_scrub_create_ragged: stripe s has shards of lens[s] bytes
        (any length >= 0; a stripe of length 0 reads SCRUB_CLEAN); data and
        coding as for Scrub(). One launch names the shard of every stripe."""
        nstripes = len(lens)
        if len(data) != nstripes * k or len(coding) != nstripes * rows:
            raise ValueError("pointer lists must hold len(lens)*k and len(lens)*rows entries")
        ln = np.ascontiguousarray(np.array(list(lens), dtype=np.int64).astype(np.intc))
        h, bad = ctypes.c_void_p(), ctypes.c_int(-1)
        rc = lib().isal_hip_scrub_create_ragged(ctypes.byref(h), k, rows, _p(gftbls), nstripes,
                                                ln.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _pp(data),
                                                _pp(coding), ctypes.byref(bad))
        if rc != 0:
            raise RuntimeError(f"isal_hip_scrub_create_ragged failed ({rc}, stripe {bad.value})")
        self = cls.__new__(cls)
        self.len, self.k, self.rows, self.nstripes = None, k, rows, nstripes
        self.lens = [int(x) for x in ln]
        self._h = h
        return self

    def run(self, verdict, stream: int = 0) -> None:
        rc = lib().isal_hip_scrub_run(self._h, ctypes.c_void_p(addr(verdict)), ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"isal_hip_scrub_run failed ({rc})")

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().isal_hip_scrub_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ragged_items(lens: Sequence[int], tile: int) -> np.ndarray:
    """isal_hip_ragged_items (host arithmetic, no GPU): the work items of a
    ragged launch over shards of lens[s] bytes in tiles of `tile` bytes, an
    (n, 2) uint32 array of {stripe, tile index} rows."""
    ln = np.array(list(lens), dtype=np.int32)
    lp = ln.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    n = int(lib().isal_hip_ragged_items(int(ln.size), lp, tile, None))
    if n < 0:
        raise ValueError("lens must be non-empty and non-negative, tile positive")
    items = np.zeros((n, 2), dtype=np.uint32)
    if n:
        lib().isal_hip_ragged_items(int(ln.size), lp, tile, items.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)))
    return items


def ragged_sector_offsets(lens: Sequence[int], sector: int) -> tuple[np.ndarray, int]:
    """isal_hip_ragged_sector_offsets (host arithmetic, no GPU): first[s], the
    number of sectors of one shard of the stripes before s (int64), and the
    total over all stripes; Ragged.sector_crc writes (k+rows) * total words."""
    ln = np.array(list(lens), dtype=np.int32)
    first = np.zeros(ln.size, dtype=np.int64)
    total = int(lib().isal_hip_ragged_sector_offsets(int(ln.size), ln.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                                     sector, first.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))))
    if total < 0:
        raise ValueError("lens must be non-empty and non-negative, sector one of 512, 1024, 2048, 4096")
    return first, total


class Ragged:
    """len(lens) stripes of one geometry, stripe s with shards of lens[s]
    bytes, encoded or checked by one launch per pass (include/isal_hip.h
    ragged batch).

    data[s*k + j] / coding[s*rows + l] are addresses (or tensors) of 16-byte
    aligned device buffers, as for Batch. encode(), check(), crc(),
    encode_crc(), crc64() and encode_crc64() only enqueue on `stream`; check() fills the DEVICE buffer bad
    (one uint64 per stripe) as Batch.check does, ~0 for a stripe of length 0."""

    def __init__(self, k: int, rows: int, gftbls, lens: Sequence[int], data: Sequence, coding: Sequence):
        ln = np.array(list(lens), dtype=np.int32)
        nstripes = int(ln.size)
        if len(data) != nstripes * k or len(coding) != nstripes * rows:
            raise ValueError("pointer lists must hold len(lens)*k and len(lens)*rows entries")
        h, bad = ctypes.c_void_p(), ctypes.c_int(-1)
        rc = lib().isal_hip_ragged_create(ctypes.byref(h), k, rows, _p(gftbls), nstripes,
                                          ln.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _pp(data), _pp(coding),
                                          ctypes.byref(bad))
        if rc != 0:
            raise RuntimeError(f"isal_hip_ragged_create failed ({rc}, stripe {bad.value})")
        self.k, self.rows, self.nstripes, self.lens = k, rows, nstripes, [int(x) for x in ln]
        self._h = h

    def encode(self, stream: int = 0) -> None:
        rc = lib().isal_hip_ragged_encode(self._h, ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"isal_hip_ragged_encode failed ({rc})")

    def check(self, bad, stream: int = 0) -> None:
        rc = lib().isal_hip_ragged_check(self._h, ctypes.c_void_p(addr(bad)), ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"isal_hip_ragged_check failed ({rc})")

    def crc(self, init: int, crc, stream: int = 0) -> None:
        """crc32_iscsi(shard, lens[s], init) of every source and parity shard
        into the DEVICE buffer crc (nstripes*(k+rows) uint32, stripe-major,
        sources then parity, as Batch.crc); a stripe of length 0 yields init."""
        rc = lib().isal_hip_ragged_crc(self._h, init & 0xFFFFFFFF, ctypes.c_void_p(addr(crc)),
                                       ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"isal_hip_ragged_crc failed ({rc})")

    def encode_crc(self, init: int, crc, stream: int = 0) -> None:
        """encode(), then crc() of the sources and the fresh parity on the same
        stream (not fused: the encode's launches plus the checksum's)."""
        rc = lib().isal_hip_ragged_encode_crc(self._h, init & 0xFFFFFFFF, ctypes.c_void_p(addr(crc)),
                                              ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"isal_hip_ragged_encode_crc failed ({rc})")

    def crc64(self, variant: int, init: int, crc, stream: int = 0) -> None:
        """crc64_<variant>(init, shard, lens[s]) of every source and parity
        shard into the DEVICE buffer crc (nstripes*(k+rows) uint64, layout as
        crc()); variant: CRC64_VARIANTS.index(name), as for Batch.crc64. A
        stripe of length 0 yields init."""
        rc = lib().isal_hip_ragged_crc64(self._h, variant, init & 0xFFFFFFFFFFFFFFFF, ctypes.c_void_p(addr(crc)),
                                         ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"isal_hip_ragged_crc64 failed ({rc})")

    def encode_crc64(self, variant: int, init: int, crc, stream: int = 0) -> None:
        """encode(), then crc64() of the sources and the fresh parity on the
        same stream (not fused: the encode's launches plus the checksum's)."""
        rc = lib().isal_hip_ragged_encode_crc64(self._h, variant, init & 0xFFFFFFFFFFFFFFFF,
                                                ctypes.c_void_p(addr(crc)), ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"isal_hip_ragged_encode_crc64 failed ({rc})")

    def sector_crc(self, sector: int, init: int, crc, stream: int = 0) -> None:
        """crc32_iscsi(sector bytes, n, init) of every `sector` bytes (512, 1024,
        2048 or 4096) of every shard into the DEVICE buffer crc ((k+rows) *
        total uint32): with (first, total) = ragged_sector_offsets(lens,
        sector) and ns = ceil(lens[s] / sector), sector i of shard j of stripe
        s is word (k+rows)*first[s] + j*ns + i. One launch
        (isal_hip_ragged_sector_crc); nothing when every length is 0."""
        rc = lib().isal_hip_ragged_sector_crc(self._h, sector, init & 0xFFFFFFFF, ctypes.c_void_p(addr(crc)),
                                              ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"isal_hip_ragged_sector_crc failed ({rc})")

    def sector_crc64(self, variant: int, sector: int, init: int, crc, stream: int = 0) -> None:
        """crc64_<variant>(init, sector bytes, n) of every sector, 64-bit words
        laid out as sector_crc()'s; variant as for crc64()."""
        rc = lib().isal_hip_ragged_sector_crc64(self._h, variant, sector, init & 0xFFFFFFFFFFFFFFFF,
                                                ctypes.c_void_p(addr(crc)), ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"isal_hip_ragged_sector_crc64 failed ({rc})")

    def sector_t10dif(self, sector: int, seed: int, crc, stream: int = 0) -> None:
        """crc16_t10dif(seed, sector bytes, n), the T10 / NVMe 16-bit guard, of
        every sector into the DEVICE buffer crc: uint16 words laid out as
        sector_crc()'s. One launch (isal_hip_ragged_sector_t10dif)."""
        _sector_t10dif("ragged", self._h, sector, seed, crc, stream)

    def dif_generate(self, sector: int, pi, type: int = DIF_TYPE1, app_tag: int = 0, seed: int = 0, ref0=None,
                     stream: int = 0) -> None:
        """The 8-byte T10 tuple (guard, application tag, reference tag, each
        big-endian) of every sector into the DEVICE buffer pi (8-byte aligned,
        8 bytes per sector in sector_crc()'s order). ref0: DEVICE uint32 per
        shard (None: 0); DIF_TYPE1 adds the sector's index, DIF_TYPE3 does
        not. One launch (isal_hip_ragged_dif_generate)."""
        _dif("ragged", "generate", self._h, sector, pi, None, type, 0, app_tag, seed, ref0, stream)

    def dif_verify(self, sector: int, pi, bad, type: int = DIF_TYPE1, flags: int = DIF_CHECK_ALL, app_tag: int = 0,
                   seed: int = 0, ref0=None, stream: int = 0) -> None:
        """Compares every sector with its stored tuple in pi, in the fields
        `flags` names: the DEVICE uint32 bad[s*(k+rows) + j] becomes DIF_CLEAN,
        or (i << 3) | kinds for the first failing sector i of the shard. A
        fill of bad and one launch (isal_hip_ragged_dif_verify)."""
        _dif("ragged", "verify", self._h, sector, pi, bad, type, flags, app_tag, seed, ref0, stream)

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().isal_hip_ragged_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Pipe:
    """Streaming encoder for host-resident stripes (include/isal_hip.h pipeline).

    mode "update": sources folded into parity as they land (ec_encode_data_update);
    mode "encode": one ec_encode_data per stripe once all sources landed.
    Host buffers must stay alive until flush() returns."""

    MODES = {"update": 0, "encode": 1}

    def __init__(self, len_: int, k: int, rows: int, gftbls, depth: int = 3, mode: str = "update"):
        self.len, self.k, self.rows = len_, k, rows
        h = ctypes.c_void_p()
        rc = lib().isal_hip_pipe_create(ctypes.byref(h), len_, k, rows, _p(gftbls), depth,
                                        self.MODES[mode])
        if rc != 0:
            raise RuntimeError(f"isal_hip_pipe_create failed ({rc})")
        self._h = h
        self._keep = []

    def submit(self, data: Sequence, coding: Sequence) -> None:
        d, c = _pp(data), _pp(coding)
        self._keep.append((d, c))  # pointer arrays are read at submit; keep refs cheap anyway
        rc = lib().isal_hip_pipe_submit(self._h, d, c)
        if rc != 0:
            raise RuntimeError(f"isal_hip_pipe_submit failed ({rc})")

    def flush(self) -> None:
        rc = lib().isal_hip_pipe_flush(self._h)
        self._keep.clear()
        if rc != 0:
            raise RuntimeError(f"isal_hip_pipe_flush failed ({rc})")

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().isal_hip_pipe_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Multi:
    """Host-resident stripes encoded on several GPUs of this process
    (include/isal_hip.h multi-device): contiguous stripe ranges per GPU, one
    pipeline and host thread each. ndev = 0: every visible GPU."""

    def __init__(self, len_: int, k: int, rows: int, gftbls, ndev: int = 0, depth: int = 3):
        self.len, self.k, self.rows = len_, k, rows
        h = ctypes.c_void_p()
        rc = lib().isal_hip_multi_create(ctypes.byref(h), ndev, len_, k, rows, _p(gftbls), depth)
        if rc != 0:
            raise RuntimeError(f"isal_hip_multi_create failed ({rc})")
        self._h = h

    @property
    def ndev(self) -> int:
        return int(lib().isal_hip_multi_ndev(self._h))

    def numa_node(self, dev: int) -> int:
        """NUMA node of device dev's PCIe root (-1 unknown)."""
        return int(lib().isal_hip_multi_numa_node(self._h, dev))

    def worker_cpus(self, dev: int) -> int:
        """How many CPUs device dev's worker thread is pinned to (0: not pinned)."""
        return int(lib().isal_hip_multi_worker_cpus(self._h, dev))

    def encode(self, nstripes: int, data: Sequence, coding: Sequence) -> None:
        """data[s*k + j], coding[s*rows + l]: host buffers of stripe s."""
        if len(data) != nstripes * self.k or len(coding) != nstripes * self.rows:
            raise ValueError("pointer lists must hold nstripes*k and nstripes*rows entries")
        rc = lib().isal_hip_multi_encode(self._h, nstripes, _pp(data), _pp(coding))
        if rc != 0:
            raise RuntimeError(f"isal_hip_multi_encode failed ({rc})")

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().isal_hip_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def partition(nstripes: int, ndev: int, dev: int) -> tuple[int, int]:
    """(first, count) of device/rank `dev`'s contiguous stripe range
    (isal_hip_multi_partition; no GPU needed)."""
    first, count = ctypes.c_longlong(), ctypes.c_longlong()
    lib().isal_hip_multi_partition(nstripes, ndev, dev, ctypes.byref(first), ctypes.byref(count))
    return int(first.value), int(count.value)


def pci_numa_node(pci_bus_id: str, sysfs_root: str | None = None) -> int:
    """NUMA node of a PCI device from sysfs (-1 unknown); no GPU needed."""
    return int(lib().isal_hip_pci_numa_node(sysfs_root.encode() if sysfs_root else None, pci_bus_id.encode()))


def numa_node_cpus(node: int, sysfs_root: str | None = None) -> list[int] | None:
    """CPUs of a NUMA node from its sysfs cpulist (None when unreadable)."""
    buf = (ctypes.c_int * 4096)()
    n = lib().isal_hip_numa_node_cpus(sysfs_root.encode() if sysfs_root else None, node, buf, 4096)
    return None if n < 0 else list(buf[:min(n, 4096)])


def crc32_iscsi(buf, len_: int, init_crc: int, base: bool = False) -> int:
    """crc.h crc32_iscsi(buffer, len, init_crc) (reference include/crc.h:136-150):
    host buffers on the library's CPU route, device buffers on the GPU."""
    f = lib().crc32_iscsi_base if base else lib().crc32_iscsi
    return int(f(ctypes.c_void_p(addr(buf) if buf is not None else 0), len_, init_crc & 0xFFFFFFFF))


def crc64(variant, init_crc: int, buf, len_: int, base: bool = False) -> int:
    """crc64.h crc64_<variant>(init_crc, buf, len) (reference include/crc64.h:54-163);
    variant: a CRC64_VARIANTS name or its index (ISAL_HIP_CRC64_*)."""
    name = variant if isinstance(variant, str) else CRC64_VARIANTS[variant]
    f = getattr(lib(), f"crc64_{name}{'_base' if base else ''}")
    return int(f(init_crc & 0xFFFFFFFFFFFFFFFF, ctypes.c_void_p(addr(buf) if buf is not None else 0), len_))


MEM_PAGEABLE, MEM_DEVICE, MEM_MANAGED, MEM_PINNED = 0, 1, 2, 3


def route_device(kinds: Sequence[int], devs: Sequence[int], cur: int) -> tuple[int, int, list[int]]:
    """isal_hip_route_device: the device a drop-in call with these shards runs
    on (-2: device shards on two GPUs), the first shard on a second GPU (-1:
    none) and the per-shard in-place flags. Pure logic, no GPU needed."""
    n = len(kinds)
    K = (ctypes.c_int * max(n, 1))(*kinds)
    D = (ctypes.c_int * max(n, 1))(*devs)
    P = (ctypes.c_int * max(n, 1))()
    bad = ctypes.c_int(0)
    dev = lib().isal_hip_route_device(n, K, D, cur, ctypes.byref(bad), P)
    return dev, bad.value, list(P[:n])


def selftest_kernels() -> tuple[int, int]:
    """isal_hip_selftest_kernels: (kernels without usable device code, kernels checked)."""
    n = ctypes.c_int(0)
    bad = lib().isal_hip_selftest_kernels(ctypes.byref(n))
    return int(bad), int(n.value)


def slow_waits() -> int:
    """Kernel-argument calls completed by hipStreamSynchronize after the spin expired."""
    return int(lib().isal_hip_slow_waits())


def contexts_created() -> int:
    """Per-thread, per-device contexts the drop-in calls have created."""
    return int(lib().isal_hip_contexts_created())


def kernel_launches() -> int:
    return int(lib().isal_hip_kernel_launches())


def cpu_calls() -> int:
    """Drop-in calls the library served on its CPU route (small host calls,
    ISAL_HIP_BACKEND=cpu, no GPU, HIP-failure fallbacks)."""
    return int(lib().isal_hip_cpu_calls())


def fallbacks() -> int:
    """Drop-in calls that hit a HIP failure and finished on the CPU route."""
    return int(lib().isal_hip_fallbacks())


def reload_config() -> None:
    """Re-read the ISAL_HIP_* environment knobs (read once otherwise)."""
    lib().isal_hip_config_reload()


def max_rows_per_pass() -> int:
    return int(lib().isal_hip_max_rows_per_pass())


def version() -> str:
    return lib().isal_get_version_str().decode()
