"""ctypes binding of libqugemm.so — the C-ABI of include/qgemul.h.

This is plumbing for tests and the benchmark harness; the product boundary is the C-ABI itself
and the C++23 header include/QuBLAS_amd.h that lowers the reference's tag API onto it.
The library has no CPU arithmetic path: loading fails loudly if it has not been built, and every
compute call fails with QG_ENOGPU when no gfx950 device is visible.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from .desc import (QG_MAX_EW, Qcomplex, Qu, host_layout, qfmt, qgemul_approx, qgemul_approx_form, qgemul_approx_seg, qgemul_batched_ep, batched_ep, qgemul_grouped_ep, grouped_ep, qgemul_grouped_member, qgemul_cmul, qgemul_cmul_form, qgemul_desc, qgemul_ep_args, qgemul_epilogue,
                   qgemul_epilogue_cplx, qgemul_ew_stage, qgemul_info, qgemul_opts)

_HERE = os.path.dirname(os.path.abspath(__file__))
# QUBLAS_AMD_DIAG=1 (tools/ only) loads the diagnostic build: environment A/B switches and ablation variants exist there and
# nowhere else (qublas_amd/build.py).  Tests, smoke and bench load the product library.
LIB_PATH = os.path.join(_HERE, "libqugemm_diag.so" if os.environ.get("QUBLAS_AMD_DIAG") == "1" else "libqugemm.so")

QG_OK, QG_EINVAL, QG_EUNSUPPORTED, QG_EHIP, QG_ERCCL, QG_ERANGE, QG_ENOGPU = 0, -1, -2, -3, -4, -5, -6
OPT_FORCE_TREE, OPT_CHECK_RANGE, OPT_GENERIC_TREE, OPT_RUNTIME_MODES, OPT_FUSED_EPILOGUE, OPT_UNFUSED_EPILOGUE = 1, 2, 4, 8, 16, 32
OPT_GENERIC_LAYOUT, OPT_LOCKSTEP_TILES, OPT_ARITHMETIC_CONV, OPT_ALL_DEVICES = 64, 128, 256, 512
OPT_SCHOOLBOOK_LIMBS = 2048   # 17/18-bit operands: balanced base-256 limbs and 9 products, not three base-64 digits and 6; result-identical
OPT_APPROX_GENERAL = 4096   # chains with an APPROX stage: uniform tables through the general form of the pass; result-identical
OPT_BATCHED_TREE = 16384   # batched plans of tree-class members on the tiled 32-bit tree kernels (at most 12 levels): one launch for the whole batch; result-identical
OPT_BATCHED_STACKED = 8192   # batched plans of complex / real x complex linear-class members: one block-diagonal launch + one combine pass; result-identical
OPT_BALANCED_LIMBS = 1024   # never centre an operand (x - c in balanced limbs): the plain balanced limbs, result-identical
OPERAND_A, OPERAND_B, OPERAND_C = 0, 1, 2
BITS_ASCII, BITS_PACKED = 0, 1
KERNEL_NAMES = {0: "none", 1: "mfma_i8", 2: "mfma_i8_limb", 3: "tree_i32", 4: "tree_i64", 5: "tree_cplx", 6: "tree_cplx_i32", 7: "mfma_cplx", 8: "gemv_i32", 9: "gemv_i64", 10: "tree_i128", 11: "tree_rc_i32", 12: "mfma_rc"}
CMUL_NAMES = {0: "none", 1: "basic", 2: "tf", 3: "real_a", 4: "real_b"}

EXPORTS = [
    "qgemul_classify", "qgemul_strerror", "qgemul_abi_version", "qgemul_last_hip_error", "qgemul_run",
    "qgemul_ctx_create", "qgemul_ctx_destroy", "qgemul_ctx_sync", "qgemul_ctx_stream",
    "qgemul_plan_create", "qgemul_plan_destroy", "qgemul_plan_info",
    "qgemul_dev_alloc", "qgemul_dev_free", "qgemul_memcpy_h2d", "qgemul_memcpy_d2h",
    "qgemul_pack", "qgemul_pack_f64", "qgemul_unpack_c", "qgemul_execute", "qgemul_fill_packed", "qgemul_time_execute",
    "qgemul_classify_ep", "qgemul_plan_create_ep", "qgemul_packed_e_bytes", "qgemul_pack_e", "qgemul_execute_ep",
    "qgemul_time_execute_ep", "qgemul_run_ep", "qgemul_plan_fuses_epilogue", "qgemul_plan_packed_layout", "qgemul_classify_epc", "qgemul_plan_create_epc", "qgemul_run_epc",
    "qgemul_bitstream_bytes", "qgemul_export_bitstream", "qgemul_run_release", "qgemul_run_sharded", "qgemul_execute_host_c", "qgemul_plan_stores_host_c",
    "qgemul_comm_unique_id", "qgemul_comm_create", "qgemul_comm_destroy", "qgemul_comm_info", "qgemul_gather_packed_c", "qgemul_comm_fence",
    "qgemul_comm_sync", "qgemul_comm_barrier", "qgemul_comm_max_f64", "qgemul_last_rccl_error", "qgemul_ctx_device",
    "qgemul_classify_epx", "qgemul_plan_create_epx", "qgemul_run_epx", "qgemul_plan_approx_uniform", "qgemul_sizeof", "qgemul_approx_plan_form", "qgemul_apply_epilogue", "qgemul_time_apply_epilogue", "qgemul_packed_c_bytes", "qgemul_pack_c",
    "qgemul_classify_epcx", "qgemul_plan_create_epcx", "qgemul_run_epcx", "qgemul_cmul_plan_form",
    "qgemul_classify_batched", "qgemul_classify_batched_launches", "qgemul_plan_create_batched", "qgemul_plan_batched_launches", "qgemul_pack_batched",
    "qgemul_unpack_c_batched", "qgemul_execute_batched", "qgemul_time_execute_batched", "qgemul_time_execute_batched_launch", "qgemul_run_batched",
    "qgemul_classify_batched_epx", "qgemul_classify_batched_epx_launches", "qgemul_plan_create_batched_epx", "qgemul_pack_e_batched", "qgemul_execute_batched_ep",
    "qgemul_time_execute_batched_ep", "qgemul_run_batched_epx",
    "qgemul_classify_grouped", "qgemul_classify_grouped_launches", "qgemul_classify_grouped_member", "qgemul_plan_create_grouped", "qgemul_plan_grouped_launches",
    "qgemul_plan_grouped_member", "qgemul_pack_grouped", "qgemul_unpack_c_grouped", "qgemul_execute_grouped", "qgemul_time_execute_grouped", "qgemul_run_grouped",
    "qgemul_classify_grouped_epx", "qgemul_classify_grouped_epx_launches", "qgemul_classify_grouped_epx_member", "qgemul_plan_create_grouped_epx",
    "qgemul_grouped_set_scalars", "qgemul_pack_e_grouped", "qgemul_execute_grouped_ep", "qgemul_time_execute_grouped_ep", "qgemul_run_grouped_epx",
]
# qgemul_sizeof ids (include/qgemul.h) and the ctypes mirror each one must match
SIZEOF_MIRRORS = {0: qfmt, 1: qgemul_desc, 2: qgemul_opts, 3: qgemul_info, 4: qgemul_ew_stage, 5: qgemul_epilogue, 6: qgemul_ep_args,
                  7: qgemul_epilogue_cplx, 8: qgemul_approx_seg, 9: qgemul_approx, 10: qgemul_cmul, 12: qgemul_grouped_member, 13: qgemul_grouped_ep}

_lib = None


class QgemulError(RuntimeError):
    def __init__(self, status: int, what: str = ""):
        self.status = status
        msg = lib().qgemul_strerror(status).decode()
        if status == QG_EHIP:
            msg += f" (hipError {lib().qgemul_last_hip_error()})"
        super().__init__(f"{what}: {msg}" if what else msg)


def lib() -> C.CDLL:
    """Load the engine.  Raises if the library is missing: there is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not built: run `python -m qublas_amd.build` (hipcc, gfx950). "
                              "The engine has no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        vp, i64, u32, u64 = C.c_void_p, C.c_int64, C.c_uint32, C.c_uint64
        pd = C.POINTER(qgemul_desc)
        L.qgemul_classify.argtypes = [pd, u32, C.POINTER(qgemul_info)]
        L.qgemul_strerror.restype = C.c_char_p
        L.qgemul_strerror.argtypes = [C.c_int]
        L.qgemul_abi_version.restype = u32
        L.qgemul_run.argtypes = [pd, vp, vp, vp, C.POINTER(qgemul_opts)]
        L.qgemul_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.qgemul_ctx_destroy.argtypes = [vp]
        L.qgemul_ctx_destroy.restype = None
        L.qgemul_ctx_sync.argtypes = [vp]
        L.qgemul_ctx_stream.argtypes = [vp]
        L.qgemul_ctx_stream.restype = vp
        L.qgemul_plan_create.argtypes = [vp, pd, u32, C.POINTER(vp)]
        L.qgemul_plan_destroy.argtypes = [vp]
        L.qgemul_plan_destroy.restype = None
        L.qgemul_plan_info.argtypes = [vp, C.POINTER(qgemul_info)]
        L.qgemul_dev_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
        L.qgemul_dev_free.argtypes = [vp, vp]
        L.qgemul_memcpy_h2d.argtypes = [vp, vp, vp, C.c_size_t]
        L.qgemul_memcpy_d2h.argtypes = [vp, vp, vp, C.c_size_t]
        L.qgemul_pack.argtypes = [vp, C.c_int, vp, i64, vp]
        L.qgemul_pack_f64.argtypes = [vp, C.c_int, vp, i64, vp]
        L.qgemul_unpack_c.argtypes = [vp, vp, vp, i64]
        L.qgemul_execute.argtypes = [vp, vp, vp, vp]
        L.qgemul_fill_packed.argtypes = [vp, C.c_int, u64, C.c_int, vp]
        L.qgemul_time_execute.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.POINTER(C.c_float)]
        pe = C.POINTER(qgemul_epilogue)
        pa = C.POINTER(qgemul_ep_args)
        L.qgemul_classify_ep.argtypes = [pd, pe, u32, C.POINTER(qgemul_info)]
        L.qgemul_plan_create_ep.argtypes = [vp, pd, pe, u32, C.POINTER(vp)]
        pec = C.POINTER(qgemul_epilogue_cplx)
        L.qgemul_classify_epc.argtypes = [pd, pec, u32, C.POINTER(qgemul_info)]
        L.qgemul_plan_create_epc.argtypes = [vp, pd, pec, u32, C.POINTER(vp)]
        L.qgemul_run_epc.argtypes = [pd, pec, vp, vp, vp, C.POINTER(vp), C.POINTER(qgemul_opts)]
        L.qgemul_plan_fuses_epilogue.argtypes = [vp]
        L.qgemul_plan_packed_layout.argtypes = [vp, C.c_int, C.POINTER(C.c_int64)]
        L.qgemul_run_release.argtypes = []
        L.qgemul_run_release.restype = None
        L.qgemul_bitstream_bytes.argtypes = [vp, C.c_int]
        L.qgemul_bitstream_bytes.restype = i64
        L.qgemul_export_bitstream.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp]
        L.qgemul_packed_e_bytes.argtypes = [vp, C.c_int]
        L.qgemul_packed_e_bytes.restype = i64
        L.qgemul_pack_e.argtypes = [vp, C.c_int, vp, i64, vp]
        L.qgemul_execute_ep.argtypes = [vp, vp, vp, vp, pa]
        L.qgemul_time_execute_ep.argtypes = [vp, vp, vp, vp, pa, C.c_int, C.c_int, C.POINTER(C.c_float)]
        L.qgemul_run_ep.argtypes = [pd, pe, vp, vp, vp, C.POINTER(vp), C.POINTER(qgemul_opts)]
        L.qgemul_comm_unique_id.argtypes = [vp]
        L.qgemul_comm_create.argtypes = [vp, C.c_int, C.c_int, vp, C.POINTER(vp)]
        L.qgemul_comm_destroy.argtypes = [vp]
        L.qgemul_comm_destroy.restype = None
        pi = C.POINTER(C.c_int)
        L.qgemul_comm_info.argtypes = [vp, pi, pi, pi]
        L.qgemul_gather_packed_c.argtypes = [vp, vp, C.c_size_t, C.POINTER(vp), C.POINTER(C.c_size_t), C.c_int, C.c_int]
        L.qgemul_comm_fence.argtypes = [vp, C.c_int]
        L.qgemul_comm_sync.argtypes = [vp]
        L.qgemul_comm_barrier.argtypes = [vp]
        L.qgemul_comm_max_f64.argtypes = [vp, C.POINTER(C.c_double)]
        L.qgemul_ctx_device.argtypes = [vp]
        pax = C.POINTER(C.POINTER(qgemul_approx))
        L.qgemul_classify_epx.argtypes = [pd, pe, pax, u32, C.POINTER(qgemul_info)]
        L.qgemul_plan_create_epx.argtypes = [vp, pd, pe, pax, u32, C.POINTER(vp)]
        L.qgemul_run_epx.argtypes = [pd, pe, pax, vp, vp, vp, C.POINTER(vp), C.POINTER(qgemul_opts)]
        L.qgemul_plan_approx_uniform.argtypes = [vp]
        L.qgemul_approx_plan_form.argtypes = [pd, pe, pax, C.POINTER(qgemul_approx_form)]
        L.qgemul_packed_c_bytes.argtypes = [vp]
        L.qgemul_packed_c_bytes.restype = i64
        L.qgemul_pack_c.argtypes = [vp, vp, i64, vp]
        L.qgemul_apply_epilogue.argtypes = [vp, vp, vp, pa]
        L.qgemul_time_apply_epilogue.argtypes = [vp, vp, vp, pa, C.c_int, C.c_int, C.POINTER(C.c_float)]
        pcx = C.POINTER(C.POINTER(qgemul_cmul))
        L.qgemul_classify_epcx.argtypes = [pd, pec, pcx, u32, C.POINTER(qgemul_info)]
        L.qgemul_plan_create_epcx.argtypes = [vp, pd, pec, pcx, u32, C.POINTER(vp)]
        L.qgemul_run_epcx.argtypes = [pd, pec, pcx, vp, vp, vp, C.POINTER(vp), C.POINTER(qgemul_opts)]
        L.qgemul_cmul_plan_form.argtypes = [pd, pec, pcx, C.POINTER(qgemul_cmul_form)]
        L.qgemul_classify_batched.argtypes = [pd, i64, u32, C.POINTER(qgemul_info)]
        L.qgemul_classify_batched_launches.argtypes = [pd, i64, u32]
        L.qgemul_plan_create_batched.argtypes = [vp, pd, i64, u32, C.POINTER(vp)]
        L.qgemul_plan_batched_launches.argtypes = [vp]
        L.qgemul_pack_batched.argtypes = [vp, C.c_int, vp, i64, i64, vp]
        L.qgemul_unpack_c_batched.argtypes = [vp, vp, vp, i64, i64]
        L.qgemul_execute_batched.argtypes = [vp, vp, vp, vp]
        L.qgemul_time_execute_batched.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.POINTER(C.c_float)]
        L.qgemul_time_execute_batched_launch.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
        L.qgemul_run_batched.argtypes = [pd, i64, vp, vp, vp, i64, i64, i64, C.POINTER(qgemul_opts)]
        pbe = C.POINTER(qgemul_batched_ep)
        L.qgemul_classify_batched_epx.argtypes = [pd, i64, pe, pax, pbe, u32, C.POINTER(qgemul_info)]
        L.qgemul_classify_batched_epx_launches.argtypes = [pd, i64, pe, pax, pbe, u32]
        L.qgemul_plan_create_batched_epx.argtypes = [vp, pd, i64, pe, pax, pbe, u32, C.POINTER(vp)]
        L.qgemul_pack_e_batched.argtypes = [vp, C.c_int, vp, i64, i64, vp]
        L.qgemul_execute_batched_ep.argtypes = [vp, vp, vp, vp, pa]
        L.qgemul_time_execute_batched_ep.argtypes = [vp, vp, vp, vp, pa, C.c_int, C.c_int, C.POINTER(C.c_float)]
        L.qgemul_run_batched_epx.argtypes = [pd, i64, pe, pax, vp, vp, vp, C.POINTER(vp), i64, i64, i64, C.POINTER(i64), C.POINTER(qgemul_opts)]
        pgm, pvp, pi64 = C.POINTER(qgemul_grouped_member), C.POINTER(vp), C.POINTER(i64)
        L.qgemul_classify_grouped.argtypes = [pd, i64, u32, C.POINTER(qgemul_info)]
        L.qgemul_classify_grouped_launches.argtypes = [pd, i64, u32]
        L.qgemul_classify_grouped_member.argtypes = [pd, i64, u32, i64, pgm]
        L.qgemul_plan_create_grouped.argtypes = [vp, pd, i64, u32, C.POINTER(vp)]
        L.qgemul_plan_grouped_launches.argtypes = [vp]
        L.qgemul_plan_grouped_member.argtypes = [vp, i64, pgm]
        L.qgemul_pack_grouped.argtypes = [vp, C.c_int, pvp, pi64, vp]
        L.qgemul_unpack_c_grouped.argtypes = [vp, vp, pvp, pi64]
        L.qgemul_execute_grouped.argtypes = [vp, vp, vp, vp]
        L.qgemul_time_execute_grouped.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.POINTER(C.c_float)]
        L.qgemul_run_grouped.argtypes = [pd, i64, pvp, pvp, pvp, pi64, pi64, pi64, C.POINTER(qgemul_opts)]
        pge = C.POINTER(qgemul_grouped_ep)
        L.qgemul_classify_grouped_epx.argtypes = [pd, i64, pe, pax, pge, u32, C.POINTER(qgemul_info)]
        L.qgemul_classify_grouped_epx_launches.argtypes = [pd, i64, pe, pax, pge, u32]
        L.qgemul_classify_grouped_epx_member.argtypes = [pd, i64, pe, pax, pge, u32, i64, pgm]
        L.qgemul_plan_create_grouped_epx.argtypes = [vp, pd, i64, pe, pax, pge, u32, C.POINTER(vp)]
        L.qgemul_grouped_set_scalars.argtypes = [vp, C.c_int, pi64]
        L.qgemul_pack_e_grouped.argtypes = [vp, C.c_int, pvp, pi64, vp]
        L.qgemul_execute_grouped_ep.argtypes = [vp, vp, vp, vp, pa]
        L.qgemul_time_execute_grouped_ep.argtypes = [vp, vp, vp, vp, pa, C.c_int, C.c_int, C.POINTER(C.c_float)]
        L.qgemul_run_grouped_epx.argtypes = [pd, i64, pe, pax, pge, pvp, pvp, pvp, C.POINTER(pvp), C.POINTER(pi64), pi64, pi64, pi64, C.POINTER(qgemul_opts)]
        L.qgemul_sizeof.argtypes = [C.c_int]
        L.qgemul_sizeof.restype = C.c_size_t
        _lib = L
    return _lib


def _chk(st: int, what: str = ""):
    if st != QG_OK:
        raise QgemulError(st, what)


def classify(desc: qgemul_desc, flags: int = 0) -> qgemul_info:
    info = qgemul_info()
    _chk(lib().qgemul_classify(C.byref(desc), flags, C.byref(info)), "qgemul_classify")
    return info


def run_release():
    """free the calling thread's qgemul_run cache (context, plan, device buffers)"""
    lib().qgemul_run_release()


def classify_ep_status(desc: qgemul_desc, ep, flags: int = 0):
    info = qgemul_info()
    fn = lib().qgemul_classify_epc if isinstance(ep, qgemul_epilogue_cplx) else lib().qgemul_classify_ep
    st = fn(C.byref(desc), C.byref(ep), flags, C.byref(info))
    return st, info


def run_ep(desc: qgemul_desc, ep, D_out: np.ndarray, A: np.ndarray, B: np.ndarray, E, *, lda: int = 0,
           ldb: int = 0, ldc: int = 0, device: int = -1, flags: int = 0) -> np.ndarray:
    """qgemul_run_ep / qgemul_run_epc: E[k] = host-layout tensor (tight, column-major flattening) or a 1-element array for a
    scalar stage ({re, im} structured elements for a complex operand)."""
    A = np.ascontiguousarray(A)
    B = np.ascontiguousarray(B)
    E = [np.ascontiguousarray(e) for e in E]
    ptrs = (C.c_void_p * max(1, len(E)))(*[e.ctypes.data for e in E])
    o = qgemul_opts(lda, ldb, ldc, device, flags)
    fn = lib().qgemul_run_epc if isinstance(ep, qgemul_epilogue_cplx) else lib().qgemul_run_ep
    _chk(fn(C.byref(desc), C.byref(ep), D_out.ctypes.data_as(C.c_void_p), A.ctypes.data_as(C.c_void_p),
            B.ctypes.data_as(C.c_void_p), ptrs, C.byref(o)), "qgemul_run_ep")
    return D_out


def _tables(approx):
    """QG_MAX_EW pointers: the stage's qgemul_approx, or null for a stage that is no APPROX stage"""
    approx = list(approx) + [None] * (QG_MAX_EW - len(approx))
    return (C.POINTER(qgemul_approx) * QG_MAX_EW)(*[C.pointer(t) if t is not None else None for t in approx[:QG_MAX_EW]])


def classify_epx(desc: qgemul_desc, ep: qgemul_epilogue, approx, flags: int = 0):
    """qgemul_classify_epx: (status, info); approx[k] = stage k's qgemul_approx or None (desc.lower_epilogue_x)"""
    info = qgemul_info()
    st = lib().qgemul_classify_epx(C.byref(desc), C.byref(ep), _tables(approx), flags, C.byref(info))
    return st, info


def run_epx(desc: qgemul_desc, ep: qgemul_epilogue, approx, D_out: np.ndarray, A: np.ndarray, B: np.ndarray, E, *, lda: int = 0,
            ldb: int = 0, ldc: int = 0, device: int = -1, flags: int = 0) -> np.ndarray:
    """qgemul_run_epx: as run_ep; E[k] of an APPROX stage is ignored (None)"""
    A = np.ascontiguousarray(A)
    B = np.ascontiguousarray(B)
    E = [None if e is None else np.ascontiguousarray(e) for e in E]
    ptrs = (C.c_void_p * max(1, len(E)))(*[None if e is None else e.ctypes.data for e in E])
    o = qgemul_opts(lda, ldb, ldc, device, flags)
    _chk(lib().qgemul_run_epx(C.byref(desc), C.byref(ep), _tables(approx), D_out.ctypes.data_as(C.c_void_p), A.ctypes.data_as(C.c_void_p),
                              B.ctypes.data_as(C.c_void_p), ptrs, C.byref(o)), "qgemul_run_epx")
    return D_out


def approx_plan_form(desc: qgemul_desc, ep: qgemul_epilogue, approx) -> qgemul_approx_form:
    out = qgemul_approx_form()
    _chk(lib().qgemul_approx_plan_form(C.byref(desc), C.byref(ep), _tables(approx), C.byref(out)), "qgemul_approx_plan_form")
    return out


def _cmuls(cmul):
    """QG_MAX_EW pointers: the stage's qgemul_cmul, or null for a stage that is no CMUL stage"""
    cmul = list(cmul) + [None] * (QG_MAX_EW - len(cmul))
    return (C.POINTER(qgemul_cmul) * QG_MAX_EW)(*[C.pointer(t) if t is not None else None for t in cmul[:QG_MAX_EW]])


def classify_epcx(desc: qgemul_desc, ep: qgemul_epilogue_cplx, cmul, flags: int = 0):
    """qgemul_classify_epcx: (status, info); cmul[k] = stage k's qgemul_cmul or None (desc.lower_epilogue_cplx_x)"""
    info = qgemul_info()
    st = lib().qgemul_classify_epcx(C.byref(desc), C.byref(ep), _cmuls(cmul), flags, C.byref(info))
    return st, info


def cmul_plan_form(desc: qgemul_desc, ep: qgemul_epilogue_cplx, cmul):
    """qgemul_cmul_plan_form: (status, form)"""
    out = qgemul_cmul_form()
    st = lib().qgemul_cmul_plan_form(C.byref(desc), C.byref(ep), _cmuls(cmul), C.byref(out))
    return st, out


def run_epcx(desc: qgemul_desc, ep: qgemul_epilogue_cplx, cmul, D_out: np.ndarray, A: np.ndarray, B: np.ndarray, E, *, lda: int = 0,
             ldb: int = 0, ldc: int = 0, device: int = -1, flags: int = 0) -> np.ndarray:
    """qgemul_run_epcx: as run_ep on a complex chain that may hold CMUL stages"""
    A = np.ascontiguousarray(A)
    B = np.ascontiguousarray(B)
    E = [np.ascontiguousarray(e) for e in E]
    ptrs = (C.c_void_p * max(1, len(E)))(*[e.ctypes.data for e in E])
    o = qgemul_opts(lda, ldb, ldc, device, flags)
    _chk(lib().qgemul_run_epcx(C.byref(desc), C.byref(ep), _cmuls(cmul), D_out.ctypes.data_as(C.c_void_p), A.ctypes.data_as(C.c_void_p),
                               B.ctypes.data_as(C.c_void_p), ptrs, C.byref(o)), "qgemul_run_epcx")
    return D_out


def sizeof(which: int) -> int:
    return int(lib().qgemul_sizeof(which))


def classify_status(desc: qgemul_desc, flags: int = 0):
    info = qgemul_info()
    st = lib().qgemul_classify(C.byref(desc), flags, C.byref(info))
    return st, info


def run(desc: qgemul_desc, C_out: np.ndarray, A: np.ndarray, B: np.ndarray, *, lda: int = 0, ldb: int = 0,
        ldc: int = 0, device: int = -1, flags: int = 0) -> np.ndarray:
    """qgemul_run on host-layout numpy buffers (see oracle.qoracle.host_dtype for the element dtype)."""
    A = np.ascontiguousarray(A)
    B = np.ascontiguousarray(B)
    assert C_out.flags["C_CONTIGUOUS"]
    o = qgemul_opts(lda, ldb, ldc, device, flags)
    _chk(lib().qgemul_run(C.byref(desc), C_out.ctypes.data_as(C.c_void_p), A.ctypes.data_as(C.c_void_p),
                          B.ctypes.data_as(C.c_void_p), C.byref(o)), "qgemul_run")
    return C_out


def classify_batched_status(desc: qgemul_desc, batch: int, flags: int = 0):
    """qgemul_classify_batched: (status, info); info.packed_bytes are for the whole batch"""
    info = qgemul_info()
    st = lib().qgemul_classify_batched(C.byref(desc), batch, flags, C.byref(info))
    return st, info


def classify_batched_launches(desc: qgemul_desc, batch: int, flags: int = 0) -> int:
    """kernel launches per execute of the batched plan (1: the block-diagonal form); a negative value is a status"""
    return int(lib().qgemul_classify_batched_launches(C.byref(desc), batch, flags))


def run_batched_status(desc: qgemul_desc, batch: int, C_out: np.ndarray, A: np.ndarray, B: np.ndarray, strideC: int, strideA: int, strideB: int, *,
                       lda: int = 0, ldb: int = 0, ldc: int = 0, device: int = -1, flags: int = 0) -> int:
    """qgemul_run_batched on host-layout numpy buffers (strides in host elements); returns the status"""
    A = np.ascontiguousarray(A)
    B = np.ascontiguousarray(B)
    assert C_out.flags["C_CONTIGUOUS"]
    o = qgemul_opts(lda, ldb, ldc, device, flags)
    return int(lib().qgemul_run_batched(C.byref(desc), batch, C_out.ctypes.data_as(C.c_void_p), A.ctypes.data_as(C.c_void_p), B.ctypes.data_as(C.c_void_p),
                                        strideC, strideA, strideB, C.byref(o)))


def run_batched(desc: qgemul_desc, batch: int, C_out: np.ndarray, A: np.ndarray, B: np.ndarray, strideC: int, strideA: int, strideB: int, **kw) -> np.ndarray:
    _chk(run_batched_status(desc, batch, C_out, A, B, strideC, strideA, strideB, **kw), "qgemul_run_batched")
    return C_out


# ---- grouped Qgemul (include/qgemul.h, qgemul_*_grouped): a list of descriptors, member g is Qgemul<...>(C_g, A_g, B_g) ----
def _desc_array(descs):
    arr = (qgemul_desc * len(descs))()
    for g, d in enumerate(descs):
        arr[g] = d
    return arr


def _ptr_array(ptrs):
    return (C.c_void_p * len(ptrs))(*[C.c_void_p(int(p)) if p else C.c_void_p() for p in ptrs])


def _ld_array(ld, n):
    """None: every member tight"""
    if ld is None:
        return None
    assert len(ld) == n
    return (C.c_int64 * n)(*[int(x) for x in ld])


def classify_grouped_status(descs, flags: int = 0):
    """qgemul_classify_grouped: (status, info); info.packed_bytes and ops are the whole group's"""
    info = qgemul_info()
    st = lib().qgemul_classify_grouped(_desc_array(descs) if len(descs) else None, len(descs), flags, C.byref(info))
    return st, info


def classify_grouped_launches(descs, flags: int = 0) -> int:
    """kernel launches per execute of the grouped plan; a negative value is a status"""
    return int(lib().qgemul_classify_grouped_launches(_desc_array(descs) if len(descs) else None, len(descs), flags))


def classify_grouped_member(descs, g: int, flags: int = 0) -> qgemul_grouped_member:
    """where member g will live (pure host code: what GroupedPlan.member(g) answers)"""
    out = qgemul_grouped_member()
    _chk(lib().qgemul_classify_grouped_member(_desc_array(descs), len(descs), flags, g, C.byref(out)), "qgemul_classify_grouped_member")
    return out


def run_grouped_status(descs, Cs, As, Bs, *, lda=None, ldb=None, ldc=None, flags: int = 0, device: int = -1) -> int:
    """qgemul_run_grouped on lists of host-layout numpy buffers (None for a member with M == 0 or N == 0); returns the status"""
    n = len(descs)
    o = qgemul_opts(device=device, flags=flags)
    ptr = lambda xs: _ptr_array([x.ctypes.data if x is not None else 0 for x in xs])
    return int(lib().qgemul_run_grouped(_desc_array(descs), n, ptr(Cs), ptr(As), ptr(Bs), _ld_array(lda, n), _ld_array(ldb, n), _ld_array(ldc, n), C.byref(o)))


def run_grouped(descs, Cs, As, Bs, **kw):
    _chk(run_grouped_status(descs, Cs, As, Bs, **kw), "qgemul_run_grouped")
    return Cs


# ---- element-wise chains on grouped plans (include/qgemul.h, qgemul_*_grouped_ep*): ONE chain, scalars per member where asked ----
def _per_member(per_member):
    """a qgemul_grouped_ep from a sequence of flags (None: no stage is per member)"""
    return C.byref(grouped_ep(per_member)) if per_member is not None else None


def _ax(approx):
    return _tables(approx) if approx is not None else None


def classify_grouped_epx_status(descs, ep: qgemul_epilogue, approx=None, per_member=None, flags: int = 0):
    """qgemul_classify_grouped_epx: (status, info); approx[k] = stage k's qgemul_approx or None, per_member[k] = scalar stage k takes a value per member"""
    info = qgemul_info()
    st = lib().qgemul_classify_grouped_epx(_desc_array(descs) if len(descs) else None, len(descs), C.byref(ep) if ep is not None else None, _ax(approx),
                                           _per_member(per_member), flags, C.byref(info))
    return st, info


def classify_grouped_epx_launches(descs, ep: qgemul_epilogue, approx=None, per_member=None, flags: int = 0) -> int:
    """kernel launches per execute_ep of the grouped plan; a negative value is a status"""
    return int(lib().qgemul_classify_grouped_epx_launches(_desc_array(descs) if len(descs) else None, len(descs), C.byref(ep), _ax(approx), _per_member(per_member), flags))


def classify_grouped_epx_member(descs, ep: qgemul_epilogue, g: int, approx=None, per_member=None, flags: int = 0) -> qgemul_grouped_member:
    """where member g will live (off[2] / bytes[2]: in packed D)"""
    out = qgemul_grouped_member()
    _chk(lib().qgemul_classify_grouped_epx_member(_desc_array(descs), len(descs), C.byref(ep), _ax(approx), _per_member(per_member), flags, g, C.byref(out)),
         "qgemul_classify_grouped_epx_member")
    return out


def run_grouped_epx_status(descs, ep: qgemul_epilogue, approx, per_member, Ds, As, Bs, E, scalars, *, lda=None, ldb=None, ldd=None, flags: int = 0,
                           device: int = -1) -> int:
    """qgemul_run_grouped_epx on lists of host-layout numpy buffers.  E[k]: the members' tight operands of tensor stage k (a list), the one
    scalar element of a scalar stage that is not per member (an array), or None; scalars[k]: the per-member raw values of stage k or None.
    Returns the status."""
    n = len(descs)
    o = qgemul_opts(device=device, flags=flags)
    ptr = lambda xs: _ptr_array([x.ctypes.data if x is not None else 0 for x in xs])
    keep = []
    Ep = (C.POINTER(C.c_void_p) * QG_MAX_EW)()
    Sp = (C.POINTER(C.c_int64) * QG_MAX_EW)()
    for k in range(QG_MAX_EW):
        e = E[k] if E is not None and k < len(E) else None
        if e is not None:
            arr = ptr(list(e) if isinstance(e, (list, tuple)) else [e] * n)
            keep.append(arr)
            Ep[k] = C.cast(arr, C.POINTER(C.c_void_p))
        sc = scalars[k] if scalars is not None and k < len(scalars) else None
        if sc is not None:
            arr = (C.c_int64 * n)(*[int(x) for x in sc])
            keep.append(arr)
            Sp[k] = C.cast(arr, C.POINTER(C.c_int64))
    return int(lib().qgemul_run_grouped_epx(_desc_array(descs), n, C.byref(ep), _ax(approx), _per_member(per_member), ptr(Ds), ptr(As), ptr(Bs), Ep, Sp,
                                            _ld_array(lda, n), _ld_array(ldb, n), _ld_array(ldd, n), C.byref(o)))


def run_grouped_epx(descs, ep, approx, per_member, Ds, As, Bs, E, scalars, **kw):
    _chk(run_grouped_epx_status(descs, ep, approx, per_member, Ds, As, Bs, E, scalars, **kw), "qgemul_run_grouped_epx")
    return Ds


def _shared(shared):
    """a qgemul_batched_ep from a sequence of flags (None: no stage is shared)"""
    return C.byref(batched_ep(shared)) if shared is not None else None


def classify_batched_epx_status(desc: qgemul_desc, batch: int, ep: qgemul_epilogue, approx=None, shared=None, flags: int = 0):
    """qgemul_classify_batched_epx: (status, info); approx[k] = stage k's qgemul_approx or None, shared[k] = stage k's operand is shared"""
    info = qgemul_info()
    st = lib().qgemul_classify_batched_epx(C.byref(desc), batch, C.byref(ep), _tables(approx) if approx is not None else None, _shared(shared), flags, C.byref(info))
    return st, info


def classify_batched_epx_launches(desc: qgemul_desc, batch: int, ep: qgemul_epilogue, approx=None, shared=None, flags: int = 0) -> int:
    """kernel launches per execute_ep of the batched plan (1 fused, 2 pass form, else batch x the member's); negative: a status"""
    return int(lib().qgemul_classify_batched_epx_launches(C.byref(desc), batch, C.byref(ep), _tables(approx) if approx is not None else None, _shared(shared), flags))


def run_batched_epx_status(desc: qgemul_desc, batch: int, ep: qgemul_epilogue, approx, D_out: np.ndarray, A: np.ndarray, B: np.ndarray, E, strideD: int, strideA: int,
                           strideB: int, strideE, *, lda: int = 0, ldb: int = 0, ldc: int = 0, device: int = -1, flags: int = 0) -> int:
    """qgemul_run_batched_epx on host-layout numpy buffers; E[k]: stage k's tensor(s), its one scalar element, or None (APPROX);
    strideE[k] = 0 marks stage k as shared.  Returns the status."""
    A = np.ascontiguousarray(A)
    B = np.ascontiguousarray(B)
    assert D_out.flags["C_CONTIGUOUS"]
    E = [None if e is None else np.ascontiguousarray(e) for e in E]
    ptrs = (C.c_void_p * QG_MAX_EW)(*[None if e is None else e.ctypes.data for e in E])
    se = (C.c_int64 * QG_MAX_EW)(*[int(x) for x in strideE])
    o = qgemul_opts(lda, ldb, ldc, device, flags)
    return int(lib().qgemul_run_batched_epx(C.byref(desc), batch, C.byref(ep), _tables(approx) if approx is not None else None, D_out.ctypes.data_as(C.c_void_p),
                                            A.ctypes.data_as(C.c_void_p), B.ctypes.data_as(C.c_void_p), ptrs, strideD, strideA, strideB, se, C.byref(o)))


def run_batched_epx(desc, batch, ep, approx, D_out, A, B, E, strideD, strideA, strideB, strideE, **kw) -> np.ndarray:
    _chk(run_batched_epx_status(desc, batch, ep, approx, D_out, A, B, E, strideD, strideA, strideB, strideE, **kw), "qgemul_run_batched_epx")
    return D_out


def run_sharded(desc: qgemul_desc, C_out: np.ndarray, A: np.ndarray, B: np.ndarray, devices, *, lda: int = 0, ldb: int = 0,
                ldc: int = 0, flags: int = 0) -> np.ndarray:
    """qgemul_run_sharded: one process, the rows of C in bands over `devices` (an ordinal may repeat)."""
    A = np.ascontiguousarray(A)
    B = np.ascontiguousarray(B)
    assert C_out.flags["C_CONTIGUOUS"]
    o = qgemul_opts(lda, ldb, ldc, -1, flags)
    devs = (C.c_int * len(devices))(*devices)
    L = lib()
    L.qgemul_run_sharded.argtypes = [C.POINTER(qgemul_desc), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(qgemul_opts), C.POINTER(C.c_int), C.c_int]
    _chk(L.qgemul_run_sharded(C.byref(desc), C_out.ctypes.data_as(C.c_void_p), A.ctypes.data_as(C.c_void_p),
                              B.ctypes.data_as(C.c_void_p), C.byref(o), devs, len(devices)), "qgemul_run_sharded")
    return C_out


class Context:
    def __init__(self, device: int = -1):
        self.h = C.c_void_p()
        _chk(lib().qgemul_ctx_create(device, C.byref(self.h)), "qgemul_ctx_create")

    def close(self):
        if self.h:
            lib().qgemul_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def sync(self):
        _chk(lib().qgemul_ctx_sync(self.h), "qgemul_ctx_sync")

    @property
    def stream(self) -> int:
        return lib().qgemul_ctx_stream(self.h)

    def alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        _chk(lib().qgemul_dev_alloc(self.h, nbytes, C.byref(p)), "qgemul_dev_alloc")
        return p.value

    def free(self, ptr: int):
        _chk(lib().qgemul_dev_free(self.h, C.c_void_p(ptr)), "qgemul_dev_free")

    def h2d(self, dst: int, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        _chk(lib().qgemul_memcpy_h2d(self.h, C.c_void_p(dst), arr.ctypes.data_as(C.c_void_p), arr.nbytes), "h2d")

    def d2h(self, arr: np.ndarray, src: int):
        _chk(lib().qgemul_memcpy_d2h(self.h, arr.ctypes.data_as(C.c_void_p), C.c_void_p(src), arr.nbytes), "d2h")

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Comm:
    """The library-owned RCCL communicator of one rank (include/qgemul.h, qgemul_comm_*): the gather of packed C bands."""
    ID_BYTES = 128

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(Comm.ID_BYTES)
        _chk_rccl(lib().qgemul_comm_unique_id(buf), "qgemul_comm_unique_id")
        return buf.raw

    def __init__(self, ctx: "Context", nranks: int, rank: int, unique_id: bytes):
        assert len(unique_id) == Comm.ID_BYTES
        self.h = C.c_void_p()
        self.nranks, self.rank = nranks, rank
        self._id = C.create_string_buffer(unique_id, Comm.ID_BYTES)
        _chk_rccl(lib().qgemul_comm_create(ctx.h, nranks, rank, self._id, C.byref(self.h)), "qgemul_comm_create")

    def info(self):
        """(ranks per ncclCommCount, this rank per ncclCommUserRank, ncclGetVersion code)"""
        n, r, v = C.c_int(), C.c_int(), C.c_int()
        _chk_rccl(lib().qgemul_comm_info(self.h, C.byref(n), C.byref(r), C.byref(v)), "qgemul_comm_info")
        return n.value, r.value, v.value

    def gather(self, send_ptr: int, send_bytes: int, recv_ptrs=None, recv_bytes=None, root: int = 0, slot: int = 0):
        rp = rb = None
        if recv_ptrs is not None:
            rp = (C.c_void_p * self.nranks)(*[p or None for p in recv_ptrs])
            rb = (C.c_size_t * self.nranks)(*recv_bytes)
        _chk_rccl(lib().qgemul_gather_packed_c(self.h, C.c_void_p(send_ptr), send_bytes, rp, rb, root, slot), "qgemul_gather_packed_c")

    def fence(self, slot: int = -1):
        _chk_rccl(lib().qgemul_comm_fence(self.h, slot), "qgemul_comm_fence")

    def sync(self):
        _chk_rccl(lib().qgemul_comm_sync(self.h), "qgemul_comm_sync")

    def barrier(self):
        _chk_rccl(lib().qgemul_comm_barrier(self.h), "qgemul_comm_barrier")

    def max_f64(self, v: float) -> float:
        x = C.c_double(v)
        _chk_rccl(lib().qgemul_comm_max_f64(self.h, C.byref(x)), "qgemul_comm_max_f64")
        return x.value

    def close(self):
        if self.h:
            lib().qgemul_comm_destroy(self.h)
            self.h = C.c_void_p()


def _chk_rccl(st: int, what: str):
    if st == QG_ERCCL:
        raise QgemulError(st, f"{what} (ncclResult {lib().qgemul_last_rccl_error()})")
    _chk(st, what)


class Plan:
    def __init__(self, ctx: Context, desc: qgemul_desc, flags: int = 0, epilogue=None, approx=None, cmul=None):
        self.ctx = ctx
        self.desc = desc
        self.epilogue = epilogue
        self.h = C.c_void_p()
        if cmul is not None:
            _chk(lib().qgemul_plan_create_epcx(ctx.h, C.byref(desc), C.byref(epilogue), _cmuls(cmul), flags, C.byref(self.h)), "qgemul_plan_create_epcx")
        elif approx is not None and any(t is not None for t in approx):
            _chk(lib().qgemul_plan_create_epx(ctx.h, C.byref(desc), C.byref(epilogue), _tables(approx), flags, C.byref(self.h)), "qgemul_plan_create_epx")
        elif epilogue is None:
            _chk(lib().qgemul_plan_create(ctx.h, C.byref(desc), flags, C.byref(self.h)), "qgemul_plan_create")
        elif isinstance(epilogue, qgemul_epilogue_cplx):
            _chk(lib().qgemul_plan_create_epc(ctx.h, C.byref(desc), C.byref(epilogue), flags, C.byref(self.h)), "qgemul_plan_create_epc")
        else:
            _chk(lib().qgemul_plan_create_ep(ctx.h, C.byref(desc), C.byref(epilogue), flags, C.byref(self.h)), "qgemul_plan_create_ep")
        self.info = qgemul_info()
        _chk(lib().qgemul_plan_info(self.h, C.byref(self.info)), "qgemul_plan_info")

    def close(self):
        if self.h:
            lib().qgemul_plan_destroy(self.h)
            self.h = C.c_void_p()

    def pack(self, operand: int, src_dev: int, packed_dev: int, ld: int = 0):
        _chk(lib().qgemul_pack(self.h, operand, C.c_void_p(src_dev), ld, C.c_void_p(packed_dev)), "qgemul_pack")

    def pack_f64(self, operand: int, src_dev: int, packed_dev: int, ld: int = 0):
        _chk(lib().qgemul_pack_f64(self.h, operand, C.c_void_p(src_dev), ld, C.c_void_p(packed_dev)), "qgemul_pack_f64")

    def fill(self, operand: int, seed: int, dist: int, packed_dev: int):
        _chk(lib().qgemul_fill_packed(self.h, operand, seed, dist, C.c_void_p(packed_dev)), "qgemul_fill_packed")

    def execute(self, pC: int, pA: int, pB: int):
        _chk(lib().qgemul_execute(self.h, C.c_void_p(pC), C.c_void_p(pA), C.c_void_p(pB)), "qgemul_execute")

    def execute_host_c(self, C_dev: int, pA: int, pB: int, ldc: int = 0):
        """packed A, packed B -> C in the reference layout on the device (no packed C where the kernel can store it directly)"""
        L = lib()
        L.qgemul_execute_host_c.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        _chk(L.qgemul_execute_host_c(self.h, C.c_void_p(C_dev), ldc, C.c_void_p(pA), C.c_void_p(pB)), "qgemul_execute_host_c")

    @property
    def stores_host_c(self) -> bool:
        L = lib()
        L.qgemul_plan_stores_host_c.argtypes = [C.c_void_p]
        return bool(L.qgemul_plan_stores_host_c(self.h))

    def bitstream_bytes(self, fmt: int = 0) -> int:
        return int(lib().qgemul_bitstream_bytes(self.h, fmt))

    def export_bitstream(self, pC: int, out_dev: int, tensor_chunk: int = 0, elem_chunk: int = 0, fmt: int = 0):
        _chk(lib().qgemul_export_bitstream(self.h, C.c_void_p(pC), tensor_chunk, elem_chunk, fmt, C.c_void_p(out_dev)),
             "qgemul_export_bitstream")

    def packed_layout(self, operand):
        """(trailer offset, row-sum offset, padded rows, centre) of a packed operand of the linear class (include/qgemul.h)"""
        out = (C.c_int64 * 4)()
        _chk(lib().qgemul_plan_packed_layout(self.h, operand, out), "qgemul_plan_packed_layout")
        return tuple(int(x) for x in out)

    def approx_uniform(self) -> int:
        """1: every APPROX table of the plan has the uniform form, 0: one takes the general form, -1: no APPROX stage"""
        return int(lib().qgemul_plan_approx_uniform(self.h))

    def fuses_epilogue(self) -> bool:
        return bool(lib().qgemul_plan_fuses_epilogue(self.h))

    def packed_e_bytes(self, stage: int) -> int:
        return int(lib().qgemul_packed_e_bytes(self.h, stage))

    def pack_e(self, stage: int, src_dev: int, packed_dev: int, ld: int = 0):
        _chk(lib().qgemul_pack_e(self.h, stage, C.c_void_p(src_dev), ld, C.c_void_p(packed_dev)), "qgemul_pack_e")

    @staticmethod
    def ep_args(packed=(), scalars=(), scalars_im=()) -> qgemul_ep_args:
        a = qgemul_ep_args()
        for k, ptr in enumerate(packed):
            a.e_packed[k] = ptr or None
        for k, v in enumerate(scalars):
            a.e_scalar[k] = int(v or 0)
        for k, v in enumerate(scalars_im):
            a.e_scalar_im[k] = int(v or 0)
        return a

    def execute_ep(self, pD: int, pA: int, pB: int, args: qgemul_ep_args):
        _chk(lib().qgemul_execute_ep(self.h, C.c_void_p(pD), C.c_void_p(pA), C.c_void_p(pB), C.byref(args)), "qgemul_execute_ep")

    def time_execute_ep(self, pD: int, pA: int, pB: int, args: qgemul_ep_args, warmup: int, iters: int) -> float:
        ms = C.c_float()
        _chk(lib().qgemul_time_execute_ep(self.h, C.c_void_p(pD), C.c_void_p(pA), C.c_void_p(pB), C.byref(args), warmup, iters,
                                          C.byref(ms)), "qgemul_time_execute_ep")
        return ms.value

    def packed_c_bytes(self) -> int:
        return int(lib().qgemul_packed_c_bytes(self.h))

    def pack_c(self, src_dev: int, packed_dev: int, ld: int = 0):
        """a device-resident tensor of the Qgemul result's element type -> the packed C that apply_epilogue reads"""
        _chk(lib().qgemul_pack_c(self.h, C.c_void_p(src_dev), ld, C.c_void_p(packed_dev)), "qgemul_pack_c")

    def apply_epilogue(self, pD: int, pC: int, args: qgemul_ep_args):
        """the chain alone: packed C (pack_c) -> packed D"""
        _chk(lib().qgemul_apply_epilogue(self.h, C.c_void_p(pD), C.c_void_p(pC), C.byref(args)), "qgemul_apply_epilogue")

    def time_apply_epilogue(self, pD: int, pC: int, args: qgemul_ep_args, warmup: int, iters: int) -> float:
        ms = C.c_float()
        _chk(lib().qgemul_time_apply_epilogue(self.h, C.c_void_p(pD), C.c_void_p(pC), C.byref(args), warmup, iters, C.byref(ms)),
             "qgemul_time_apply_epilogue")
        return ms.value

    def unpack_c(self, pC: int, dst_dev: int, ld: int = 0):
        _chk(lib().qgemul_unpack_c(self.h, C.c_void_p(pC), C.c_void_p(dst_dev), ld), "qgemul_unpack_c")

    def time_execute(self, pC: int, pA: int, pB: int, warmup: int, iters: int) -> float:
        ms = C.c_float()
        _chk(lib().qgemul_time_execute(self.h, C.c_void_p(pC), C.c_void_p(pA), C.c_void_p(pB), warmup, iters,
                                       C.byref(ms)), "qgemul_time_execute")
        return ms.value


class BatchedPlan:
    """A batched plan (include/qgemul.h, qgemul_*_batched): `batch` GEMMs of one descriptor at constant strides."""

    def __init__(self, ctx: Context, desc: qgemul_desc, batch: int, flags: int = 0, ep=None, approx=None, shared=None):
        """ep: an element-wise chain after every member's GEMM (qgemul_plan_create_batched_epx); approx[k]: stage k's table or
        None; shared[k]: stage k's tensor operand is ONE tensor for every member"""
        self.ctx = ctx
        self.desc = desc
        self.batch = batch
        self.epilogue = ep
        self.h = C.c_void_p()
        if ep is None:
            _chk(lib().qgemul_plan_create_batched(ctx.h, C.byref(desc), batch, flags, C.byref(self.h)), "qgemul_plan_create_batched")
        else:
            _chk(lib().qgemul_plan_create_batched_epx(ctx.h, C.byref(desc), batch, C.byref(ep), _tables(approx) if approx is not None else None, _shared(shared), flags,
                                                      C.byref(self.h)), "qgemul_plan_create_batched_epx")
        self.info = qgemul_info()
        _chk(lib().qgemul_plan_info(self.h, C.byref(self.info)), "qgemul_plan_info")

    def close(self):
        if self.h:
            lib().qgemul_plan_destroy(self.h)
            self.h = C.c_void_p()

    @property
    def launches(self) -> int:
        return int(lib().qgemul_plan_batched_launches(self.h))

    def packed_layout(self, operand):
        out = (C.c_int64 * 4)()
        _chk(lib().qgemul_plan_packed_layout(self.h, operand, out), "qgemul_plan_packed_layout")
        return tuple(int(x) for x in out)

    def pack(self, operand: int, src_dev: int, packed_dev: int, member_stride: int, ld: int = 0):
        _chk(lib().qgemul_pack_batched(self.h, operand, C.c_void_p(src_dev), ld, member_stride, C.c_void_p(packed_dev)), "qgemul_pack_batched")

    def execute(self, pC: int, pA: int, pB: int):
        _chk(lib().qgemul_execute_batched(self.h, C.c_void_p(pC), C.c_void_p(pA), C.c_void_p(pB)), "qgemul_execute_batched")

    def unpack_c(self, pC: int, dst_dev: int, member_stride: int, ld: int = 0):
        _chk(lib().qgemul_unpack_c_batched(self.h, C.c_void_p(pC), C.c_void_p(dst_dev), ld, member_stride), "qgemul_unpack_c_batched")

    def time_execute(self, pC: int, pA: int, pB: int, warmup: int, iters: int) -> float:
        ms = C.c_float()
        _chk(lib().qgemul_time_execute_batched(self.h, C.c_void_p(pC), C.c_void_p(pA), C.c_void_p(pB), warmup, iters, C.byref(ms)), "qgemul_time_execute_batched")
        return ms.value

    def time_execute_launch(self, pC: int, pA: int, pB: int, launch: int, warmup: int, iters: int) -> float:
        """a plan in the stacked form (OPT_BATCHED_STACKED): ms per run of ONE of its launches, 0 the block-diagonal GEMM, 1 the combine pass"""
        ms = C.c_float()
        _chk(lib().qgemul_time_execute_batched_launch(self.h, C.c_void_p(pC), C.c_void_p(pA), C.c_void_p(pB), launch, warmup, iters, C.byref(ms)),
             "qgemul_time_execute_batched_launch")
        return ms.value

    # ---- plans with an element-wise chain (ep is not None) ----
    @property
    def fuses(self) -> int:
        """1: the chain runs inside the GEMM launch(es), 0: as its own pass"""
        return int(lib().qgemul_plan_fuses_epilogue(self.h))

    def packed_e_bytes(self, stage: int) -> int:
        """one member's bytes for a shared stage, the stack's for a per-member one, 0 for a scalar or APPROX stage"""
        return int(lib().qgemul_packed_e_bytes(self.h, stage))

    def pack_e(self, stage: int, src_dev: int, packed_dev: int, member_stride: int, ld: int = 0):
        _chk(lib().qgemul_pack_e_batched(self.h, stage, C.c_void_p(src_dev), ld, member_stride, C.c_void_p(packed_dev)), "qgemul_pack_e_batched")

    def execute_ep(self, pD: int, pA: int, pB: int, args: qgemul_ep_args):
        _chk(lib().qgemul_execute_batched_ep(self.h, C.c_void_p(pD), C.c_void_p(pA), C.c_void_p(pB), C.byref(args)), "qgemul_execute_batched_ep")

    def time_execute_ep(self, pD: int, pA: int, pB: int, args: qgemul_ep_args, warmup: int, iters: int) -> float:
        ms = C.c_float()
        _chk(lib().qgemul_time_execute_batched_ep(self.h, C.c_void_p(pD), C.c_void_p(pA), C.c_void_p(pB), C.byref(args), warmup, iters, C.byref(ms)),
             "qgemul_time_execute_batched_ep")
        return ms.value


class GroupedPlan:
    """A grouped plan (include/qgemul.h, qgemul_*_grouped): GEMMs of different shapes, the eligible ones of one launch key in ONE launch."""

    def __init__(self, ctx: Context, descs, flags: int = 0, ep=None, approx=None, per_member=None):
        """ep: ONE element-wise chain after every member's GEMM (qgemul_plan_create_grouped_epx); approx[k]: stage k's table or None;
        per_member[k]: scalar stage k takes one raw value per member (set_scalars)"""
        self.ctx = ctx
        self.descs = list(descs)
        self.groups = len(self.descs)
        self.h = C.c_void_p()
        if ep is None:
            _chk(lib().qgemul_plan_create_grouped(ctx.h, _desc_array(self.descs), self.groups, flags, C.byref(self.h)), "qgemul_plan_create_grouped")
        else:
            _chk(lib().qgemul_plan_create_grouped_epx(ctx.h, _desc_array(self.descs), self.groups, C.byref(ep), _ax(approx), _per_member(per_member), flags,
                                                      C.byref(self.h)), "qgemul_plan_create_grouped_epx")
        self.info = qgemul_info()
        _chk(lib().qgemul_plan_info(self.h, C.byref(self.info)), "qgemul_plan_info")

    def close(self):
        if self.h:
            lib().qgemul_plan_destroy(self.h)
            self.h = C.c_void_p()

    @property
    def launches(self) -> int:
        return int(lib().qgemul_plan_grouped_launches(self.h))

    def member(self, g: int) -> qgemul_grouped_member:
        out = qgemul_grouped_member()
        _chk(lib().qgemul_plan_grouped_member(self.h, g, C.byref(out)), "qgemul_plan_grouped_member")
        return out

    def pack(self, operand: int, src_devs, packed_dev: int, ld=None):
        """src_devs: one device pointer per member (0 / None for a member with M == 0 or N == 0); ld: one per member or None (tight)"""
        _chk(lib().qgemul_pack_grouped(self.h, operand, _ptr_array(src_devs), _ld_array(ld, self.groups), C.c_void_p(packed_dev)), "qgemul_pack_grouped")

    def execute(self, pC: int, pA: int, pB: int):
        _chk(lib().qgemul_execute_grouped(self.h, C.c_void_p(pC), C.c_void_p(pA), C.c_void_p(pB)), "qgemul_execute_grouped")

    def unpack_c(self, pC: int, dst_devs, ld=None):
        _chk(lib().qgemul_unpack_c_grouped(self.h, C.c_void_p(pC), _ptr_array(dst_devs), _ld_array(ld, self.groups)), "qgemul_unpack_c_grouped")

    def time_execute(self, pC: int, pA: int, pB: int, warmup: int, iters: int) -> float:
        ms = C.c_float()
        _chk(lib().qgemul_time_execute_grouped(self.h, C.c_void_p(pC), C.c_void_p(pA), C.c_void_p(pB), warmup, iters, C.byref(ms)), "qgemul_time_execute_grouped")
        return ms.value

    # ---- with a chain (ep) ----
    def fuses(self) -> int:
        """1: the chain runs inside the one grouped launch"""
        return int(lib().qgemul_plan_fuses_epilogue(self.h))

    def packed_e_bytes(self, stage: int) -> int:
        """bytes of stage `stage`'s packed tensor operand for the whole group"""
        return int(lib().qgemul_packed_e_bytes(self.h, stage))

    def pack_e(self, stage: int, src_devs, packed_dev: int, ld=None):
        _chk(lib().qgemul_pack_e_grouped(self.h, stage, _ptr_array(src_devs), _ld_array(ld, self.groups), C.c_void_p(packed_dev)), "qgemul_pack_e_grouped")

    def set_scalars(self, stage: int, values):
        """the per-member raw values of scalar stage `stage`, in the caller's member order"""
        assert len(values) == self.groups
        _chk(lib().qgemul_grouped_set_scalars(self.h, stage, (C.c_int64 * self.groups)(*[int(v) for v in values])), "qgemul_grouped_set_scalars")

    def execute_ep(self, pD: int, pA: int, pB: int, args: qgemul_ep_args):
        _chk(lib().qgemul_execute_grouped_ep(self.h, C.c_void_p(pD), C.c_void_p(pA), C.c_void_p(pB), C.byref(args)), "qgemul_execute_grouped_ep")

    def time_execute_ep(self, pD: int, pA: int, pB: int, args: qgemul_ep_args, warmup: int, iters: int) -> float:
        ms = C.c_float()
        _chk(lib().qgemul_time_execute_grouped_ep(self.h, C.c_void_p(pD), C.c_void_p(pA), C.c_void_p(pB), C.byref(args), warmup, iters, C.byref(ms)),
             "qgemul_time_execute_grouped_ep")
        return float(ms.value)
