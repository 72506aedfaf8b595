"""ctypes binding of the C-ABI in include/wavelet_amd.h (libwavelet_amd.so).

This module is the only place Python touches the native library.  It has no
CPU fallback: loading fails loudly if the shared object is missing, and
creating a context fails loudly if no HIP device is visible.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path
from typing import Iterable, Sequence

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
LIB_DIR = PKG_DIR / "lib"
LIB_PATH = LIB_DIR / "libwavelet_amd.so"
HOST_LIB_PATH = LIB_DIR / "libwavelet_amd_host.so"

WC_OK, WC_ERR_INVALID, WC_ERR_HIP, WC_ERR_NOMEM, WC_ERR_FORMAT = 0, 1, 2, 3, 4
WC_F32, WC_F64 = 0, 1

# Every symbol include/wavelet_amd.h declares (checked by tests/test_capi.py).
EXPORTED = (
    "wc_ctx_create", "wc_ctx_destroy", "wc_last_error", "wc_set_stream", "wc_synchronize",
    "wc_payload_bound", "wc_cell_count", "wc_forward", "wc_forward_host", "wc_decompose",
    "wc_inverse", "wc_inverse_host", "wc_inverse_flat", "wc_rmse", "wc_version",
    "wc_profile_enable", "wc_profile_read", "wc_set_option", "wc_inverse_flat_host", "wc_rmse_host",
    "wc_decompose_host", "wc_device_count", "wc_forward_stage", "wc_hist_threshold",
    "wc_forward_emit", "wc_inverse_rmse", "wc_get_option", "wc_rowindex_bytes", "wc_forward_rows",
    "wc_inverse_rows", "wc_forward_host_units", "wc_round_trip_host",
    "wc_tol_threshold", "wc_forward_tol", "wc_forward_emit_tol", "wc_forward_tol_host",
    "wc_levels_for", "wc_payload_levels", "wc_forward_levels", "wc_decompose_levels",
    "wc_inverse_flat_levels", "wc_inverse_levels", "wc_forward_levels_host", "wc_inverse_levels_host",
    "wc_coarse_units", "wc_inverse_coarse", "wc_inverse_coarse_host",
    "wc_tol_levels_threshold", "wc_forward_levels_tol", "wc_forward_levels_tol_host",
    "wc_region_align", "wc_region_units", "wc_inverse_region", "wc_inverse_region_host",
    "wc_budget_thresholds", "wc_budget_select", "wc_forward_levels_budget", "wc_forward_levels_budget_host",
    "wc_pack_value", "wc_packed_tag", "wc_payload_packed", "wc_packed_size", "wc_pack_unit", "wc_unpack_unit",
    "wc_packed_bound", "wc_pack", "wc_unpack", "wc_pack_host", "wc_unpack_host",
    "wc_inverse_packed", "wc_inverse_packed_coarse", "wc_inverse_packed_region",
    "wc_inverse_packed_host", "wc_inverse_packed_coarse_host", "wc_inverse_packed_region_host",
    "wc_thin_unit", "wc_thin_bound", "wc_thin_budget", "wc_thin_thresh", "wc_thin_budget_host", "wc_thin_thresh_host",
    "wc_split_unit", "wc_merge_unit", "wc_split_bound", "wc_merge_bound", "wc_split_budget", "wc_split_thresh",
    "wc_merge", "wc_split_budget_host", "wc_split_thresh_host", "wc_merge_host",
    "wc_thin_tol_unit", "wc_split_tol_unit", "wc_thin_tol", "wc_split_tol", "wc_thin_tol_host", "wc_split_tol_host",
    "wc_maxerr_select", "wc_forward_levels_maxerr", "wc_forward_levels_maxerr_host", "wc_maxerr", "wc_maxerr_host",
)
WC_MAX_LEVELS = 4  # levels of the opt-in multi-level transform (1 = the reference's codec)
WC_PACK_MAX_CELLS = 1 << 21  # the largest unit wc_pack / wc_unpack take (the host rule has no limit)
WC_LTOL_SHIFT = 24  # bins between the walks of two adjacent levels in the multi-level RMSE-tolerance rule
WC_OPT_SPARSE = 12   # sparse coefficient staging in the forward (default 1)
WC_OPT_ORDERED = 13  # look-back tile index from the launch order (1, default) or per-unit tickets (0)
WC_OPT_INVERSE_ROWS = 14  # row-indexed inverse of even-dims units (1, default) or dense decode (0)
WC_OPT_RIX_LDS = 15  # row-indexed inverse: LDS floats per workgroup (default 9216)
WC_OPT_RIX_TX = 16  # row-indexed inverse: log2 of the tile's x blocks (default 4)
WC_OPT_RIX_BLOCKED = 17  # row-indexed inverse: contiguous tile runs per workgroup (default 0)
WC_OPT_HOST_CHUNK = 18  # wc_forward_host: cells per pipelined unit run (default 2^25, 0 = one run)
WC_OPT_SPIN_LIMIT = 19  # polls of an unpublished look-back predecessor before a block derives it itself (0: 64)
WC_OPT_TICKETS = 20  # 1: ticket form whatever WC_OPT_ORDERED says
WC_OPT_REVERSE_TILES = 29  # test hook: each unit's look-back tiles in reverse launch order
WC_OPT_RIX_XCD = 22  # row-indexed inverse tiles dealt to XCDs in contiguous runs (default 0)
WC_OPT_INV_GROUPS = 23  # row-indexed inverse in N unit groups, row index of g+1 beside K6r of g (default 1)
WC_OPT_HOST_THREADS = 27  # _host calls: threads that fault in a copy's host destination first (0 = off)
WC_OPT_HOST_THP = 28  # _host calls: advise huge pages on those destinations (default 0)
WC_OPT_TOL_SOLO_TILES = 30  # RMSE-tolerance mode: flat tiles a unit may have and still be binned by one workgroup (default 64)

# Stage ids of wc_profile_read (include/wavelet_amd.h WC_STAGE_*).
STAGES = ("transform", "emit", "decode", "inverse", "rmse", "hist", "pairs", "tol", "levels", "pack")


class WcUnit(ctypes.Structure):
    """wc_unit: one Box3D component, x fastest (reference src/grid.h:15-19)."""
    _fields_ = [("cell_offset", ctypes.c_uint64), ("nx", ctypes.c_int32),
                ("ny", ctypes.c_int32), ("nz", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class WcRegion(ctypes.Structure):
    """wc_region: origin and extent of a sub-box in full-resolution cells."""
    _fields_ = [("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("z0", ctypes.c_int32),
                ("nx", ctypes.c_int32), ("ny", ctypes.c_int32), ("nz", ctypes.c_int32)]


class WaveletError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"wavelet_amd error {code}: {msg}")
        self.code = code


_lib = None


def load_library() -> ctypes.CDLL:
    """Load libwavelet_amd.so (built by __graft_entry__.build()); raise if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise FileNotFoundError(
            f"{LIB_PATH} is missing: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()')")
    _share_torch_runtime()
    # WCAMD_LIB: another build of the same library (A/B runs of kernel variants)
    L = ctypes.CDLL(os.environ.get("WCAMD_LIB") or str(LIB_PATH))
    vp, u64, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    up = ctypes.POINTER(WcUnit)
    rp = ctypes.POINTER(WcRegion)
    sigs = {
        "wc_ctx_create": (i32, [i32, ctypes.POINTER(vp)]),
        "wc_ctx_destroy": (None, [vp]),
        "wc_last_error": (ctypes.c_char_p, [vp]),
        "wc_set_stream": (i32, [vp, vp]),
        "wc_synchronize": (i32, [vp]),
        "wc_payload_bound": (u64, [up, i32]),
        "wc_cell_count": (u64, [up, i32]),
        "wc_forward": (i32, [vp, vp, i32, up, i32, ctypes.c_double, vp, u64, vp, vp]),
        "wc_forward_host": (i32, [vp, vp, i32, up, i32, ctypes.c_double, vp, u64, vp, vp]),
        "wc_decompose": (i32, [vp, vp, i32, up, i32, vp]),
        "wc_inverse": (i32, [vp, vp, vp, up, i32, vp]),
        "wc_inverse_host": (i32, [vp, vp, vp, up, i32, vp]),
        "wc_inverse_flat": (i32, [vp, vp, up, i32, vp]),
        "wc_inverse_rmse": (i32, [vp, vp, vp, up, i32, vp, i32, vp, vp]),
        "wc_rmse": (i32, [vp, vp, i32, vp, up, i32, vp]),
        "wc_version": (ctypes.c_char_p, []),
        "wc_profile_enable": (i32, [vp, i32]),
        "wc_set_option": (i32, [vp, i32, ctypes.c_int64]),
        "wc_get_option": (i32, [vp, i32, ctypes.POINTER(ctypes.c_int64)]),
        "wc_inverse_flat_host": (i32, [vp, vp, up, i32, vp]),
        "wc_rmse_host": (i32, [vp, vp, i32, vp, up, i32, vp]),
        "wc_decompose_host": (i32, [vp, vp, i32, up, i32, vp]),
        "wc_profile_read": (i32, [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32), i32]),
        "wc_forward_stage": (i32, [vp, vp, i32, up, i32, vp]),
        "wc_hist_threshold": (i32, [vp, ctypes.c_double, ctypes.POINTER(ctypes.c_float),
                                    ctypes.POINTER(ctypes.c_uint64)]),
        "wc_forward_emit": (i32, [vp, up, i32, ctypes.c_double, ctypes.POINTER(ctypes.c_float), vp, u64,
                                  vp, vp]),
        "wc_rowindex_bytes": (u64, [up, i32]),
        "wc_forward_rows": (i32, [vp, vp, i32, up, i32, ctypes.c_double, vp, u64, vp, vp, vp, u64]),
        "wc_inverse_rows": (i32, [vp, vp, vp, up, i32, vp, u64, vp, i32, vp, vp]),
        "wc_forward_host_units": (i32, [vp, ctypes.POINTER(vp), i32, up, i32, ctypes.c_double, vp, u64, vp, vp]),
        "wc_round_trip_host": (i32, [vp, vp, i32, up, i32, ctypes.c_double, vp, u64, vp, vp, vp]),
        "wc_tol_threshold": (i32, [vp, u64, ctypes.c_double, ctypes.POINTER(ctypes.c_float),
                                   ctypes.POINTER(ctypes.c_double)]),
        "wc_forward_tol": (i32, [vp, vp, i32, up, i32, vp, vp, u64, vp, vp, vp, vp]),
        "wc_forward_emit_tol": (i32, [vp, up, i32, vp, vp, u64, vp, vp, vp, vp]),
        "wc_forward_tol_host": (i32, [vp, vp, i32, up, i32, vp, vp, u64, vp, vp, vp, vp, vp]),
        "wc_levels_for": (i32, [i32, i32, i32, i32]),
        "wc_payload_levels": (i32, [vp, ctypes.c_size_t, ctypes.POINTER(i32)]),
        "wc_forward_levels": (i32, [vp, vp, i32, up, i32, vp, ctypes.c_double, ctypes.POINTER(ctypes.c_float), vp,
                                    u64, vp, vp]),
        "wc_decompose_levels": (i32, [vp, vp, i32, up, i32, vp, vp]),
        "wc_inverse_flat_levels": (i32, [vp, vp, up, i32, vp, vp]),
        "wc_inverse_levels": (i32, [vp, vp, vp, up, i32, vp, vp]),
        "wc_forward_levels_host": (i32, [vp, vp, i32, up, i32, vp, ctypes.c_double, ctypes.POINTER(ctypes.c_float),
                                         vp, u64, vp, vp]),
        "wc_inverse_levels_host": (i32, [vp, vp, vp, up, i32, vp, vp]),
        "wc_coarse_units": (i32, [up, vp, i32, up, ctypes.POINTER(u64)]),
        "wc_inverse_coarse": (i32, [vp, vp, vp, up, i32, vp, vp, up, vp]),
        "wc_inverse_coarse_host": (i32, [vp, vp, vp, up, i32, vp, vp, up, vp]),
        "wc_tol_levels_threshold": (i32, [vp, i32, u64, ctypes.c_double, ctypes.POINTER(ctypes.c_float),
                                          ctypes.POINTER(ctypes.c_double)]),
        "wc_forward_levels_tol": (i32, [vp, vp, i32, up, i32, vp, vp, vp, u64, vp, vp, vp, vp]),
        "wc_forward_levels_tol_host": (i32, [vp, vp, i32, up, i32, vp, vp, vp, u64, vp, vp, vp, vp, vp]),
        "wc_budget_thresholds": (i32, [ctypes.c_uint32, i32, ctypes.POINTER(ctypes.c_float)]),
        "wc_budget_select": (i32, [vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, i32, ctypes.c_uint32,
                                   ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_float),
                                   ctypes.POINTER(ctypes.c_uint32)]),
        "wc_forward_levels_budget": (i32, [vp, vp, i32, up, i32, vp, vp, vp, u64, vp, vp, vp, vp]),
        "wc_maxerr_select": (i32, [vp, vp, i32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, i32, ctypes.c_double,
                                   vp, vp, vp]),
        "wc_forward_levels_maxerr": (i32, [vp, vp, i32, up, i32, vp, vp, vp, u64, vp, vp, vp, vp]),
        "wc_forward_levels_maxerr_host": (i32, [vp, vp, i32, up, i32, vp, vp, vp, u64, vp, vp, vp, vp, vp]),
        "wc_maxerr": (i32, [vp, vp, i32, vp, up, i32, vp]),
        "wc_maxerr_host": (i32, [vp, vp, i32, vp, up, i32, vp]),
        "wc_forward_levels_budget_host": (i32, [vp, vp, i32, up, i32, vp, vp, vp, u64, vp, vp, vp, vp, vp]),
        "wc_region_align": (i32, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, i32, rp, rp]),
        "wc_region_units": (i32, [up, rp, vp, i32, up, ctypes.POINTER(u64)]),
        "wc_inverse_region": (i32, [vp, vp, vp, up, i32, vp, vp, rp, up, vp]),
        "wc_inverse_region_host": (i32, [vp, vp, vp, up, i32, vp, vp, rp, up, vp]),
        "wc_pack_value": (ctypes.c_uint32, [ctypes.c_uint32, i32]),
        "wc_packed_tag": (ctypes.c_int32, [i32, i32]),
        "wc_payload_packed": (i32, [vp, ctypes.c_size_t, ctypes.POINTER(i32), ctypes.POINTER(i32)]),
        "wc_packed_size": (i32, [vp, ctypes.c_size_t, ctypes.POINTER(u64)]),
        "wc_pack_unit": (i32, [vp, ctypes.c_size_t, i32, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
        "wc_unpack_unit": (i32, [vp, ctypes.c_size_t, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
        "wc_packed_bound": (i32, [up, i32, i32, ctypes.POINTER(u64)]),
        "wc_pack": (i32, [vp, vp, vp, up, i32, i32, vp, u64, vp, vp]),
        "wc_unpack": (i32, [vp, vp, vp, u64, up, i32, vp, u64, vp, vp]),
        "wc_pack_host": (i32, [vp, vp, vp, up, i32, i32, vp, u64, vp, vp]),
        "wc_unpack_host": (i32, [vp, vp, vp, up, i32, vp, u64, vp, vp]),
        "wc_inverse_packed": (i32, [vp, vp, vp, u64, up, i32, vp, vp]),
        "wc_inverse_packed_coarse": (i32, [vp, vp, vp, u64, up, i32, vp, vp, up, vp]),
        "wc_inverse_packed_region": (i32, [vp, vp, vp, u64, up, i32, vp, vp, rp, up, vp]),
        "wc_inverse_packed_host": (i32, [vp, vp, vp, up, i32, vp, vp]),
        "wc_inverse_packed_coarse_host": (i32, [vp, vp, vp, up, i32, vp, vp, up, vp]),
        "wc_inverse_packed_region_host": (i32, [vp, vp, vp, up, i32, vp, vp, rp, up, vp]),
        "wc_thin_unit": (i32, [vp, ctypes.c_size_t, vp, vp, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                               ctypes.POINTER(ctypes.c_uint32), vp]),
        "wc_thin_bound": (u64, [up, i32, vp]),
        "wc_thin_budget": (i32, [vp, vp, vp, up, i32, vp, vp, vp, u64, vp, vp, vp, vp]),
        "wc_thin_thresh": (i32, [vp, vp, vp, up, i32, vp, vp, vp, u64, vp, vp]),
        "wc_thin_budget_host": (i32, [vp, vp, vp, up, i32, vp, vp, vp, u64, vp, vp, vp, vp]),
        "wc_thin_thresh_host": (i32, [vp, vp, vp, up, i32, vp, vp, vp, u64, vp, vp]),
        "wc_thin_tol_unit": (i32, [vp, ctypes.c_size_t, ctypes.c_double, vp, ctypes.c_size_t,
                                   ctypes.POINTER(ctypes.c_size_t), vp, ctypes.POINTER(ctypes.c_double)]),
        "wc_split_tol_unit": (i32, [vp, ctypes.c_size_t, ctypes.c_double, vp, ctypes.c_size_t,
                                    ctypes.POINTER(ctypes.c_size_t), vp, ctypes.c_size_t,
                                    ctypes.POINTER(ctypes.c_size_t), vp, ctypes.POINTER(ctypes.c_double)]),
        "wc_thin_tol": (i32, [vp, vp, vp, up, i32, vp, vp, vp, u64, vp, vp, vp, vp]),
        "wc_thin_tol_host": (i32, [vp, vp, vp, up, i32, vp, vp, vp, u64, vp, vp, vp, vp]),
        "wc_split_tol": (i32, [vp, vp, vp, up, i32, vp, vp, vp, u64, vp, vp, vp, u64, vp, vp, vp, vp]),
        "wc_split_tol_host": (i32, [vp, vp, vp, up, i32, vp, vp, vp, u64, vp, vp, vp, u64, vp, vp, vp, vp]),
        "wc_split_unit": (i32, [vp, ctypes.c_size_t, vp, vp, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_uint32),
                                vp]),
        "wc_merge_unit": (i32, [vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp, ctypes.c_size_t,
                                ctypes.POINTER(ctypes.c_size_t)]),
        "wc_split_bound": (i32, [up, i32, vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        "wc_merge_bound": (u64, [up, i32]),
        "wc_split_budget": (i32, [vp, vp, vp, up, i32, vp, vp, vp, u64, vp, vp, vp, u64, vp, vp, vp, vp]),
        "wc_split_thresh": (i32, [vp, vp, vp, up, i32, vp, vp, vp, u64, vp, vp, vp, u64, vp, vp]),
        "wc_merge": (i32, [vp, vp, vp, vp, vp, up, i32, vp, vp, u64, vp, vp]),
        "wc_split_budget_host": (i32, [vp, vp, vp, up, i32, vp, vp, vp, u64, vp, vp, vp, u64, vp, vp, vp, vp]),
        "wc_split_thresh_host": (i32, [vp, vp, vp, up, i32, vp, vp, vp, u64, vp, vp, vp, u64, vp, vp]),
        "wc_merge_host": (i32, [vp, vp, vp, vp, vp, up, i32, vp, vp, u64, vp, vp]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def make_units(dims: Sequence[Sequence[int]], offsets: Iterable[int] | None = None,
               align: int = 4):
    """Build a wc_unit array for boxes of `dims` = [(W, H, D), ...].

    Without explicit offsets the boxes are packed back to back, each start
    rounded up to `align` elements (vector loads stay aligned)."""
    n = len(dims)
    arr = (WcUnit * max(n, 1))()
    cur = 0
    offs = list(offsets) if offsets is not None else None
    for i, (W, H, D) in enumerate(dims):
        if offs is None:
            cur = (cur + align - 1) // align * align
            off = cur
            cur += W * H * D
        else:
            off = offs[i]
        arr[i] = WcUnit(off, W, H, D, 0)
    extent = max((arr[i].cell_offset + arr[i].nx * arr[i].ny * arr[i].nz for i in range(n)), default=0)
    return arr, n, int(extent)


def payload_bound(units, n) -> int:
    return int(load_library().wc_payload_bound(units, n))


def rowindex_bytes(units, n) -> int:
    """Bytes of a batch's row index (wc_rowindex_bytes: W*H + 1 entries of 8 B per unit
    with cells, none for an empty unit)."""
    return int(load_library().wc_rowindex_bytes(units, n))


def _share_torch_runtime():
    """torch ships its own HIP runtime (torch/lib/libamdhip64.so, SONAME
    libamdhip64.so.7, ROCm 7.0) beside the system one this library links
    (/opt/rocm/lib/libamdhip64.so.7).  If torch is loaded first, the dynamic
    loader resolves our NEEDED libamdhip64.so.7 to torch's copy and the process
    has ONE HIP runtime; loaded the other way round there would be two, and
    only the first to initialise gets the GPU.  So import torch (if present)
    before dlopen-ing the library.  Set WCAMD_NO_TORCH=1 to skip (torch-free
    processes then use the system ROCm runtime)."""
    if os.environ.get("WCAMD_NO_TORCH") == "1":
        return
    try:
        import torch  # noqa: F401
    except Exception:
        pass


class Context:
    """One wc_ctx: a HIP device, its stream and its HBM scratch."""

    def __init__(self, device: int = 0):
        L = load_library()
        h = ctypes.c_void_p()
        rc = L.wc_ctx_create(int(device), ctypes.byref(h))
        if rc != WC_OK:
            raise WaveletError(rc, f"wc_ctx_create(device={device}) failed: no usable HIP device")
        self._h = h
        self.device = device
        self._L = L

    def close(self):
        if self._h:
            self._L.wc_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != WC_OK:
            raise WaveletError(rc, self._L.wc_last_error(self._h).decode())

    @property
    def handle(self):
        return self._h

    def set_stream(self, stream_ptr: int | None):
        self._check(self._L.wc_set_stream(self._h, ctypes.c_void_p(stream_ptr or 0)))

    def synchronize(self):
        self._check(self._L.wc_synchronize(self._h))

    def set_option(self, option: int, value: int):
        self._check(self._L.wc_set_option(self._h, int(option), int(value)))

    def get_option(self, option: int) -> int:
        v = ctypes.c_int64()
        self._check(self._L.wc_get_option(self._h, int(option), ctypes.byref(v)))
        return int(v.value)

    def profile_enable(self, on: bool = True):
        self._check(self._L.wc_profile_enable(self._h, 1 if on else 0))

    def profile_read(self) -> dict:
        """{stage: (total_ms, launches)} since the previous read (hipEvent timing)."""
        n = len(STAGES)
        ms = (ctypes.c_double * n)()
        cnt = (ctypes.c_uint32 * n)()
        self._check(self._L.wc_profile_read(self._h, ms, cnt, n))
        return {STAGES[i]: (ms[i], cnt[i]) for i in range(n) if cnt[i]}

    # ---- device-pointer API (torch tensors or raw ints) ------------------
    def forward(self, d_cells: int, dtype: int, units, n: int, keep: float, d_payload: int,
                capacity: int, d_offsets: int, d_kept: int):
        self._check(self._L.wc_forward(self._h, ctypes.c_void_p(d_cells), dtype, units, n,
                                       float(keep), ctypes.c_void_p(d_payload), capacity,
                                       ctypes.c_void_p(d_offsets), ctypes.c_void_p(d_kept)))

    def forward_rows(self, d_cells: int, dtype: int, units, n: int, keep: float, d_payload: int,
                     capacity: int, d_offsets: int, d_kept: int, d_rowinfo: int, rowinfo_capacity: int):
        """wc_forward that also writes the payloads' row index (include/wavelet_amd.h)."""
        self._check(self._L.wc_forward_rows(self._h, ctypes.c_void_p(d_cells), dtype, units, n, float(keep),
                                            ctypes.c_void_p(d_payload), capacity, ctypes.c_void_p(d_offsets),
                                            ctypes.c_void_p(d_kept), ctypes.c_void_p(d_rowinfo), rowinfo_capacity))

    def inverse_rows(self, d_payload: int, d_offsets: int, units, n: int, d_rowinfo: int | None, d_out: int,
                     d_orig: int | None = None, dtype: int = WC_F32, d_rmse: int | None = None,
                     rowinfo_capacity: int | None = None):
        """wc_inverse (d_orig None) or wc_inverse_rmse with the row index of
        wc_forward_rows (d_rowinfo None: derived from the payloads).
        rowinfo_capacity: bytes of the d_rowinfo buffer (default: exactly
        rowindex_bytes(units, n), the size forward_rows needs)."""
        cap = rowinfo_capacity if rowinfo_capacity is not None else (rowindex_bytes(units, n) if d_rowinfo else 0)
        self._check(self._L.wc_inverse_rows(self._h, ctypes.c_void_p(d_payload), ctypes.c_void_p(d_offsets),
                                            units, n, ctypes.c_void_p(d_rowinfo or 0), cap,
                                            ctypes.c_void_p(d_orig or 0), dtype, ctypes.c_void_p(d_out),
                                            ctypes.c_void_p(d_rmse or 0)))

    def forward_stage(self, d_cells: int, dtype: int, units, n: int, d_hist: int | None = None):
        """Global-threshold mode, step 1 (include/wavelet_amd.h): transform into
        the context scratch; add the magnitude histogram to d_hist if given."""
        self._check(self._L.wc_forward_stage(self._h, ctypes.c_void_p(d_cells), dtype, units, n,
                                             ctypes.c_void_p(d_hist or 0)))

    def forward_emit(self, units, n: int, keep: float, thresh: float | None, d_payload: int,
                     capacity: int, d_offsets: int, d_kept: int):
        """Step 2: pack the staged batch with one fp32 threshold (None: the
        reference's per-unit rule with `keep`)."""
        t = None if thresh is None else ctypes.byref(ctypes.c_float(thresh))
        self._check(self._L.wc_forward_emit(self._h, units, n, float(keep), t, ctypes.c_void_p(d_payload),
                                            capacity, ctypes.c_void_p(d_offsets), ctypes.c_void_p(d_kept)))

    def forward_tol(self, d_cells: int, dtype: int, units, n: int, tol, d_payload: int, capacity: int,
                    d_offsets: int, d_kept: int, d_thresh: int | None = None, d_bound: int | None = None):
        """wc_forward with per-unit RMSE tolerances (n host doubles) in place of
        keep; d_thresh (n floats) / d_bound (n doubles): optional device outputs."""
        t = _tol_array(tol, n)
        self._check(self._L.wc_forward_tol(self._h, ctypes.c_void_p(d_cells), dtype, units, n, t.ctypes.data,
                                           ctypes.c_void_p(d_payload), capacity, ctypes.c_void_p(d_offsets),
                                           ctypes.c_void_p(d_kept), ctypes.c_void_p(d_thresh or 0),
                                           ctypes.c_void_p(d_bound or 0)))

    def forward_emit_tol(self, units, n: int, tol, d_payload: int, capacity: int, d_offsets: int, d_kept: int,
                         d_thresh: int | None = None, d_bound: int | None = None):
        """The staged form of forward_tol, after forward_stage(..., None); may be
        repeated with other tolerances on the same staged batch."""
        t = _tol_array(tol, n)
        self._check(self._L.wc_forward_emit_tol(self._h, units, n, t.ctypes.data, ctypes.c_void_p(d_payload),
                                                capacity, ctypes.c_void_p(d_offsets), ctypes.c_void_p(d_kept),
                                                ctypes.c_void_p(d_thresh or 0), ctypes.c_void_p(d_bound or 0)))

    def forward_levels(self, d_cells: int, dtype: int, units, n: int, levels, keep: float, thresh: float | None,
                       d_payload: int, capacity: int, d_offsets: int, d_kept: int):
        """wc_forward with levels[u] transform levels per unit (n host ints, or one
        value for all); thresh None: the keep rule on the final array, else one
        fp32 threshold.  Units with L >= 2 write ncoeff = -L in their headers."""
        lv = _levels_array(levels, n)
        t = None if thresh is None else ctypes.byref(ctypes.c_float(thresh))
        self._check(self._L.wc_forward_levels(self._h, ctypes.c_void_p(d_cells), dtype, units, n, lv.ctypes.data,
                                              float(keep), t, ctypes.c_void_p(d_payload), capacity,
                                              ctypes.c_void_p(d_offsets), ctypes.c_void_p(d_kept)))

    def forward_levels_tol(self, d_cells: int, dtype: int, units, n: int, levels, tol, d_payload: int, capacity: int,
                           d_offsets: int, d_kept: int, d_thresh: int | None = None, d_bound: int | None = None):
        """wc_forward_levels with per-unit RMSE tolerances (n host doubles) in place
        of keep / thresh: one threshold per level.  d_thresh (n x WC_MAX_LEVELS
        floats, level l of unit u at u * WC_MAX_LEVELS + l - 1) / d_bound (n
        doubles): optional device outputs."""
        lv = _levels_array(levels, n)
        t = _tol_array(tol, n)
        self._check(self._L.wc_forward_levels_tol(self._h, ctypes.c_void_p(d_cells), dtype, units, n, lv.ctypes.data,
                                                  t.ctypes.data, ctypes.c_void_p(d_payload), capacity,
                                                  ctypes.c_void_p(d_offsets), ctypes.c_void_p(d_kept),
                                                  ctypes.c_void_p(d_thresh or 0), ctypes.c_void_p(d_bound or 0)))

    def forward_levels_budget(self, d_cells: int, dtype: int, units, n: int, levels, max_pairs, d_payload: int,
                              capacity: int, d_offsets: int, d_kept: int, d_thresh: int | None = None,
                              d_key: int | None = None):
        """wc_forward_levels with per-unit pair budgets (n host uint32, or one value
        for all) in place of keep / thresh: each unit keeps its max_pairs largest
        weighted coefficients and never more.  levels None: all 1.  d_thresh (n x
        WC_MAX_LEVELS floats) / d_key (n uint32, the units' T): optional device
        outputs."""
        lv = None if levels is None else _levels_array(levels, n)
        k = _pairs_array(max_pairs, n)
        self._check(self._L.wc_forward_levels_budget(self._h, ctypes.c_void_p(d_cells), dtype, units, n,
                                                     None if lv is None else lv.ctypes.data, k.ctypes.data,
                                                     ctypes.c_void_p(d_payload), capacity, ctypes.c_void_p(d_offsets),
                                                     ctypes.c_void_p(d_kept), ctypes.c_void_p(d_thresh or 0),
                                                     ctypes.c_void_p(d_key or 0)))

    def forward_levels_maxerr(self, d_cells: int, dtype: int, units, n: int, levels, maxerr, d_payload: int,
                              capacity: int, d_offsets: int, d_kept: int, d_thresh: int | None = None,
                              d_err: int | None = None):
        """wc_forward_levels with per-unit pointwise error bounds (n host doubles, or
        one value for all) in place of keep / thresh: no cell of a unit's
        reconstruction is further than its bound from the original (verified on
        the device).  levels None: all 1.  d_thresh (n floats, ONE per unit) /
        d_err (n doubles, the achieved max error): optional device outputs."""
        lv = None if levels is None else _levels_array(levels, n)
        t = _tol_array(maxerr, n)
        self._check(self._L.wc_forward_levels_maxerr(self._h, ctypes.c_void_p(d_cells), dtype, units, n,
                                                     None if lv is None else lv.ctypes.data, t.ctypes.data,
                                                     ctypes.c_void_p(d_payload), capacity, ctypes.c_void_p(d_offsets),
                                                     ctypes.c_void_p(d_kept), ctypes.c_void_p(d_thresh or 0),
                                                     ctypes.c_void_p(d_err or 0)))

    def maxerr(self, d_orig: int, dtype: int, d_regen: int, units, n: int, d_err: int):
        """wc_maxerr: per unit the max of |orig - regen| over the non-NaN differences (n device doubles)."""
        self._check(self._L.wc_maxerr(self._h, ctypes.c_void_p(d_orig), dtype, ctypes.c_void_p(d_regen), units, n,
                                      ctypes.c_void_p(d_err)))

    def thin_budget(self, d_payload: int, d_offsets: int, units, n: int, levels, max_pairs, d_out: int,
                    capacity: int, d_out_offsets: int, d_kept: int, d_thresh: int | None = None,
                    d_key: int | None = None):
        """wc_thin_budget: standard payloads -> the payloads of a tighter pair budget, in
        the compressed domain.  Slots of 24 + 8 min(max_pairs, N) bytes (thin_bound)."""
        lv = _levels_array(levels, n)
        k = _pairs_array(max_pairs, n)
        self._check(self._L.wc_thin_budget(self._h, ctypes.c_void_p(d_payload), ctypes.c_void_p(d_offsets), units, n,
                                           lv.ctypes.data, k.ctypes.data, ctypes.c_void_p(d_out), int(capacity),
                                           ctypes.c_void_p(d_out_offsets), ctypes.c_void_p(d_kept),
                                           ctypes.c_void_p(d_thresh or 0), ctypes.c_void_p(d_key or 0)))

    def thin_thresh(self, d_payload: int, d_offsets: int, units, n: int, levels, thresh, d_out: int, capacity: int,
                    d_out_offsets: int, d_kept: int):
        """wc_thin_thresh: standard payloads -> what |c| > thresh[u][lvl - 1] keeps of them
        (thresh: n x WC_MAX_LEVELS host floats).  wc_forward's slot layout."""
        lv = _levels_array(levels, n)
        t = _thin_thresh_array(thresh, n)
        self._check(self._L.wc_thin_thresh(self._h, ctypes.c_void_p(d_payload), ctypes.c_void_p(d_offsets), units, n,
                                           lv.ctypes.data, t.ctypes.data, ctypes.c_void_p(d_out), int(capacity),
                                           ctypes.c_void_p(d_out_offsets), ctypes.c_void_p(d_kept)))

    def thin_tol(self, d_payload: int, d_offsets: int, units, n: int, levels, tol, d_out: int, capacity: int,
                 d_out_offsets: int, d_kept: int, d_thresh: int | None = None, d_bound: int | None = None):
        """wc_thin_tol: standard payloads -> what wc_forward_levels_tol's rule keeps of them
        at the per-unit RMSE tolerances tol (host doubles).  wc_forward's slot layout."""
        lv = _levels_array(levels, n)
        t = _tol_array(tol, n)
        self._check(self._L.wc_thin_tol(self._h, ctypes.c_void_p(d_payload), ctypes.c_void_p(d_offsets), units, n,
                                        lv.ctypes.data, t.ctypes.data, ctypes.c_void_p(d_out), int(capacity),
                                        ctypes.c_void_p(d_out_offsets), ctypes.c_void_p(d_kept),
                                        ctypes.c_void_p(d_thresh or 0), ctypes.c_void_p(d_bound or 0)))

    def split_tol(self, d_payload: int, d_offsets: int, units, n: int, levels, tol, d_base: int,
                  base_capacity: int, d_base_offsets: int, d_kept: int, d_rest: int, rest_capacity: int,
                  d_rest_offsets: int, d_rest_pairs: int, d_thresh: int | None = None, d_bound: int | None = None):
        """wc_split_tol: base is thin_tol's output, rest the other candidates."""
        lv = _levels_array(levels, n)
        t = _tol_array(tol, n)
        self._check(self._L.wc_split_tol(self._h, ctypes.c_void_p(d_payload), ctypes.c_void_p(d_offsets), units, n,
                                         lv.ctypes.data, t.ctypes.data, ctypes.c_void_p(d_base), int(base_capacity),
                                         ctypes.c_void_p(d_base_offsets), ctypes.c_void_p(d_kept),
                                         ctypes.c_void_p(d_rest), int(rest_capacity),
                                         ctypes.c_void_p(d_rest_offsets), ctypes.c_void_p(d_rest_pairs),
                                         ctypes.c_void_p(d_thresh or 0), ctypes.c_void_p(d_bound or 0)))

    def split_budget(self, d_payload: int, d_offsets: int, units, n: int, levels, max_pairs, d_base: int,
                     base_capacity: int, d_base_offsets: int, d_kept: int, d_rest: int, rest_capacity: int,
                     d_rest_offsets: int, d_rest_pairs: int, d_thresh: int | None = None, d_key: int | None = None):
        """wc_split_budget: standard payloads -> (base, rest): base is thin_budget's
        output, rest the other candidates.  Slots as split_bound gives them."""
        lv = _levels_array(levels, n)
        k = _pairs_array(max_pairs, n)
        self._check(self._L.wc_split_budget(self._h, ctypes.c_void_p(d_payload), ctypes.c_void_p(d_offsets), units, n,
                                            lv.ctypes.data, k.ctypes.data, ctypes.c_void_p(d_base), int(base_capacity),
                                            ctypes.c_void_p(d_base_offsets), ctypes.c_void_p(d_kept),
                                            ctypes.c_void_p(d_rest), int(rest_capacity),
                                            ctypes.c_void_p(d_rest_offsets), ctypes.c_void_p(d_rest_pairs),
                                            ctypes.c_void_p(d_thresh or 0), ctypes.c_void_p(d_key or 0)))

    def split_thresh(self, d_payload: int, d_offsets: int, units, n: int, levels, thresh, d_base: int,
                     base_capacity: int, d_base_offsets: int, d_kept: int, d_rest: int, rest_capacity: int,
                     d_rest_offsets: int, d_rest_pairs: int):
        """wc_split_thresh: base is thin_thresh's output (thresh: n x WC_MAX_LEVELS host
        floats), rest the candidates at or below their level's threshold."""
        lv = _levels_array(levels, n)
        t = _thin_thresh_array(thresh, n)
        self._check(self._L.wc_split_thresh(self._h, ctypes.c_void_p(d_payload), ctypes.c_void_p(d_offsets), units, n,
                                            lv.ctypes.data, t.ctypes.data, ctypes.c_void_p(d_base), int(base_capacity),
                                            ctypes.c_void_p(d_base_offsets), ctypes.c_void_p(d_kept),
                                            ctypes.c_void_p(d_rest), int(rest_capacity),
                                            ctypes.c_void_p(d_rest_offsets), ctypes.c_void_p(d_rest_pairs)))

    def merge(self, d_a: int, d_a_offsets: int, d_b: int, d_b_offsets: int, units, n: int, levels, d_out: int,
              capacity: int, d_out_offsets: int, d_pairs: int):
        """wc_merge: the union of two standard payloads per unit (disjoint positions).
        wc_forward's slot layout (merge_bound)."""
        lv = _levels_array(levels, n)
        self._check(self._L.wc_merge(self._h, ctypes.c_void_p(d_a), ctypes.c_void_p(d_a_offsets), ctypes.c_void_p(d_b),
                                     ctypes.c_void_p(d_b_offsets), units, n, lv.ctypes.data, ctypes.c_void_p(d_out),
                                     int(capacity), ctypes.c_void_p(d_out_offsets), ctypes.c_void_p(d_pairs)))

    def decompose_levels(self, d_cells: int, dtype: int, units, n: int, levels, d_flat: int):
        lv = _levels_array(levels, n)
        self._check(self._L.wc_decompose_levels(self._h, ctypes.c_void_p(d_cells), dtype, units, n, lv.ctypes.data,
                                                ctypes.c_void_p(d_flat)))

    def inverse_flat_levels(self, d_flat: int, units, n: int, levels, d_out: int):
        lv = _levels_array(levels, n)
        self._check(self._L.wc_inverse_flat_levels(self._h, ctypes.c_void_p(d_flat), units, n, lv.ctypes.data,
                                                   ctypes.c_void_p(d_out)))

    def inverse_levels(self, d_payload: int, d_offsets: int, units, n: int, levels, d_out: int):
        """wc_inverse of multi-level payloads: unit u's header must carry levels[u]."""
        lv = _levels_array(levels, n)
        self._check(self._L.wc_inverse_levels(self._h, ctypes.c_void_p(d_payload), ctypes.c_void_p(d_offsets),
                                              units, n, lv.ctypes.data, ctypes.c_void_p(d_out)))

    def inverse_coarse(self, d_payload: int, d_offsets: int, units, n: int, levels, reduce, out_units, d_out: int):
        """wc_inverse_coarse: unit u at 1/2^reduce[u] resolution into out_units[u]
        (coarse_units, or the caller's offsets with the same dims).  levels None:
        all 1; levels and reduce: n host ints, or one value for all."""
        lv = None if levels is None else _levels_array(levels, n)
        rd = _levels_array(reduce, n)
        self._check(self._L.wc_inverse_coarse(self._h, ctypes.c_void_p(d_payload), ctypes.c_void_p(d_offsets), units,
                                              n, None if lv is None else lv.ctypes.data, rd.ctypes.data, out_units,
                                              ctypes.c_void_p(d_out)))

    def inverse_region(self, d_payload: int, d_offsets: int, units, n: int, levels, reduce, regions, out_units,
                       d_out: int):
        """wc_inverse_region: the cells of regions[u] of unit u at 1/2^reduce[u]
        resolution into out_units[u] (region_units, or the caller's offsets with
        the same dims).  levels None: all 1; reduce None: all 0; regions: a
        WcRegion array or n (x0, y0, z0, nx, ny, nz) rows."""
        lv = None if levels is None else _levels_array(levels, n)
        rd = None if reduce is None else _levels_array(reduce, n)
        self._check(self._L.wc_inverse_region(self._h, ctypes.c_void_p(d_payload), ctypes.c_void_p(d_offsets), units,
                                              n, None if lv is None else lv.ctypes.data,
                                              None if rd is None else rd.ctypes.data, make_regions(regions, n),
                                              out_units, ctypes.c_void_p(d_out)))

    def pack(self, d_payload: int, d_offsets: int, units, n: int, vbytes: int, d_packed: int, capacity: int,
             d_packed_offsets: int, d_packed_bytes: int):
        """wc_pack: standard payloads -> packed units in their slots (packed_bound);
        d_packed_offsets: n + 1 uint64, d_packed_bytes: n uint64 (exact lengths)."""
        self._check(self._L.wc_pack(self._h, ctypes.c_void_p(d_payload), ctypes.c_void_p(d_offsets), units, n,
                                    int(vbytes), ctypes.c_void_p(d_packed), int(capacity),
                                    ctypes.c_void_p(d_packed_offsets), ctypes.c_void_p(d_packed_bytes)))

    def unpack(self, d_packed: int, d_packed_offsets: int, packed_capacity: int, units, n: int, d_payload: int,
               capacity: int, d_offsets: int, d_kept: int):
        """wc_unpack: packed units -> standard payloads in the forward's slot layout
        (payload_bound), values q(v), runs unchanged."""
        self._check(self._L.wc_unpack(self._h, ctypes.c_void_p(d_packed), ctypes.c_void_p(d_packed_offsets),
                                      int(packed_capacity), units, n, ctypes.c_void_p(d_payload), int(capacity),
                                      ctypes.c_void_p(d_offsets), ctypes.c_void_p(d_kept)))

    def inverse_packed(self, d_packed: int, d_packed_offsets: int, packed_capacity: int, units, n: int, levels,
                       d_out: int):
        """wc_inverse_packed: packed units -> boxes, bit for bit unpack +
        inverse_levels without the standard payloads.  levels None: all 1."""
        lv = None if levels is None else _levels_array(levels, n)
        self._check(self._L.wc_inverse_packed(self._h, ctypes.c_void_p(d_packed), ctypes.c_void_p(d_packed_offsets),
                                              int(packed_capacity), units, n, None if lv is None else lv.ctypes.data,
                                              ctypes.c_void_p(d_out)))

    def inverse_packed_coarse(self, d_packed: int, d_packed_offsets: int, packed_capacity: int, units, n: int, levels,
                              reduce, out_units, d_out: int):
        """wc_inverse_packed_coarse: inverse_coarse with packed units as its source."""
        lv = None if levels is None else _levels_array(levels, n)
        rd = _levels_array(reduce, n)
        self._check(self._L.wc_inverse_packed_coarse(self._h, ctypes.c_void_p(d_packed),
                                                     ctypes.c_void_p(d_packed_offsets), int(packed_capacity), units, n,
                                                     None if lv is None else lv.ctypes.data, rd.ctypes.data, out_units,
                                                     ctypes.c_void_p(d_out)))

    def inverse_packed_region(self, d_packed: int, d_packed_offsets: int, packed_capacity: int, units, n: int, levels,
                              reduce, regions, out_units, d_out: int):
        """wc_inverse_packed_region: inverse_region with packed units as its source."""
        lv = None if levels is None else _levels_array(levels, n)
        rd = None if reduce is None else _levels_array(reduce, n)
        self._check(self._L.wc_inverse_packed_region(self._h, ctypes.c_void_p(d_packed),
                                                     ctypes.c_void_p(d_packed_offsets), int(packed_capacity), units, n,
                                                     None if lv is None else lv.ctypes.data,
                                                     None if rd is None else rd.ctypes.data, make_regions(regions, n),
                                                     out_units, ctypes.c_void_p(d_out)))

    def decompose(self, d_cells: int, dtype: int, units, n: int, d_flat: int):
        self._check(self._L.wc_decompose(self._h, ctypes.c_void_p(d_cells), dtype, units, n,
                                         ctypes.c_void_p(d_flat)))

    def inverse(self, d_payload: int, d_offsets: int, units, n: int, d_out: int):
        self._check(self._L.wc_inverse(self._h, ctypes.c_void_p(d_payload), ctypes.c_void_p(d_offsets),
                                       units, n, ctypes.c_void_p(d_out)))

    def inverse_rmse(self, d_payload: int, d_offsets: int, units, n: int, d_orig: int, dtype: int, d_out: int,
                     d_rmse: int):
        """inverse + rmse fused (include/wavelet_amd.h wc_inverse_rmse)."""
        self._check(self._L.wc_inverse_rmse(self._h, ctypes.c_void_p(d_payload), ctypes.c_void_p(d_offsets),
                                            units, n, ctypes.c_void_p(d_orig), dtype, ctypes.c_void_p(d_out),
                                            ctypes.c_void_p(d_rmse)))

    def inverse_flat(self, d_flat: int, units, n: int, d_out: int):
        self._check(self._L.wc_inverse_flat(self._h, ctypes.c_void_p(d_flat), units, n,
                                            ctypes.c_void_p(d_out)))

    def rmse(self, d_orig: int, dtype: int, d_regen: int, units, n: int, d_rmse: int):
        self._check(self._L.wc_rmse(self._h, ctypes.c_void_p(d_orig), dtype, ctypes.c_void_p(d_regen),
                                    units, n, ctypes.c_void_p(d_rmse)))

    # ---- host-array API ---------------------------------------------------
    def forward_host(self, cells: np.ndarray, units, n: int, keep: float, out=None):
        """cells: flat host array (float32 or float64) -> (payload bytes, offsets, kept).
        out: optional (payload uint8[>= payload_bound], offsets uint64[n + 1],
        kept uint32[>= n]) to fill instead of new arrays (a caller that streams
        batches reuses its buffers: no page faults, no frees per call)."""
        c = np.ascontiguousarray(cells)
        dtype = WC_F64 if c.dtype == np.float64 else WC_F32
        if c.dtype not in (np.float32, np.float64):
            raise TypeError("cells must be float32 or float64")
        cap = payload_bound(units, n)
        if out is None:
            payload = np.empty(cap, np.uint8)
            offsets = np.zeros(n + 1, np.uint64)
            kept = np.zeros(max(n, 1), np.uint32)
        else:
            payload, offsets, kept = out
            if (payload.dtype != np.uint8 or payload.size < cap or not payload.flags.c_contiguous
                    or offsets.dtype != np.uint64 or offsets.size < n + 1 or not offsets.flags.c_contiguous
                    or kept.dtype != np.uint32 or kept.size < n or not kept.flags.c_contiguous):
                raise ValueError("out: (uint8[>= payload_bound], uint64[n + 1], uint32[n]) contiguous arrays")
            cap = payload.size
        self._check(self._L.wc_forward_host(self._h, c.ctypes.data, dtype, units, n, float(keep),
                                            payload.ctypes.data, cap, offsets.ctypes.data,
                                            kept.ctypes.data))
        return payload, offsets, kept[:n]

    def round_trip_host(self, cells: np.ndarray, units, n: int, keep: float):
        """wc_round_trip_host: forward_host's (payload, offsets, kept) and the
        per-unit RMSE of the reconstruction (computed on the device)."""
        c = np.ascontiguousarray(cells)
        if c.dtype not in (np.float32, np.float64):
            raise TypeError("cells must be float32 or float64")
        dtype = WC_F64 if c.dtype == np.float64 else WC_F32
        cap = payload_bound(units, n)
        payload = np.empty(cap, np.uint8)
        offsets = np.zeros(n + 1, np.uint64)
        kept = np.zeros(max(n, 1), np.uint32)
        rmse = np.zeros(max(n, 1), np.float64)
        self._check(self._L.wc_round_trip_host(self._h, c.ctypes.data, dtype, units, n, float(keep),
                                               payload.ctypes.data, cap, offsets.ctypes.data, kept.ctypes.data,
                                               rmse.ctypes.data))
        return payload, offsets, kept[:n], rmse[:n]

    def forward_tol_host(self, cells: np.ndarray, units, n: int, tol):
        """wc_forward_tol_host: per-unit RMSE tolerances in place of keep ->
        (payload, offsets, kept, thresh, bound, rmse); rmse is the actual RMSE of
        each unit's round trip, taken on the device."""
        c = np.ascontiguousarray(cells)
        if c.dtype not in (np.float32, np.float64):
            raise TypeError("cells must be float32 or float64")
        dtype = WC_F64 if c.dtype == np.float64 else WC_F32
        t = _tol_array(tol, n)
        cap = payload_bound(units, n)
        payload = np.empty(cap, np.uint8)
        offsets = np.zeros(n + 1, np.uint64)
        kept = np.zeros(max(n, 1), np.uint32)
        thresh = np.zeros(max(n, 1), np.float32)
        bound = np.zeros(max(n, 1), np.float64)
        rmse = np.zeros(max(n, 1), np.float64)
        self._check(self._L.wc_forward_tol_host(self._h, c.ctypes.data, dtype, units, n, t.ctypes.data,
                                                payload.ctypes.data, cap, offsets.ctypes.data, kept.ctypes.data,
                                                thresh.ctypes.data, bound.ctypes.data, rmse.ctypes.data))
        return payload, offsets, kept[:n], thresh[:n], bound[:n], rmse[:n]

    def forward_levels_tol_host(self, cells: np.ndarray, units, n: int, levels, tol, want_rmse: bool = True):
        """wc_forward_levels_tol_host -> (payload, offsets, kept, thresh [n,
        WC_MAX_LEVELS], bound, rmse); rmse is the actual RMSE of each unit's round
        trip, taken on the device (None, and no round trip, without want_rmse)."""
        c = np.ascontiguousarray(cells)
        if c.dtype not in (np.float32, np.float64):
            raise TypeError("cells must be float32 or float64")
        dtype = WC_F64 if c.dtype == np.float64 else WC_F32
        lv = _levels_array(levels, n)
        t = _tol_array(tol, n)
        cap = payload_bound(units, n)
        payload = np.empty(cap, np.uint8)
        offsets = np.zeros(n + 1, np.uint64)
        kept = np.zeros(max(n, 1), np.uint32)
        thresh = np.zeros((max(n, 1), WC_MAX_LEVELS), np.float32)
        bound = np.zeros(max(n, 1), np.float64)
        rmse = np.zeros(max(n, 1), np.float64) if want_rmse else None
        self._check(self._L.wc_forward_levels_tol_host(self._h, c.ctypes.data, dtype, units, n, lv.ctypes.data,
                                                       t.ctypes.data, payload.ctypes.data, cap, offsets.ctypes.data,
                                                       kept.ctypes.data, thresh.ctypes.data, bound.ctypes.data,
                                                       rmse.ctypes.data if want_rmse else None))
        return payload, offsets, kept[:n], thresh[:n], bound[:n], rmse[:n] if want_rmse else None

    def forward_levels_maxerr_host(self, cells: np.ndarray, units, n: int, levels, maxerr, want_rmse: bool = True):
        """wc_forward_levels_maxerr_host -> (payload, offsets, kept, thresh [n], err
        [n], rmse); err is the achieved max error of each unit, rmse the RMSE of its
        round trip, taken on the device (None, and no round trip, without
        want_rmse)."""
        c = np.ascontiguousarray(cells)
        if c.dtype not in (np.float32, np.float64):
            raise TypeError("cells must be float32 or float64")
        dtype = WC_F64 if c.dtype == np.float64 else WC_F32
        lv = None if levels is None else _levels_array(levels, n)
        t = _tol_array(maxerr, n)
        cap = payload_bound(units, n)
        payload = np.empty(cap, np.uint8)
        offsets = np.zeros(n + 1, np.uint64)
        kept = np.zeros(max(n, 1), np.uint32)
        thresh = np.zeros(max(n, 1), np.float32)
        err = np.zeros(max(n, 1), np.float64)
        rmse = np.zeros(max(n, 1), np.float64) if want_rmse else None
        self._check(self._L.wc_forward_levels_maxerr_host(self._h, c.ctypes.data, dtype, units, n,
                                                          None if lv is None else lv.ctypes.data, t.ctypes.data,
                                                          payload.ctypes.data, cap, offsets.ctypes.data,
                                                          kept.ctypes.data, thresh.ctypes.data, err.ctypes.data,
                                                          rmse.ctypes.data if want_rmse else None))
        return payload, offsets, kept[:n], thresh[:n], err[:n], rmse[:n] if want_rmse else None

    def forward_levels_budget_host(self, cells: np.ndarray, units, n: int, levels, max_pairs, want_rmse: bool = True):
        """wc_forward_levels_budget_host -> (payload, offsets, kept, thresh [n,
        WC_MAX_LEVELS], key, rmse); rmse is the actual RMSE of each unit's round
        trip, taken on the device (None, and no round trip, without want_rmse)."""
        c = np.ascontiguousarray(cells)
        if c.dtype not in (np.float32, np.float64):
            raise TypeError("cells must be float32 or float64")
        dtype = WC_F64 if c.dtype == np.float64 else WC_F32
        lv = None if levels is None else _levels_array(levels, n)
        k = _pairs_array(max_pairs, n)
        cap = payload_bound(units, n)
        payload = np.empty(cap, np.uint8)
        offsets = np.zeros(n + 1, np.uint64)
        kept = np.zeros(max(n, 1), np.uint32)
        thresh = np.zeros((max(n, 1), WC_MAX_LEVELS), np.float32)
        key = np.zeros(max(n, 1), np.uint32)
        rmse = np.zeros(max(n, 1), np.float64) if want_rmse else None
        self._check(self._L.wc_forward_levels_budget_host(self._h, c.ctypes.data, dtype, units, n,
                                                          None if lv is None else lv.ctypes.data, k.ctypes.data,
                                                          payload.ctypes.data, cap, offsets.ctypes.data,
                                                          kept.ctypes.data, thresh.ctypes.data, key.ctypes.data,
                                                          rmse.ctypes.data if want_rmse else None))
        return payload, offsets, kept[:n], thresh[:n], key[:n], rmse[:n] if want_rmse else None

    def thin_host(self, payload: np.ndarray, offsets: np.ndarray, units, n: int, levels=None, max_pairs=None,
                  thresh=None):
        """wc_thin_budget_host (max_pairs) or wc_thin_thresh_host (thresh: n x
        WC_MAX_LEVELS) -> (out, out_offsets, kept, thresh [n, WC_MAX_LEVELS] or None, key or
        None), packed as forward_host.  levels None: from the headers."""
        if (max_pairs is None) == (thresh is None):
            raise ValueError("exactly one of max_pairs and thresh")
        p = np.ascontiguousarray(payload, np.uint8)
        off = np.ascontiguousarray(offsets, np.uint64)
        lv = None if levels is None else _levels_array(levels, n)
        k = None if max_pairs is None else _pairs_array(max_pairs, n)
        cap = thin_bound(units, n, k)
        out = np.empty(cap, np.uint8)
        out_offsets = np.zeros(n + 1, np.uint64)
        kept = np.zeros(max(n, 1), np.uint32)
        if k is not None:
            th = np.zeros((max(n, 1), WC_MAX_LEVELS), np.float32)
            key = np.zeros(max(n, 1), np.uint32)
            self._check(self._L.wc_thin_budget_host(self._h, p.ctypes.data, off.ctypes.data, units, n,
                                                    None if lv is None else lv.ctypes.data, k.ctypes.data,
                                                    out.ctypes.data, cap, out_offsets.ctypes.data, kept.ctypes.data,
                                                    th.ctypes.data, key.ctypes.data))
            return out, out_offsets, kept[:n], th[:n], key[:n]
        t = _thin_thresh_array(thresh, n)
        self._check(self._L.wc_thin_thresh_host(self._h, p.ctypes.data, off.ctypes.data, units, n,
                                                None if lv is None else lv.ctypes.data, t.ctypes.data,
                                                out.ctypes.data, cap, out_offsets.ctypes.data, kept.ctypes.data))
        return out, out_offsets, kept[:n], None, None

    def split_host(self, payload: np.ndarray, offsets: np.ndarray, units, n: int, levels=None, max_pairs=None,
                   thresh=None):
        """wc_split_budget_host (max_pairs) or wc_split_thresh_host (thresh: n x
        WC_MAX_LEVELS) -> (base, base_offsets, kept, rest, rest_offsets, rest_pairs, thresh
        [n, WC_MAX_LEVELS] or None, key or None), both packed as forward_host."""
        if (max_pairs is None) == (thresh is None):
            raise ValueError("exactly one of max_pairs and thresh")
        p = np.ascontiguousarray(payload, np.uint8)
        off = np.ascontiguousarray(offsets, np.uint64)
        lv = None if levels is None else _levels_array(levels, n)
        k = None if max_pairs is None else _pairs_array(max_pairs, n)
        bcap, rcap = split_bound(units, n, k)
        base, rest = np.empty(bcap, np.uint8), np.empty(rcap, np.uint8)
        boff, roff = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        kept, rpairs = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        lvp = None if lv is None else lv.ctypes.data
        if k is not None:
            th = np.zeros((max(n, 1), WC_MAX_LEVELS), np.float32)
            key = np.zeros(max(n, 1), np.uint32)
            self._check(self._L.wc_split_budget_host(self._h, p.ctypes.data, off.ctypes.data, units, n, lvp,
                                                     k.ctypes.data, base.ctypes.data, bcap, boff.ctypes.data,
                                                     kept.ctypes.data, rest.ctypes.data, rcap, roff.ctypes.data,
                                                     rpairs.ctypes.data, th.ctypes.data, key.ctypes.data))
            return base, boff, kept[:n], rest, roff, rpairs[:n], th[:n], key[:n]
        t = _thin_thresh_array(thresh, n)
        self._check(self._L.wc_split_thresh_host(self._h, p.ctypes.data, off.ctypes.data, units, n, lvp, t.ctypes.data,
                                                 base.ctypes.data, bcap, boff.ctypes.data, kept.ctypes.data,
                                                 rest.ctypes.data, rcap, roff.ctypes.data, rpairs.ctypes.data))
        return base, boff, kept[:n], rest, roff, rpairs[:n], None, None

    def thin_tol_host(self, payload: np.ndarray, offsets: np.ndarray, units, n: int, tol, levels=None):
        """wc_thin_tol_host -> (out, out_offsets, kept, thresh [n, WC_MAX_LEVELS], bound),
        packed as forward_host.  levels None: from the headers."""
        p = np.ascontiguousarray(payload, np.uint8)
        off = np.ascontiguousarray(offsets, np.uint64)
        lv = None if levels is None else _levels_array(levels, n)
        t = _tol_array(tol, n)
        cap = thin_bound(units, n, None)
        out = np.empty(cap, np.uint8)
        out_offsets = np.zeros(n + 1, np.uint64)
        kept = np.zeros(max(n, 1), np.uint32)
        th = np.zeros((max(n, 1), WC_MAX_LEVELS), np.float32)
        bound = np.zeros(max(n, 1), np.float64)
        self._check(self._L.wc_thin_tol_host(self._h, p.ctypes.data, off.ctypes.data, units, n,
                                             None if lv is None else lv.ctypes.data, t.ctypes.data, out.ctypes.data,
                                             cap, out_offsets.ctypes.data, kept.ctypes.data, th.ctypes.data,
                                             bound.ctypes.data))
        return out, out_offsets, kept[:n], th[:n], bound[:n]

    def split_tol_host(self, payload: np.ndarray, offsets: np.ndarray, units, n: int, tol, levels=None):
        """wc_split_tol_host -> (base, base_offsets, kept, rest, rest_offsets, rest_pairs,
        thresh [n, WC_MAX_LEVELS], bound), both packed as forward_host."""
        p = np.ascontiguousarray(payload, np.uint8)
        off = np.ascontiguousarray(offsets, np.uint64)
        lv = None if levels is None else _levels_array(levels, n)
        t = _tol_array(tol, n)
        bcap, rcap = split_bound(units, n, None)
        base, rest = np.empty(bcap, np.uint8), np.empty(rcap, np.uint8)
        boff, roff = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        kept, rpairs = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        th = np.zeros((max(n, 1), WC_MAX_LEVELS), np.float32)
        bound = np.zeros(max(n, 1), np.float64)
        self._check(self._L.wc_split_tol_host(self._h, p.ctypes.data, off.ctypes.data, units, n,
                                              None if lv is None else lv.ctypes.data, t.ctypes.data,
                                              base.ctypes.data, bcap, boff.ctypes.data, kept.ctypes.data,
                                              rest.ctypes.data, rcap, roff.ctypes.data, rpairs.ctypes.data,
                                              th.ctypes.data, bound.ctypes.data))
        return base, boff, kept[:n], rest, roff, rpairs[:n], th[:n], bound[:n]

    def merge_host(self, a: np.ndarray, a_offsets: np.ndarray, b: np.ndarray, b_offsets: np.ndarray, units, n: int,
                   levels=None):
        """wc_merge_host -> (out, out_offsets, pairs), packed as forward_host.  levels None:
        from the headers."""
        pa, pb = np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(b, np.uint8)
        oa, ob = np.ascontiguousarray(a_offsets, np.uint64), np.ascontiguousarray(b_offsets, np.uint64)
        lv = None if levels is None else _levels_array(levels, n)
        cap = merge_bound(units, n)
        out = np.empty(cap, np.uint8)
        out_offsets = np.zeros(n + 1, np.uint64)
        pairs = np.zeros(max(n, 1), np.uint32)
        self._check(self._L.wc_merge_host(self._h, pa.ctypes.data, oa.ctypes.data, pb.ctypes.data, ob.ctypes.data,
                                          units, n, None if lv is None else lv.ctypes.data, out.ctypes.data, cap,
                                          out_offsets.ctypes.data, pairs.ctypes.data))
        return out, out_offsets, pairs[:n]

    def forward_levels_host(self, cells: np.ndarray, units, n: int, levels, keep: float,
                            thresh: float | None = None):
        """wc_forward_levels_host -> (payload, offsets, kept), packed as forward_host."""
        c = np.ascontiguousarray(cells)
        if c.dtype not in (np.float32, np.float64):
            raise TypeError("cells must be float32 or float64")
        dtype = WC_F64 if c.dtype == np.float64 else WC_F32
        lv = _levels_array(levels, n)
        t = None if thresh is None else ctypes.byref(ctypes.c_float(thresh))
        cap = payload_bound(units, n)
        payload = np.empty(cap, np.uint8)
        offsets = np.zeros(n + 1, np.uint64)
        kept = np.zeros(max(n, 1), np.uint32)
        self._check(self._L.wc_forward_levels_host(self._h, c.ctypes.data, dtype, units, n, lv.ctypes.data,
                                                   float(keep), t, payload.ctypes.data, cap, offsets.ctypes.data,
                                                   kept.ctypes.data))
        return payload, offsets, kept[:n]

    def inverse_levels_host(self, payload: np.ndarray, offsets: np.ndarray, units, n: int, extent: int,
                            levels=None, out=None):
        """wc_inverse_levels_host -> float32[extent] boxes; levels None: each
        unit's L is read from its payload header."""
        p = np.ascontiguousarray(payload, dtype=np.uint8)
        o = np.ascontiguousarray(offsets, dtype=np.uint64)
        lv = None if levels is None else _levels_array(levels, n)
        if out is None:
            out = np.zeros(max(extent, 1), np.float32)
        elif out.dtype != np.float32 or out.size < extent or not out.flags.c_contiguous:
            raise ValueError("out: contiguous float32[>= extent]")
        self._check(self._L.wc_inverse_levels_host(self._h, p.ctypes.data, o.ctypes.data, units, n,
                                                   None if lv is None else lv.ctypes.data, out.ctypes.data))
        return out[:extent]

    def inverse_coarse_host(self, payload: np.ndarray, offsets: np.ndarray, units, n: int, reduce, out_units,
                            extent: int, levels=None, out=None):
        """wc_inverse_coarse_host -> float32[extent] coarse boxes at out_units'
        offsets; levels None: each unit's L is read from its payload header."""
        p = np.ascontiguousarray(payload, dtype=np.uint8)
        o = np.ascontiguousarray(offsets, dtype=np.uint64)
        lv = None if levels is None else _levels_array(levels, n)
        rd = _levels_array(reduce, n)
        if out is None:
            out = np.zeros(max(extent, 1), np.float32)
        elif out.dtype != np.float32 or out.size < extent or not out.flags.c_contiguous:
            raise ValueError("out: contiguous float32[>= extent]")
        self._check(self._L.wc_inverse_coarse_host(self._h, p.ctypes.data, o.ctypes.data, units, n,
                                                   None if lv is None else lv.ctypes.data, rd.ctypes.data, out_units,
                                                   out.ctypes.data))
        return out[:extent]

    def inverse_region_host(self, payload: np.ndarray, offsets: np.ndarray, units, n: int, reduce, regions, out_units,
                            extent: int, levels=None, out=None):
        """wc_inverse_region_host -> float32[extent] region boxes at out_units'
        offsets; levels None: each unit's L is read from its payload header;
        reduce None: all 0."""
        p = np.ascontiguousarray(payload, dtype=np.uint8)
        o = np.ascontiguousarray(offsets, dtype=np.uint64)
        lv = None if levels is None else _levels_array(levels, n)
        rd = None if reduce is None else _levels_array(reduce, n)
        if out is None:
            out = np.zeros(max(extent, 1), np.float32)
        elif out.dtype != np.float32 or out.size < extent or not out.flags.c_contiguous:
            raise ValueError("out: contiguous float32[>= extent]")
        self._check(self._L.wc_inverse_region_host(self._h, p.ctypes.data, o.ctypes.data, units, n,
                                                   None if lv is None else lv.ctypes.data,
                                                   None if rd is None else rd.ctypes.data, make_regions(regions, n),
                                                   out_units, out.ctypes.data))
        return out[:extent]

    def pack_host(self, payload: np.ndarray, offsets: np.ndarray, units, n: int, vbytes: int):
        """wc_pack_host: standard payloads (host) -> (packed uint8, packed_offsets
        uint64[n + 1], packed_bytes uint64[n]); unit u's packed bytes are
        packed[packed_offsets[u] : packed_offsets[u] + packed_bytes[u]]."""
        p = np.ascontiguousarray(payload, dtype=np.uint8)
        o = np.ascontiguousarray(offsets, dtype=np.uint64)
        cap = packed_bound(units, n, vbytes)
        packed = np.empty(cap, np.uint8)
        poff = np.zeros(n + 1, np.uint64)
        pbytes = np.zeros(max(n, 1), np.uint64)
        self._check(self._L.wc_pack_host(self._h, p.ctypes.data, o.ctypes.data, units, n, int(vbytes),
                                         packed.ctypes.data, cap, poff.ctypes.data, pbytes.ctypes.data))
        return packed[:int(poff[n])] if n else packed[:0], poff, pbytes[:n]

    def unpack_host(self, packed: np.ndarray, packed_offsets: np.ndarray, units, n: int):
        """wc_unpack_host: packed units (host, each offset == 4 mod 8) -> (payload,
        offsets, kept) as forward_host returns them."""
        p = np.ascontiguousarray(packed, dtype=np.uint8)
        o = np.ascontiguousarray(packed_offsets, dtype=np.uint64)
        cap = payload_bound(units, n)
        payload = np.empty(cap, np.uint8)
        offsets = np.zeros(n + 1, np.uint64)
        kept = np.zeros(max(n, 1), np.uint32)
        self._check(self._L.wc_unpack_host(self._h, p.ctypes.data, o.ctypes.data, units, n, payload.ctypes.data, cap,
                                           offsets.ctypes.data, kept.ctypes.data))
        return payload, offsets, kept[:n]

    def _packed_host_args(self, packed, packed_offsets, n, extent, levels, out):
        p = np.ascontiguousarray(packed, dtype=np.uint8)
        o = np.ascontiguousarray(packed_offsets, dtype=np.uint64)
        lv = None if levels is None else _levels_array(levels, n)
        if out is None:
            out = np.zeros(max(extent, 1), np.float32)
        elif out.dtype != np.float32 or out.size < extent or not out.flags.c_contiguous:
            raise ValueError("out: contiguous float32[>= extent]")
        return p, o, lv, out

    def inverse_packed_host(self, packed: np.ndarray, packed_offsets: np.ndarray, units, n: int, extent: int,
                            levels=None, out=None):
        """wc_inverse_packed_host: packed units (host, each offset == 4 mod 8) ->
        float32[extent] boxes; levels None: each unit's L is read from its tag."""
        p, o, lv, out = self._packed_host_args(packed, packed_offsets, n, extent, levels, out)
        self._check(self._L.wc_inverse_packed_host(self._h, p.ctypes.data, o.ctypes.data, units, n,
                                                   None if lv is None else lv.ctypes.data, out.ctypes.data))
        return out[:extent]

    def inverse_packed_coarse_host(self, packed: np.ndarray, packed_offsets: np.ndarray, units, n: int, reduce,
                                   out_units, extent: int, levels=None, out=None):
        """wc_inverse_packed_coarse_host -> float32[extent] coarse boxes at out_units' offsets."""
        p, o, lv, out = self._packed_host_args(packed, packed_offsets, n, extent, levels, out)
        rd = _levels_array(reduce, n)
        self._check(self._L.wc_inverse_packed_coarse_host(self._h, p.ctypes.data, o.ctypes.data, units, n,
                                                          None if lv is None else lv.ctypes.data, rd.ctypes.data,
                                                          out_units, out.ctypes.data))
        return out[:extent]

    def inverse_packed_region_host(self, packed: np.ndarray, packed_offsets: np.ndarray, units, n: int, reduce,
                                   regions, out_units, extent: int, levels=None, out=None):
        """wc_inverse_packed_region_host -> float32[extent] region boxes at out_units' offsets; reduce None: all 0."""
        p, o, lv, out = self._packed_host_args(packed, packed_offsets, n, extent, levels, out)
        rd = None if reduce is None else _levels_array(reduce, n)
        self._check(self._L.wc_inverse_packed_region_host(self._h, p.ctypes.data, o.ctypes.data, units, n,
                                                          None if lv is None else lv.ctypes.data,
                                                          None if rd is None else rd.ctypes.data,
                                                          make_regions(regions, n), out_units, out.ctypes.data))
        return out[:extent]

    def forward_host_units(self, boxes, units, n: int, keep: float):
        """wc_forward_host_units: unit u's cells from boxes[u] (its own host
        array, all float32 or all float64) -> (payload, offsets, kept)."""
        arrs = [np.ascontiguousarray(b) for b in boxes]
        dt = {a.dtype for a in arrs if a.size}
        if not dt <= {np.dtype(np.float32)} and not dt <= {np.dtype(np.float64)}:
            raise TypeError("boxes must be all float32 or all float64")
        dtype = WC_F64 if dt == {np.dtype(np.float64)} else WC_F32
        ptrs = (ctypes.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
        cap = payload_bound(units, n)
        payload = np.empty(cap, np.uint8)
        offsets = np.zeros(n + 1, np.uint64)
        kept = np.zeros(max(n, 1), np.uint32)
        self._check(self._L.wc_forward_host_units(self._h, ptrs, dtype, units, n, float(keep), payload.ctypes.data,
                                                  cap, offsets.ctypes.data, kept.ctypes.data))
        return payload, offsets, kept[:n]

    def decompose_host(self, cells: np.ndarray, units, n: int, extent: int) -> np.ndarray:
        c = np.ascontiguousarray(cells)
        dtype = WC_F64 if c.dtype == np.float64 else WC_F32
        out = np.zeros(max(extent, 1), np.float32)
        self._check(self._L.wc_decompose_host(self._h, c.ctypes.data, dtype, units, n, out.ctypes.data))
        return out[:extent]

    def inverse_flat_host(self, flat: np.ndarray, units, n: int, extent: int) -> np.ndarray:
        f = np.ascontiguousarray(flat, np.float32)
        out = np.zeros(max(extent, 1), np.float32)
        self._check(self._L.wc_inverse_flat_host(self._h, f.ctypes.data, units, n, out.ctypes.data))
        return out[:extent]

    def rmse_host(self, orig: np.ndarray, regen: np.ndarray, units, n: int) -> np.ndarray:
        o = np.ascontiguousarray(orig)
        dtype = WC_F64 if o.dtype == np.float64 else WC_F32
        r = np.ascontiguousarray(regen, np.float32)
        out = np.zeros(max(n, 1), np.float64)
        self._check(self._L.wc_rmse_host(self._h, o.ctypes.data, dtype, r.ctypes.data, units, n, out.ctypes.data))
        return out[:n]

    def maxerr_host(self, orig: np.ndarray, regen: np.ndarray, units, n: int) -> np.ndarray:
        """wc_maxerr_host: per unit the max of |orig - regen| over the non-NaN differences."""
        o = np.ascontiguousarray(orig)
        dtype = WC_F64 if o.dtype == np.float64 else WC_F32
        r = np.ascontiguousarray(regen, np.float32)
        out = np.zeros(max(n, 1), np.float64)
        self._check(self._L.wc_maxerr_host(self._h, o.ctypes.data, dtype, r.ctypes.data, units, n, out.ctypes.data))
        return out[:n]

    def inverse_host(self, payload: np.ndarray, offsets: np.ndarray, units, n: int, extent: int, out=None):
        """-> float32[extent] boxes (cells no unit owns stay 0, or as they were in `out`)."""
        p = np.ascontiguousarray(payload, dtype=np.uint8)
        o = np.ascontiguousarray(offsets, dtype=np.uint64)
        if out is None:
            out = np.zeros(max(extent, 1), np.float32)
        elif out.dtype != np.float32 or out.size < extent or not out.flags.c_contiguous:
            raise ValueError("out: contiguous float32[>= extent]")
        self._check(self._L.wc_inverse_host(self._h, p.ctypes.data, o.ctypes.data, units, n,
                                            out.ctypes.data))
        return out[:extent]


HIST_BINS = 4096  # WC_HIST_BINS
HIST_SHIFT = 19   # WC_HIST_SHIFT


def hist_threshold(hist: np.ndarray, quantile: float):
    """wc_hist_threshold (host only): (fp32 threshold, retained count) for an
    all-reduced WC_HIST_BINS uint64 histogram."""
    h = np.ascontiguousarray(hist, dtype=np.uint64)
    if h.size != HIST_BINS:
        raise ValueError(f"histogram must have {HIST_BINS} bins")
    t = ctypes.c_float()
    r = ctypes.c_uint64()
    rc = load_library().wc_hist_threshold(h.ctypes.data, float(quantile), ctypes.byref(t), ctypes.byref(r))
    if rc:
        raise WaveletError(rc, "wc_hist_threshold: invalid argument")
    return float(t.value), int(r.value)


def _tol_array(tol, n: int) -> np.ndarray:
    """Per-unit tolerances as n contiguous doubles (one value: the same for every unit)."""
    t = np.ascontiguousarray(np.broadcast_to(np.asarray(tol, np.float64), (n,)) if np.ndim(tol) == 0 else tol,
                             dtype=np.float64)
    if t.shape != (n,):
        raise ValueError(f"tol: one value or {n} values")
    return t


def _pairs_array(max_pairs, n: int) -> np.ndarray:
    """Per-unit pair budgets as n contiguous uint32 (one value: the same for every unit)."""
    k = np.asarray(max_pairs)
    if k.size and (k.min() < 0 or k.max() > 0xFFFFFFFF):
        raise ValueError("max_pairs: values in 0..2^32 - 1")
    k = np.ascontiguousarray(np.broadcast_to(k, (n,)) if k.ndim == 0 else k, dtype=np.uint32)
    if k.shape != (n,):
        raise ValueError(f"max_pairs: one value or {n} values")
    return k


def _levels_array(levels, n: int) -> np.ndarray:
    """Per-unit levels as n contiguous int32 (one value: the same for every unit)."""
    lv = np.ascontiguousarray(np.broadcast_to(np.asarray(levels, np.int32), (n,)) if np.ndim(levels) == 0 else levels,
                              dtype=np.int32)
    if lv.shape != (n,):
        raise ValueError(f"levels: one value or {n} values")
    return lv


def levels_for(nx: int, ny: int, nz: int, want: int) -> int:
    """wc_levels_for (host only): the largest L <= min(want, WC_MAX_LEVELS) with
    2^L dividing nx, ny and nz; 1 if none does or the box has no cells."""
    return int(load_library().wc_levels_for(int(nx), int(ny), int(nz), int(want)))


def coarse_units(units, n: int, reduce):
    """wc_coarse_units (host only): (out_units, extent) of a reduction: unit u's
    dims >> reduce[u], packed back to back with each start rounded up to 4."""
    rd = _levels_array(reduce, n)
    out = (WcUnit * max(n, 1))()
    ext = ctypes.c_uint64()
    rc = load_library().wc_coarse_units(units, rd.ctypes.data, n, out, ctypes.byref(ext))
    if rc:
        raise WaveletError(rc, "wc_coarse_units: negative dims or a reduce outside 0..WC_MAX_LEVELS")
    return out, int(ext.value)


def make_regions(regions, n: int):
    """A wc_region array from n (x0, y0, z0, nx, ny, nz) rows (a WcRegion array passes through)."""
    if isinstance(regions, ctypes.Array) and regions._type_ is WcRegion:
        return regions
    rows = [tuple(int(v) for v in g) for g in regions]
    if len(rows) != n or any(len(g) != 6 for g in rows):
        raise ValueError(f"regions: {n} rows of (x0, y0, z0, nx, ny, nz)")
    return (WcRegion * max(n, 1))(*[WcRegion(*g) for g in rows])


def region_align(dims, levels: int, region):
    """wc_region_align (host only): the smallest region aligned to 2^levels that
    contains region = (x0, y0, z0, nx, ny, nz) inside the box dims = (W, H, D),
    as the same kind of tuple."""
    want, got = WcRegion(*[int(v) for v in region]), WcRegion()
    rc = load_library().wc_region_align(int(dims[0]), int(dims[1]), int(dims[2]), int(levels), ctypes.byref(want),
                                        ctypes.byref(got))
    if rc:
        raise WaveletError(rc, "wc_region_align: a region outside the box, levels outside 1..WC_MAX_LEVELS or "
                               "dimensions that 2^levels does not divide")
    return (got.x0, got.y0, got.z0, got.nx, got.ny, got.nz)


def region_units(units, n: int, regions, reduce=None):
    """wc_region_units (host only): (out_units, extent) of the regions' boxes:
    unit u's extents >> reduce[u], packed back to back with each start rounded up to 4."""
    rd = None if reduce is None else _levels_array(reduce, n)
    out = (WcUnit * max(n, 1))()
    ext = ctypes.c_uint64()
    rc = load_library().wc_region_units(units, make_regions(regions, n), None if rd is None else rd.ctypes.data, n, out,
                                        ctypes.byref(ext))
    if rc:
        raise WaveletError(rc, "wc_region_units: negative extents or a reduce outside 0..WC_MAX_LEVELS")
    return out, int(ext.value)


def payload_levels(header) -> int:
    """wc_payload_levels (host only): L of a payload from its first 20 bytes."""
    h = np.frombuffer(bytes(header), dtype=np.uint8)
    lv = ctypes.c_int()
    rc = load_library().wc_payload_levels(h.ctypes.data, h.size, ctypes.byref(lv))
    if rc:
        raise WaveletError(rc, "wc_payload_levels: not a payload header")
    return int(lv.value)


def pack_value(bits: int, vbytes: int) -> int:
    """wc_pack_value (host only): q, the fp32 bits rounded to nearest even at vbytes bytes."""
    return int(load_library().wc_pack_value(int(bits) & 0xFFFFFFFF, int(vbytes)))


def packed_tag(levels: int, vbytes: int) -> int:
    """wc_packed_tag (host only): -(16 * vbytes + levels); 0 for values out of range."""
    return int(load_library().wc_packed_tag(int(levels), int(vbytes)))


def payload_packed(header):
    """wc_payload_packed (host only): (levels, vbytes) of a unit from its first 20
    bytes; vbytes = 0 for a standard or multi-level payload."""
    h = np.frombuffer(bytes(header[:20]), dtype=np.uint8)
    lv, vb = ctypes.c_int(), ctypes.c_int()
    rc = load_library().wc_payload_packed(h.ctypes.data, h.size, ctypes.byref(lv), ctypes.byref(vb))
    if rc:
        raise WaveletError(rc, "wc_payload_packed: neither a payload header nor a packed one")
    return int(lv.value), int(vb.value)


def packed_size(unit) -> int:
    """wc_packed_size (host only): the length of the packed unit at the start of
    `unit`, from its header and width table."""
    b = np.frombuffer(bytes(unit), dtype=np.uint8)
    out = ctypes.c_uint64()
    rc = load_library().wc_packed_size(b.ctypes.data, b.size, ctypes.byref(out))
    if rc:
        raise WaveletError(rc, "wc_packed_size: a short buffer or a malformed packed unit")
    return int(out.value)


def packed_bound(units, n: int, vbytes: int) -> int:
    """wc_packed_bound (host only): the capacity wc_pack needs (the slots' end)."""
    out = ctypes.c_uint64()
    rc = load_library().wc_packed_bound(units, n, int(vbytes), ctypes.byref(out))
    if rc:
        raise WaveletError(rc, "wc_packed_bound: negative dims or vbytes outside 2..4")
    return int(out.value)


def pack_unit(payload, vbytes: int) -> bytes:
    """wc_pack_unit (host only): one standard payload -> its packed unit."""
    p = np.frombuffer(bytes(payload), dtype=np.uint8)
    n = (p.size - 20) // 8 if p.size >= 20 else 0
    out = np.empty(20 + (n // 64 + 8) + 31 * (n // 8 + 1) + 4 * n + 16, np.uint8)
    w = ctypes.c_size_t()
    rc = load_library().wc_pack_unit(p.ctypes.data, p.size, int(vbytes), out.ctypes.data, out.size, ctypes.byref(w))
    if rc:
        raise WaveletError(rc, "wc_pack_unit: a malformed payload, a short buffer or vbytes outside 2..4")
    return out[:w.value].tobytes()


def unpack_unit(packed) -> bytes:
    """wc_unpack_unit (host only): one packed unit -> its standard payload (values q(v))."""
    p = np.frombuffer(bytes(packed), dtype=np.uint8)
    nrle = int(np.frombuffer(p[16:20].tobytes(), np.int32)[0]) if p.size >= 20 else 0
    out = np.empty(20 + 8 * min(max(nrle, 0), p.size), np.uint8)  # a pair takes at least two packed bytes
    w = ctypes.c_size_t()
    rc = load_library().wc_unpack_unit(p.ctypes.data, p.size, out.ctypes.data, out.size, ctypes.byref(w))
    if rc:
        raise WaveletError(rc, "wc_unpack_unit: a malformed or short packed unit")
    return out[:w.value].tobytes()


def tol_threshold(counts: np.ndarray, ncoeff: int, tol: float):
    """wc_tol_threshold (host only): (fp32 threshold, model RMSE bound) of the
    RMSE-tolerance rule on one unit's WC_HIST_BINS uint64 bin counts."""
    h = np.ascontiguousarray(counts, dtype=np.uint64)
    if h.size != HIST_BINS:
        raise ValueError(f"histogram must have {HIST_BINS} bins")
    t = ctypes.c_float()
    b = ctypes.c_double()
    rc = load_library().wc_tol_threshold(h.ctypes.data, int(ncoeff), float(tol), ctypes.byref(t), ctypes.byref(b))
    if rc:
        raise WaveletError(rc, "wc_tol_threshold: invalid argument")
    return float(t.value), float(b.value)


def tol_levels_threshold(counts: np.ndarray, levels: int, ncoeff: int, tol: float):
    """wc_tol_levels_threshold (host only): (fp32 thresholds of levels 1..L, model
    RMSE bound) of the multi-level RMSE-tolerance rule on one unit's counts,
    levels x WC_HIST_BINS uint64, level-major."""
    h = np.ascontiguousarray(counts, dtype=np.uint64)
    L = int(levels)
    if 1 <= L <= WC_MAX_LEVELS and h.size != L * HIST_BINS:  # other L: the library refuses them
        raise ValueError(f"counts must have levels x {HIST_BINS} bins")
    t = (ctypes.c_float * WC_MAX_LEVELS)()
    b = ctypes.c_double()
    rc = load_library().wc_tol_levels_threshold(h.ctypes.data, L, int(ncoeff), float(tol), t, ctypes.byref(b))
    if rc:
        raise WaveletError(rc, "wc_tol_levels_threshold: invalid argument")
    return [float(t[l]) for l in range(L)], float(b.value)


def _thin_thresh_array(thresh, n):
    """Per-unit, per-level thresholds as n x WC_MAX_LEVELS contiguous float32 (one value: the same everywhere)."""
    t = np.asarray(thresh, np.float32)
    if t.ndim == 0:
        t = np.full((max(n, 1), WC_MAX_LEVELS), t, np.float32)
    if t.shape != (max(n, 1), WC_MAX_LEVELS) and t.shape != (n, WC_MAX_LEVELS):
        raise ValueError("thresh must be n x WC_MAX_LEVELS floats")
    return np.ascontiguousarray(t, np.float32)


def thin_bound(units, n: int, max_pairs=None) -> int:
    """wc_thin_bound: the output extent of thin_budget (max_pairs) / thin_thresh (None)."""
    k = None if max_pairs is None else _pairs_array(max_pairs, n)
    return int(load_library().wc_thin_bound(units, n, None if k is None else k.ctypes.data))


def thin_unit(payload, max_pairs=None, thresh=None):
    """wc_thin_unit (host only): the rule on one standard payload -> (bytes, T, fp32
    thresholds of levels 1..L).  Exactly one of max_pairs (K) and thresh (L floats)."""
    p = np.frombuffer(bytes(payload), np.uint8)
    out = np.empty(max(p.size, 20), np.uint8)
    written = ctypes.c_size_t(0)
    key = ctypes.c_uint32(0)
    tout = np.zeros(WC_MAX_LEVELS, np.float32)
    k = None if max_pairs is None else ctypes.c_uint32(int(max_pairs))
    t = None if thresh is None else np.ascontiguousarray(np.resize(np.asarray(thresh, np.float32), WC_MAX_LEVELS))
    rc = load_library().wc_thin_unit(p.ctypes.data, p.size, None if k is None else ctypes.addressof(k),
                                     None if t is None else t.ctypes.data, out.ctypes.data, out.size,
                                     ctypes.byref(written), ctypes.byref(key), tout.ctypes.data)
    if rc != 0:
        raise WaveletError(rc, "wc_thin_unit: refused")
    return out[:written.value].tobytes(), int(key.value), tout[:payload_levels(bytes(payload[:20]))].copy()


def thin_tol_unit(payload, tol: float, cap=None):
    """wc_thin_tol_unit (host only): the tolerance rule on one standard payload ->
    (bytes, fp32 thresholds of levels 1..L, bound)."""
    p = np.frombuffer(bytes(payload), np.uint8)
    out = np.empty(max(p.size, 20) if cap is None else max(int(cap), 1), np.uint8)
    written = ctypes.c_size_t(0)
    tout = np.zeros(WC_MAX_LEVELS, np.float32)
    bound = ctypes.c_double(0.0)
    rc = load_library().wc_thin_tol_unit(p.ctypes.data, p.size, float(tol), out.ctypes.data,
                                         out.size if cap is None else int(cap), ctypes.byref(written),
                                         tout.ctypes.data, ctypes.byref(bound))
    if rc != 0:
        raise WaveletError(rc, "wc_thin_tol_unit: refused")
    return out[:written.value].tobytes(), tout[:payload_levels(bytes(payload[:20]))].copy(), float(bound.value)


def split_tol_unit(payload, tol: float, base_cap=None, rest_cap=None):
    """wc_split_tol_unit (host only): the tolerance rule on one standard payload ->
    (base bytes, rest bytes, fp32 thresholds of levels 1..L, bound)."""
    p = np.frombuffer(bytes(payload), np.uint8)
    base = np.empty(max(p.size, 20) if base_cap is None else max(int(base_cap), 1), np.uint8)
    rest = np.empty(max(p.size, 20) if rest_cap is None else max(int(rest_cap), 1), np.uint8)
    bl, rl = ctypes.c_size_t(0), ctypes.c_size_t(0)
    tout = np.zeros(WC_MAX_LEVELS, np.float32)
    bound = ctypes.c_double(0.0)
    rc = load_library().wc_split_tol_unit(p.ctypes.data, p.size, float(tol), base.ctypes.data,
                                          base.size if base_cap is None else int(base_cap), ctypes.byref(bl),
                                          rest.ctypes.data, rest.size if rest_cap is None else int(rest_cap),
                                          ctypes.byref(rl), tout.ctypes.data, ctypes.byref(bound))
    if rc != 0:
        raise WaveletError(rc, "wc_split_tol_unit: refused")
    return (base[:bl.value].tobytes(), rest[:rl.value].tobytes(),
            tout[:payload_levels(bytes(payload[:20]))].copy(), float(bound.value))


def split_bound(units, n: int, max_pairs=None):
    """wc_split_bound -> (base bytes, rest bytes) of split_budget (max_pairs) / split_thresh (None)."""
    k = None if max_pairs is None else _pairs_array(max_pairs, n)
    b, r = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = load_library().wc_split_bound(units, n, None if k is None else k.ctypes.data, ctypes.byref(b), ctypes.byref(r))
    if rc:
        raise WaveletError(rc, "wc_split_bound: invalid argument")
    return int(b.value), int(r.value)


def merge_bound(units, n: int) -> int:
    """wc_merge_bound: the output extent of merge (= payload_bound)."""
    return int(load_library().wc_merge_bound(units, n))


def split_unit(payload, max_pairs=None, thresh=None, base_cap=None, rest_cap=None):
    """wc_split_unit (host only): the rule on one standard payload -> (base bytes, rest
    bytes, T, fp32 thresholds of levels 1..L).  Exactly one of max_pairs (K) and thresh."""
    p = np.frombuffer(bytes(payload), np.uint8)
    base = np.empty(max(p.size, 20) if base_cap is None else max(int(base_cap), 1), np.uint8)
    rest = np.empty(max(p.size, 20) if rest_cap is None else max(int(rest_cap), 1), np.uint8)
    bl, rl = ctypes.c_size_t(0), ctypes.c_size_t(0)
    key = ctypes.c_uint32(0)
    tout = np.zeros(WC_MAX_LEVELS, np.float32)
    k = None if max_pairs is None else ctypes.c_uint32(int(max_pairs))
    t = None if thresh is None else np.ascontiguousarray(np.resize(np.asarray(thresh, np.float32), WC_MAX_LEVELS))
    rc = load_library().wc_split_unit(p.ctypes.data, p.size, None if k is None else ctypes.addressof(k),
                                      None if t is None else t.ctypes.data, base.ctypes.data,
                                      base.size if base_cap is None else int(base_cap), ctypes.byref(bl),
                                      rest.ctypes.data, rest.size if rest_cap is None else int(rest_cap),
                                      ctypes.byref(rl), ctypes.byref(key), tout.ctypes.data)
    if rc != 0:
        raise WaveletError(rc, "wc_split_unit: refused")
    return (base[:bl.value].tobytes(), rest[:rl.value].tobytes(), int(key.value),
            tout[:payload_levels(bytes(payload[:20]))].copy())


def merge_unit(a, b, cap=None):
    """wc_merge_unit (host only): the union of two standard payloads of one unit -> bytes."""
    pa, pb = np.frombuffer(bytes(a), np.uint8), np.frombuffer(bytes(b), np.uint8)
    out = np.empty(max(pa.size + pb.size, 20) if cap is None else max(int(cap), 1), np.uint8)
    written = ctypes.c_size_t(0)
    rc = load_library().wc_merge_unit(pa.ctypes.data, pa.size, pb.ctypes.data, pb.size, out.ctypes.data,
                                      out.size if cap is None else int(cap), ctypes.byref(written))
    if rc != 0:
        raise WaveletError(rc, "wc_merge_unit: refused")
    return out[:written.value].tobytes()


def budget_thresholds(key: int, levels: int):
    """wc_budget_thresholds (host only): the fp32 thresholds of levels 1..L that
    keep exactly the candidates whose key is above `key`."""
    t = (ctypes.c_float * WC_MAX_LEVELS)()
    rc = load_library().wc_budget_thresholds(int(key), int(levels), t)
    if rc:
        raise WaveletError(rc, "wc_budget_thresholds: invalid argument")
    return [float(t[l]) for l in range(int(levels))]


def budget_select(flat: np.ndarray, dims, levels: int, max_pairs: int):
    """wc_budget_select (host only): (T, fp32 thresholds of levels 1..L, kept) of
    the size-budget rule on one unit's final flat array, dims = (W, H, D)."""
    f = np.ascontiguousarray(flat, dtype=np.float32).ravel()
    W, H, D = (int(v) for v in dims)
    if W >= 0 and H >= 0 and D >= 0 and f.size != W * H * D:
        raise ValueError("flat must have W * H * D values")
    t = (ctypes.c_float * WC_MAX_LEVELS)()
    key, kept = ctypes.c_uint32(), ctypes.c_uint32()
    rc = load_library().wc_budget_select(f.ctypes.data, W, H, D, int(levels), int(max_pairs), ctypes.byref(key), t,
                                         ctypes.byref(kept))
    if rc:
        raise WaveletError(rc, "wc_budget_select: invalid argument")
    return int(key.value), [float(t[l]) for l in range(int(levels))], int(kept.value)


def maxerr_select(flat: np.ndarray, cells: np.ndarray, dims, levels: int, maxerr: float):
    """wc_maxerr_select (host only): (thresh, err, b*) of the max-error rule on
    one unit: flat = its final flat array, cells = its cells (float32 or float64,
    x fastest), dims = (W, H, D)."""
    f = np.ascontiguousarray(flat, dtype=np.float32).ravel()
    x = np.ascontiguousarray(cells).ravel()
    if x.dtype not in (np.float32, np.float64):
        raise TypeError("cells must be float32 or float64")
    W, H, D = (int(v) for v in dims)
    if W >= 0 and H >= 0 and D >= 0 and (f.size != W * H * D or x.size != W * H * D):
        raise ValueError("flat and cells must have W * H * D values")
    t, e, b = ctypes.c_float(), ctypes.c_double(), ctypes.c_uint32()
    rc = load_library().wc_maxerr_select(f.ctypes.data, x.ctypes.data, WC_F64 if x.dtype == np.float64 else WC_F32,
                                         W, H, D, int(levels), float(maxerr), ctypes.byref(t), ctypes.byref(e),
                                         ctypes.byref(b))
    if rc:
        raise WaveletError(rc, "wc_maxerr_select: invalid argument")
    return float(t.value), float(e.value), int(b.value)


def unit_payload(payload: np.ndarray, offsets: np.ndarray, kept: np.ndarray, u: int) -> bytes:
    """Unit u's serialized bytes (reference src/compressor.cpp:55-80 layout)."""
    o = int(offsets[u])
    return payload[o:o + 20 + 8 * int(kept[u])].tobytes()
