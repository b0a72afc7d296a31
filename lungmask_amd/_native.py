"""ctypes binding of liblungmask_hip.so (include/lungmask_hip.h).

The product path has NO CPU fallback: if the HIP library is missing or no GPU is
visible, `load()` / `Engine()` raise.  (`tests/` may point `Library` at the
g++-built emulation of the same kernel sources; that library reports
`lm_is_gpu_build() == 0` and is refused here unless explicitly allowed.)
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import Dict, Optional, Sequence

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(HERE, "liblungmask_hip.so")

LM_DTYPES = {
    np.dtype(np.int16): 0,
    np.dtype(np.int32): 1,
    np.dtype(np.float32): 2,
    np.dtype(np.float64): 3,
    np.dtype(np.uint8): 4,
    np.dtype(np.uint16): 5,
    np.dtype(np.int64): 6,
}


# output dtypes of the probability maps (include/lungmask_hip.h: lm_uncrop_probs_dev, lm_apply_probs_dev)
LM_PROB_DTYPES = {np.dtype(np.float32): 2, np.dtype(np.float16): 7}


class LMError(RuntimeError):
    pass


class LabelStats(C.Structure):
    """include/lungmask_hip.h: lm_label_stats."""
    _fields_ = [("voxels", C.c_int64), ("nonfinite", C.c_int64), ("clipped_low", C.c_int64), ("clipped_high", C.c_int64),
                ("hu_min", C.c_int64), ("hu_max", C.c_int64), ("index_sum", C.c_int64 * 3), ("bbox", C.c_int32 * 6)]


class TextureParams(C.Structure):
    """include/lungmask_hip.h: lm_texture_params."""
    _fields_ = [(f, C.c_int32) for f in ("lo", "hi", "bin_width", "distance", "nr")]


class TextureCounts(C.Structure):
    """include/lungmask_hip.h: lm_texture_counts."""
    _fields_ = [(f, C.c_int64) for f in ("voxels", "valid", "nonfinite", "below", "above", "longest_run")]


TEXTURE_DIRECTIONS = tuple((dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) > (0, 0, 0))
TEXTURE_COUNT_FIELDS = ("voxels", "valid", "nonfinite", "below", "above", "longest_run")


class LabelAgreement(C.Structure):
    """include/lungmask_hip.h: lm_label_agreement."""
    _fields_ = [(f, C.c_int64) for f in ("voxels_a", "voxels_b", "intersection", "surface_a", "surface_b", "other_a", "other_b")] + \
               [("sum_d_ab", C.c_double), ("sum_d_ba", C.c_double), ("max_d2_ab", C.c_float), ("max_d2_ba", C.c_float),
                ("order_ab", C.c_float * 2 * 8), ("order_ba", C.c_float * 2 * 8), ("order_pooled", C.c_float * 2 * 8),
                ("bbox", C.c_int32 * 6)]


AGREEMENT_MAX_PERCENTILES = 8


class RoiParams(C.Structure):
    """include/lungmask_hip.h: lm_roi_params."""
    _fields_ = [("bbox", C.c_int32 * 6), ("out_dims", C.c_int32 * 3), ("step", C.c_double * 3), ("keep", C.c_uint8 * 256),
                ("dilate_mm", C.c_double), ("spacing", C.c_double * 3), ("fill", C.c_double), ("window_lo", C.c_double),
                ("window_hi", C.c_double), ("flags", C.c_uint32), ("out_dtype", C.c_int32)]


ROI_MASK_OUTSIDE, ROI_WINDOW = 1, 2

# output dtypes of the ROI image (include/lungmask_hip.h: lm_roi_dev)
LM_ROI_DTYPES = {np.dtype(np.float32): 2, np.dtype(np.float16): 7, np.dtype(np.int16): 0}


class ResampleParams(C.Structure):
    """include/lungmask_hip.h: lm_resample_params."""
    _fields_ = [("out_dims", C.c_int32 * 3), ("mode", C.c_int32), ("A", C.c_double * 9), ("b", C.c_double * 3), ("fill", C.c_double),
                ("out_dtype", C.c_int32)]


RESAMPLE_MODES = {"nearest": 0, "linear": 1, "cubic": 2, "label_linear": 3}


class JointHistParams(C.Structure):
    """include/lungmask_hip.h: lm_joint_hist_params."""
    _fields_ = [("A", C.c_double * 9), ("b", C.c_double * 3), ("start", C.c_int32 * 3), ("step", C.c_int32 * 3), ("bins", C.c_int32),
                ("mode", C.c_int32), ("f_lo", C.c_int32), ("f_width", C.c_int32), ("m_lo", C.c_int32), ("m_width", C.c_int32),
                ("keep", C.c_uint8 * 256)]


JOINT_HIST_MODES = {"linear": 0, "nearest": 1}
JOINT_HIST_Q = 65536  # the weight of one sample


class DemonsParams(C.Structure):
    """include/lungmask_hip.h: lm_demons_params."""
    _fields_ = [("A", C.c_double * 9), ("b", C.c_double * 3), ("field_scale", C.c_double * 3), ("grad_scale", C.c_double * 3),
                ("inv_k2", C.c_double), ("den_min", C.c_double), ("keep", C.c_uint8 * 256)]


DEMONS_COUNTS = ("selected", "contributed", "outside", "nan", "ssd16")  # counts_out of lm_demons_step_dev; ssd16: 16 x the squared sum


class LccParams(C.Structure):
    """include/lungmask_hip.h: lm_lcc_params."""
    _fields_ = [("A", C.c_double * 9), ("b", C.c_double * 3), ("field_scale", C.c_double * 3), ("grad_scale", C.c_double * 3),
                ("inv_k2", C.c_double), ("den_min", C.c_double), ("var_eps", C.c_double), ("a_max", C.c_double),
                ("moving_dims", C.c_int32 * 3), ("keep", C.c_uint8 * 256)]


# counts_out of lm_lcc_step_dev; ssd16: 16 x the sum of the squared residuals; rho2q: LCC_Q x the sum of the squared local correlations
LCC_COUNTS = ("selected", "contributed", "outside", "nan", "ssd16", "rho2q")
LCC_Q = 1 << 20
LCC_MAX_RADIUS = 8


class FieldCombineParams(C.Structure):
    """include/lungmask_hip.h: lm_field_combine_params."""
    _fields_ = [("out_dims", C.c_int32 * 3), ("A", C.c_double * 9), ("b", C.c_double * 3), ("field_scale", C.c_double * 3),
                ("R", C.c_double * 9), ("alpha", C.c_double), ("beta", C.c_double)]


# counts_out of lm_field_combine_dev; sum_q, max_q: the squared difference from `ref` in units of 2^-22 (FIELD_Q per squared unit)
FIELD_COUNTS = ("outside", "nan", "sum_q", "max_q")
FIELD_Q = 4194304


class PairParams(C.Structure):
    """include/lungmask_hip.h: lm_pair_params."""
    _fields_ = [("A", C.c_double * 9), ("b", C.c_double * 3), ("field_scale", C.c_double * 3), ("jac_scale", C.c_double), ("air", C.c_double),
                ("fixed_thr", C.c_double), ("moving_thr", C.c_double), ("lo", C.c_double), ("hi", C.c_double), ("n_labels", C.c_int32),
                ("keep", C.c_uint8 * 256)]


# the columns of lm_pair_map_dev's table; sum_j in units of 2^-20 (PAIR_J_Q per unit), sum_change and sum_change2 in 1/16 (PAIR_C_Q per
# HU and per HU^2); code1 .. code4: the classes 1 + (f < fixed_thr) + 2 * (m < moving_thr)
LM_PAIR_COLS = 13
PAIR_COLS = ("selected", "valid", "outside", "nonfinite", "folded", "sum_j", "sum_change", "sum_change2", "excluded", "code1", "code2", "code3",
             "code4")
PAIR_J_Q = 1048576
PAIR_C_Q = 16


class MorphParams(C.Structure):
    """include/lungmask_hip.h: lm_morph_params."""
    _fields_ = [("op", C.c_int32), ("radius_mm", C.c_double), ("spacing", C.c_double * 3), ("keep", C.c_uint8 * 256),
                ("into", C.c_uint8 * 256)]


MORPH_OPS = {"dilate": 0, "erode": 1, "open": 2, "close": 3}


class ComponentsParams(C.Structure):
    """include/lungmask_hip.h: lm_components_params."""
    _fields_ = [("keep", C.c_uint8 * 256), ("lo", C.c_int32), ("hi", C.c_int32), ("has_lo", C.c_int32), ("has_hi", C.c_int32),
                ("per_label", C.c_int32), ("connectivity", C.c_int32)]


# include/lungmask_hip.h: lm_component, as a numpy record (a table can hold 10^6 rows)
COMPONENT_DTYPE = np.dtype([("voxels", "<i8"), ("index_sum", "<i8", (3,)), ("hu_sum", "<i8"), ("faces", "<i8", (3,)), ("bbox", "<i4", (6,)),
                            ("hu_min", "<i4"), ("hu_max", "<i4"), ("label", "<i4"), ("first", "<i4")])
assert COMPONENT_DTYPE.itemsize == 104


class FilterParams(C.Structure):
    """include/lungmask_hip.h: lm_filter_params."""
    _fields_ = [("kind", C.c_int32), ("size", C.c_int32 * 3), ("radius", C.c_int32 * 3), ("taps", C.c_float * 65 * 3),
                ("keep", C.c_uint8 * 256), ("flags", C.c_uint32), ("ind_lo", C.c_int32), ("ind_hi", C.c_int32), ("fill", C.c_float)]


FILTER_MEDIAN, FILTER_SEPARABLE = 0, 1
FILTER_MASKED, FILTER_INDICATOR, FILTER_FILL_OUTSIDE = 1, 2, 4
FILTER_MAX_RADIUS = 32


class VesselScale(C.Structure):
    """include/lungmask_hip.h: lm_vessel_scale."""
    _fields_ = [("radius", C.c_int32 * 3), ("taps", C.c_float * 65 * 3 * 3), ("nrm", C.c_float * 6)]


VESSEL_MASKED, VESSEL_DARK = 1, 2
VESSEL_MAX_SCALES = 8
VESSEL_COUNT_COLUMNS = 9


class VesselParams(C.Structure):
    """include/lungmask_hip.h: lm_vessel_params."""
    _fields_ = [("keep", C.c_uint8 * 256), ("flags", C.c_uint32), ("ka", C.c_float), ("kb", C.c_float), ("kc", C.c_float),
                ("n_scales", C.c_int32), ("scales", VesselScale * VESSEL_MAX_SCALES)]


CALIBRE_MAX_EDGES = 7  # include/lungmask_hip.h: LM_CALIBRE_MAX_EDGES, LM_CALIBRE_COLUMNS
CALIBRE_COLUMNS = 9
SEED_MAX = 64  # include/lungmask_hip.h: LM_SEED_MAX


class NoKeptVoxel(ValueError):
    """morph_dev: no voxel of the labels carries a kept label value (lm_morph_dev's "no kept voxel")."""


# the HU histogram of lm_label_stats_dev: bin b holds clip(hu, -1024, 3071) == b - 1024
STATS_HU_LO, STATS_BINS = -1024, 4096


class _Tensor(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.POINTER(C.c_float)), ("numel", C.c_int64)]


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int64), ("total_ms", C.c_double), ("flops", C.c_double), ("bytes", C.c_double)]


class LaunchSpan(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("lane", C.c_int), ("start_ms", C.c_double), ("end_ms", C.c_double)]


_INT = object()  # restype left at ctypes' default (int: the status)
_P, _I, _I64, _SZ, _F = C.c_void_p, C.c_int, C.c_int64, C.c_size_t, C.c_float
_PTR = C.POINTER


def _sig(*argtypes, restype=_INT, optional=False):
    return (list(argtypes), restype, optional)


def _opt(*argtypes, restype=_INT):
    """An entry point that may be absent: older builds that tools/ab_forward.py loads for comparison lack the newer ones, and
    callers probe for those with hasattr at call time."""
    return _sig(*argtypes, restype=restype, optional=True)


# include/lungmask_hip.h: name -> (argtypes, restype, may be absent from the library)
_ENTRY_POINTS = {
    "lm_last_error": (None, C.c_char_p, False),
    "lm_version": (None, C.c_char_p, False),
    "lm_engine_create": _sig(_PTR(_P), _I),
    "lm_engine_destroy": _sig(_P, restype=None),
    "lm_engine_sync": _sig(_P),
    "lm_dev_alloc": _sig(_P, _PTR(_P), _SZ),
    "lm_dev_free": _sig(_P, _P),
    "lm_copy_h2d": _sig(_P, _P, _P, _SZ),
    "lm_copy_d2h": _sig(_P, _P, _P, _SZ),
    "lm_host_alloc": _opt(_P, _PTR(_P), _SZ),
    "lm_host_free": _opt(_P, _P),
    "lm_model_load": _sig(_P, _I, _PTR(_Tensor), _I),
    "lm_model_classes": _sig(_P, _I),
    "lm_engine_stream": _opt(_P, restype=_P),
    "lm_dist_unique_id": _opt(_P),
    "lm_dist_init": _opt(_P, _I, _I, _P),
    "lm_dist_rank": _opt(_P),
    "lm_dist_world": _opt(_P),
    "lm_dist_all_gather": _opt(_P, _P, _P, _SZ),
    "lm_dist_destroy": _opt(_P),
    "lm_model_precision": _opt(_P, _I),
    "lm_model_probe_error": _opt(_P, _I, _PTR(_F)),
    "lm_model_chain_limit": _opt(_P, _I),
    "lm_forward_dev": _sig(_P, _I, _P, _I, _I, _I, _P, _P),
    "lm_set_precision": _sig(_P, _I),
    "lm_set_streams": _sig(_P, _I),
    "lm_set_fusion": _sig(_P, _I),
    "lm_forward_batches_dev": _sig(_P, _I, _P, _I, _I, _I, _I, _P),
    "lm_preprocess_dev": _sig(_P, _P, _I, *[_I] * 5, *[_P] * 4),
    "lm_reshape_mask_dev": _sig(_P, _P, _P, *[_I] * 5, _P),
    "lm_uncrop_probs_dev": _opt(_P, _P, _P, *[_I] * 7, _P),
    "lm_apply_probs_dev": _opt(_P, _I, _P, *[_I] * 6, _P, _I, _P),
    "lm_reorient_dev": _sig(_P, _P, _P, *[_I] * 4, *[_I64] * 4),
    "lm_postprocess_dev": _sig(_P, _P, _I, _I, _I, _PTR(_I), _I, _I),
    "lm_bbox3d_dev": _opt(_P, _P, _I, _I, _I, _I, _PTR(C.c_int32)),
    "lm_keep_largest_dev": _opt(_P, _P, _I, _I, _I, _PTR(_I64)),
    "lm_label_stats_dev": _opt(_P, _P, _P, *[_I] * 5, _PTR(LabelStats), _P, _PTR(_I64)),
    "lm_texture_dev": _opt(_P, _P, _P, *[_I] * 5, _PTR(TextureParams), _PTR(TextureCounts), _P, _P),
    "lm_edt_dev": _opt(_P, _P, _I, _I, _I, _PTR(C.c_double), _P),
    "lm_label_agreement_dev": _opt(_P, _P, _P, *[_I] * 4, _PTR(C.c_double), _PTR(C.c_double), _I, _PTR(LabelAgreement)),
    "lm_roi_plan_dev": _opt(_P, _P, _I, _I, _I, _PTR(C.c_uint8), _PTR(C.c_int32)),
    "lm_roi_dev": _opt(_P, _P, _I, _P, _I, _I, _I, _PTR(RoiParams), _P, _P),
    "lm_spline_prefilter_dev": _opt(_P, _P, _I, _I, _I, _I, _P),
    "lm_resample_dev": _opt(_P, _P, _I, _I, _I, _I, _PTR(ResampleParams), _P),
    "lm_joint_hist_dev": _opt(_P, _P, _I, _I, _I, _I, _P, _P, _I, _I, _I, _I, _PTR(JointHistParams), _P, _P),
    "lm_warp_dev": _opt(_P, _P, _I, _I, _I, _I, _P, _PTR(ResampleParams), _PTR(C.c_double), _P),
    "lm_demons_step_dev": _opt(_P, _P, _I, _I, _I, _I, _P, _P, _I, _I, _I, _I, _P, _PTR(DemonsParams), _P, _P),
    "lm_jacobian_dev": _opt(_P, _P, _I, _I, _I, _PTR(C.c_double), _P, _P),
    "lm_local_moments_dev": _opt(_P, _P, _P, _I, _I, _I, _PTR(C.c_int32), _P),
    "lm_lcc_step_dev": _opt(_P, _P, _P, _P, _P, _I, _I, _I, _P, _PTR(LccParams), _P, _P),
    "lm_field_combine_dev": _opt(_P, _P, _P, _P, _I, _I, _I, _P, _PTR(FieldCombineParams), _P, _P),
    "lm_pair_map_dev": _opt(_P, _P, _I, _I, _I, _I, _P, _P, _I, _I, _I, _I, _P, _PTR(PairParams), _P, _P, _P, _P),
    "lm_nearest_label_dev": _opt(_P, _P, _I, _I, _I, _PTR(C.c_uint8), _PTR(C.c_double), _P, _P),
    "lm_morph_dev": _opt(_P, _P, _I, _I, _I, _PTR(MorphParams), _P, _PTR(_I64)),
    "lm_components_dev": _opt(_P, _P, _P, _I, _I, _I, _I, _PTR(ComponentsParams), _P, _PTR(_I64), _P),
    "lm_component_table_dev": _opt(_P, _P, _P, _P, _I, _I, _I, _I, _P, _I64, _PTR(_I64)),
    "lm_component_table_launch": _opt(_I64, _PTR(_I64), _PTR(_I64)),
    "lm_relabel_dev": _opt(_P, _P, _P, _I64, _I64, _P),
    "lm_filter_dev": _opt(_P, _P, _I, _P, _I, _I, _I, _PTR(FilterParams), _P),
    "lm_hessian_dev": _opt(_P, _P, _I, _P, _I, _I, _I, _PTR(VesselParams), _P, _P),
    "lm_vesselness_dev": _opt(_P, _P, _I, _P, _I, _I, _I, _PTR(VesselParams), _P, _P),
    "lm_vessel_counts_dev": _opt(_P, _P, _P, _P, _I, _I, _I, _I, _F, _PTR(_I64)),
    "lm_skeleton_dev": _opt(_P, _P, _I, _I, _I, _PTR(C.c_uint8), _P, _PTR(_I64)),
    "lm_skeleton_points_dev": _opt(_P, _P, _P, _I, _I, _I, _I64, _P, _P, _P, _PTR(_I64)),
    "lm_calibre_dev": _opt(_P, _P, _P, _PTR(C.c_uint8), _P, _I, _I, _I, _PTR(C.c_double), _PTR(C.c_double), _I, _I, _P, _P, _PTR(_I64)),
    "lm_vessel_mask_dev": _opt(_P, _P, _P, _I, _I, _I, _F, _P),
    "lm_seed_cost_dev": _opt(_P, _P, _I, _I, _I, _I, _PTR(_I64), _I, _I, _I64, _P, _P, _PTR(_I64)),
    "lm_seed_cost_bricks": _opt(_I, _I, _I, _PTR(_I64), _PTR(C.c_int32)),
    "lm_airway_mask_dev": _opt(_P, _P, _P, _I, _I, _I, _I, _P, _P),
    "lm_mesh_plan_dev": _opt(_P, _P, _I, _I, _I, _PTR(C.c_uint8), _PTR(C.c_int32), _PTR(_I64), _PTR(_I64)),
    "lm_mesh_dev": _opt(_P, _P, _I, _I, _I, _PTR(C.c_uint8), _I, _F, _F, _P, _I64, _P, _I64),
    "lm_debug_fill_workspaces": _opt(_P, _I, _PTR(_I64)),
    "lm_slab_begin": _sig(_P, _P, *[_I] * 7, _PTR(_I), _I, _I),
    "lm_slab_pending": _sig(_P, restype=_I64),
    "lm_slab_pending_uniform": _sig(_P),
    "lm_slab_emit": _sig(_P, _P),
    "lm_slab_step": _sig(_P, _P, _I64, _PTR(_I64)),
    "lm_postprocess_info": _sig(_P, _PTR(_I64)),
    "lm_fuse_dev": _sig(_P, _P, _P, _SZ, _PTR(_I)),
    "lm_label_max_dev": _sig(_P, _P, _SZ, _PTR(_I)),
    "lm_fuse_spare_dev": _sig(_P, _P, _P, _SZ, _I),
    "lm_apply_dev": _sig(_P, _I, _I, _P, *[_I] * 6, _P),
    "lm_apply_host": _sig(_P, _I, _I, _P, *[_I] * 6, _P),
    "lm_apply_host_ex": _opt(_P, _I, _I, _P, *[_I] * 6, _P, C.c_uint),
    "lm_pipe_upload": _opt(_P, _I, _P, _SZ),
    "lm_pipe_apply": _opt(_P, *[_I] * 9),
    "lm_pipe_download": _opt(_P, _I, _P, _SZ),
    "lm_pipe_wait": _opt(_P, _I),
    "lm_pipe_query": _opt(_P, _I),
    "lm_profile_enable": _sig(_P, _I),
    "lm_profile_reset": _sig(_P),
    "lm_profile_read": _sig(_P, _PTR(KernelStat), _I),
    "lm_profile_timeline": _opt(_P, _PTR(LaunchSpan), _I),
}


class Library:
    def __init__(self, path: Optional[str] = None, allow_emulation: bool = False):
        path = path or os.environ.get("LUNGMASK_HIP_LIB") or DEFAULT_LIB
        if not os.path.exists(path):
            raise LMError(
                f"{path} not found: build it with `python -m lungmask_amd.build` (hipcc, gfx950). "
                "lungmask_amd has no CPU fallback."
            )
        self.path = path
        self.lib = C.CDLL(path)
        L = self.lib
        for name, (argtypes, restype, optional) in _ENTRY_POINTS.items():
            if optional and not hasattr(L, name):
                continue
            fn = getattr(L, name)  # (a required entry point that is missing: AttributeError)
            if argtypes is not None:
                fn.argtypes = argtypes
            if restype is not _INT:
                fn.restype = restype
        self.is_gpu = bool(L.lm_is_gpu_build())
        if not self.is_gpu and not allow_emulation:
            raise LMError(f"{path} is not a GPU build; refusing to run the product path on an emulation library")

    def check(self, status: int, what: str = ""):
        if status < 0:
            raise LMError(f"{what or 'lungmask_hip'} failed ({status}): {self.lib.lm_last_error().decode()}")
        return status


_default: Optional[Library] = None


def load() -> Library:
    global _default
    if _default is None:
        _default = Library()
    return _default


class DeviceArray:
    """A typed device allocation owned by an Engine (freed with it or via free())."""

    def __init__(self, eng: "Engine", shape, dtype):
        self.eng = eng
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        p = C.c_void_p()
        eng.L.check(eng.L.lib.lm_dev_alloc(eng.h, C.byref(p), self.nbytes), "lm_dev_alloc")
        self.ptr = p.value

    def upload(self, arr: np.ndarray) -> "DeviceArray":
        a = np.ascontiguousarray(arr, dtype=self.dtype)
        assert a.nbytes == self.nbytes, (a.shape, self.shape)
        self.eng.L.check(self.eng.L.lib.lm_copy_h2d(self.eng.h, self.ptr, a.ctypes.data, self.nbytes), "lm_copy_h2d")
        return self

    def download(self) -> np.ndarray:
        out = np.empty(self.shape, dtype=self.dtype)
        self.eng.L.check(self.eng.L.lib.lm_copy_d2h(self.eng.h, out.ctypes.data, self.ptr, self.nbytes), "lm_copy_d2h")
        return out

    def download_into(self, out: np.ndarray) -> np.ndarray:
        """Copies the whole array into `out` (C-contiguous, same byte size): page-locked memory there takes the copy at link speed."""
        assert out.flags.c_contiguous and out.nbytes == self.nbytes, (out.shape, out.dtype, self.shape, self.dtype)
        self.eng.L.check(self.eng.L.lib.lm_copy_d2h(self.eng.h, out.ctypes.data, self.ptr, self.nbytes), "lm_copy_d2h")
        return out

    def view(self, offset_bytes: int, shape, dtype=None) -> "DeviceView":
        """A non-owning typed window into this allocation (e.g. one class map of a [C][n][h][w] stack)."""
        return DeviceView(self, offset_bytes, shape, dtype or self.dtype)

    def free(self):
        if self.ptr:
            self.eng.L.lib.lm_dev_free(self.eng.h, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            if self.ptr and self.eng.h:
                self.free()
        except Exception:
            pass


class DeviceView(DeviceArray):
    """Part of a DeviceArray: same interface, owns nothing (the parent must outlive it)."""

    def __init__(self, parent: DeviceArray, offset_bytes: int, shape, dtype):
        self.eng = parent.eng
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        assert 0 <= offset_bytes and offset_bytes + self.nbytes <= parent.nbytes
        self._parent = parent
        self.ptr = parent.ptr + int(offset_bytes)

    def free(self):
        self.ptr = None

    def __del__(self):
        pass


class DeviceScope:
    """The device arrays of one piece of work: everything uploaded, allocated or registered (`add`) through the scope is freed when
    it is left, on every path.  What the host forms below and LMInferer's apply_* methods are built on (`Engine.scope()`)."""

    def __init__(self, eng: "Engine"):
        self.eng = eng
        self.arrays = []

    def add(self, *arrays):
        """Hands device arrays (None is skipped) over to the scope -> the one array, or the tuple of them."""
        self.arrays += [d for d in arrays if d is not None]
        return arrays[0] if len(arrays) == 1 else arrays

    def upload(self, arr: np.ndarray, dtype=None) -> DeviceArray:
        return self.add(self.eng.to_device(arr if dtype is None else np.ascontiguousarray(arr, dtype=dtype)))

    def empty(self, shape, dtype) -> DeviceArray:
        return self.add(self.eng.empty(shape, dtype))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for d in self.arrays:
            d.free()


@contextlib.contextmanager
def engine_scope(engine: Optional["Engine"] = None):
    """`engine`, or -- when none was passed -- a new Engine(0) that is closed on exit: the `engine=None` of every stand-alone
    function of the package."""
    own = engine is None
    eng = Engine(0) if own else engine
    try:
        yield eng
    finally:
        if own:
            eng.close()


def _ptr(a: Optional[DeviceArray]):
    """The device pointer of an optional array (None: NULL)."""
    return a.ptr if a is not None else None


def _mat9(M):
    """A 3 x 3 matrix as the nine floats of a params struct, row-major."""
    return [float(v) for v in np.asarray(M, np.float64).reshape(9)]


def _affine_into(p, A, b):
    """Fills the `A` and `b` of a params struct (index map: A @ o + b)."""
    p.A[:] = _mat9(A)
    p.b[:] = [float(v) for v in np.asarray(b, np.float64).reshape(3)]


class Engine:
    """One device + one HIP stream + workspaces (lm_engine)."""

    def __init__(self, device_id: int = 0, library: Optional[Library] = None):
        self.L = library or load()
        h = C.c_void_p()
        self.L.check(self.L.lib.lm_engine_create(C.byref(h), device_id), "lm_engine_create")
        self.h = h.value
        self.device_id = int(device_id)

    def close(self):
        if getattr(self, "h", None):
            self.L.lib.lm_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def debug_fill_workspaces(self, byte: int) -> int:
        """TEST SEAM (lm_debug_fill_workspaces): sets every scratch workspace the engine owns, device and pinned host, to `byte`
        -> the number of bytes written.  Results after it must be what a new engine returns."""
        filled = C.c_int64()
        self.L.check(self.L.lib.lm_debug_fill_workspaces(self.h, int(byte), C.byref(filled)), "lm_debug_fill_workspaces")
        return int(filled.value)

    # -- memory
    def empty(self, shape, dtype) -> DeviceArray:
        return DeviceArray(self, shape, dtype)

    def to_device(self, arr: np.ndarray) -> DeviceArray:
        arr = np.ascontiguousarray(arr)
        return DeviceArray(self, arr.shape, arr.dtype).upload(arr)

    def sync(self):
        self.L.check(self.L.lib.lm_engine_sync(self.h), "lm_engine_sync")

    def scope(self) -> DeviceScope:
        return DeviceScope(self)

    @contextlib.contextmanager
    def _out_or_new(self, out: Optional[DeviceArray], shape, dtype):
        """The caller's `out`, or a new DeviceArray that is freed again if the body raises."""
        own = out is None
        if own:
            out = self.empty(shape, dtype)
        try:
            yield out
        except BaseException:
            if own:
                out.free()
            raise

    @contextlib.contextmanager
    def _optional_new(self, wanted: bool, shape, dtype, out: Optional[DeviceArray] = None):
        """The caller's `out` or a new DeviceArray that is freed again if the body raises, or None when the optional result is not
        `wanted`."""
        if not wanted:
            yield None
            return
        with self._out_or_new(out, shape, dtype) as arr:
            yield arr

    # -- argument checks shared by the entry points: each raises in the name (`who`) or with the text of its caller
    @staticmethod
    def _lm_dtype(dtype, who: str = "", signed_only: bool = False, text: Optional[str] = None) -> int:
        """The library's code of a volume dtype (`signed_only`: uint8 / uint16 are refused too)."""
        code = LM_DTYPES.get(np.dtype(dtype))
        if code is None or (signed_only and code in (4, 5)):
            raise LMError(text or f"{who + ': ' if who else ''}unsupported volume dtype {dtype}")
        return code

    @staticmethod
    def _check_labels_and_volume(who: str, lab: DeviceArray, vol: DeviceArray):
        if lab.dtype != np.uint8 or len(lab.shape) != 3 or tuple(lab.shape) != tuple(vol.shape):
            raise LMError(f"{who}: need u8 labels and a volume of the same 3-D shape (got {lab.shape} {lab.dtype}, {vol.shape})")

    @staticmethod
    def _check_size(who: str, shape):
        """lm_edt_dev's limits, checked before a result of that size is allocated."""
        n, h, w = shape
        if max(n, h, w) > 4096 or n * h * w >= 2 ** 31 - 1:
            raise LMError(f"{who}: volume too large (every dimension <= 4096 and n * h * w below 2^31)")

    def _check_kept(self, rc: int, what: str, exc, text: str, keep):
        """`check(rc, what)`, the library's "no kept voxel" raised as `exc`: `text` and the kept label values."""
        if rc < 0 and b"no kept voxel" in self.L.lib.lm_last_error():
            raise exc(text + ("" if keep is None else f" {sorted(set(keep))}"))
        self.L.check(rc, what)

    def host_alloc(self, nbytes: int) -> int:
        """Page-locked host memory (lm_host_alloc) -> address.  The caller owns it: free with host_free (also after close())."""
        p = C.c_void_p()
        self.L.check(self.L.lib.lm_host_alloc(self.h, C.byref(p), int(nbytes)), "lm_host_alloc")
        return int(p.value)

    def host_free(self, addr: int):
        self.L.check(self.L.lib.lm_host_free(self.h if getattr(self, "h", None) else None, C.c_void_p(addr)), "lm_host_free")

    # -- model
    def load_state_dict(self, slot: int, state_dict: Dict[str, "np.ndarray"]) -> int:
        """state_dict: name -> array-like (torch tensors are converted with .numpy())."""
        keep, names, arrs = [], [], []
        for k, v in state_dict.items():
            if hasattr(v, "detach"):
                v = v.detach().cpu().numpy()
            a = np.asarray(v)
            if a.dtype.kind != "f":
                continue  # num_batches_tracked
            a = np.ascontiguousarray(a, dtype=np.float32)
            names.append(k.encode())
            arrs.append(a)
        tens = (_Tensor * len(arrs))()
        for i, (n, a) in enumerate(zip(names, arrs)):
            tens[i].name = n
            tens[i].data = a.ctypes.data_as(C.POINTER(C.c_float))
            tens[i].numel = a.size
        keep.append((names, arrs))
        self.L.check(self.L.lib.lm_model_load(self.h, slot, tens, len(arrs)), "lm_model_load")
        return self.L.check(self.L.lib.lm_model_classes(self.h, slot))

    def stream_handle(self) -> int:
        """hipStream_t of the engine as an integer (0 under emulation): see lm_engine_stream in include/lungmask_hip.h."""
        if not hasattr(self.L.lib, "lm_engine_stream"):  # an older build of the library: the documented fall-back (host syncs)
            return 0
        return int(self.L.lib.lm_engine_stream(self.h) or 0)

    # -- one rank per engine: the RCCL communicator behind the C ABI (include/lungmask_hip.h: lm_dist_*)
    def dist_unique_id(self) -> bytes:
        """128 opaque bytes that rank 0 creates and every rank passes to dist_init (ncclUniqueId)."""
        buf = (C.c_uint8 * 128)()
        self.L.check(self.L.lib.lm_dist_unique_id(buf), "lm_dist_unique_id")
        return bytes(buf)

    def dist_init(self, rank: int, world: int, unique_id: Optional[bytes] = None):
        if unique_id is not None and len(unique_id) != 128:
            raise ValueError("unique_id must be the 128 bytes of dist_unique_id()")
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id) if unique_id is not None else None
        self.L.check(self.L.lib.lm_dist_init(self.h, int(rank), int(world), buf), "lm_dist_init")

    def dist_all_gather(self, send_ptr: int, recv_ptr: int, nbytes: int):
        """Equal-size all-gather of device buffers, enqueued on the engine's stream (recv holds world * nbytes)."""
        self.L.check(self.L.lib.lm_dist_all_gather(self.h, send_ptr, recv_ptr, int(nbytes)), "lm_dist_all_gather")

    def dist_destroy(self):
        self.L.check(self.L.lib.lm_dist_destroy(self.h), "lm_dist_destroy")

    def n_classes(self, slot: int) -> int:
        return self.L.check(self.L.lib.lm_model_classes(self.h, slot), "lm_model_classes")

    def model_precision(self, slot: int) -> str:
        """'split_f16' or 'f32': what the next forward of `slot` runs on (a model whose activations left the f16 range is
        pinned to 'f32' by the engine's range guard)."""
        return "split_f16" if self.L.check(self.L.lib.lm_model_precision(self.h, slot), "lm_model_precision") == 1 else "f32"

    # -- network
    def model_probe(self, slot: int):
        """(max |delta log-prob| split-f16 vs exact fp32 on the load-time probe slice or None when no probe ran, pinned by it?)"""
        err = C.c_float()
        rc = self.L.lib.lm_model_probe_error(self.h, slot, C.byref(err))
        self.L.check(min(rc, 0), "lm_model_probe_error")
        return (None if err.value < 0 else float(err.value)), rc == 1

    def model_tier(self, slot: int) -> str:
        """'split_f16' (fast form), 'split_f16_chain<K>' (the accuracy guard's middle tiers: 3x3 convs split along K, no accumulator chain
        over K products) or 'f32'."""
        err = C.c_float()
        rc = self.L.lib.lm_model_probe_error(self.h, slot, C.byref(err))
        self.L.check(min(rc, 0), "lm_model_probe_error")
        if self.model_precision(slot) == "f32":
            return "f32"
        return f"split_f16_chain{self.L.lib.lm_model_chain_limit(self.h, slot)}" if rc == 2 else "split_f16"

    def set_precision(self, mode):
        """'f32' / 0: exact fp32 matrix ops;  'split_f16' / 1: 3-product split-f16."""
        m = {"f32": 0, "split_f16": 1}.get(mode, mode)
        self.L.check(self.L.lib.lm_set_precision(self.h, int(m)), "lm_set_precision")

    def set_streams(self, n: int):
        self.L.check(self.L.lib.lm_set_streams(self.h, int(n)), "lm_set_streams")

    def set_fusion(self, mask: int):
        """Bit 0: first conv inside conv 2's loader (bit-identical to the stand-alone kernel); bit 1: reserved (bilinear x2 inside the
        decoder conv's loader: not built); bit 2: split-K of the 16 x 16 / 32 x 32 decoder 1x1 convs (fixed order, last bits differ;
        measured slower -- off by default); bit 3: head inside the last conv's epilogue (fp32 instead of the stored 22-bit tensor:
        last bits differ).  Default 11 (A/B and test hook)."""
        self.L.check(self.L.lib.lm_set_fusion(self.h, int(mask)), "lm_set_fusion")

    def forward_dev(self, slot: int, x: DeviceArray, labels: Optional[DeviceArray] = None, logp: Optional[DeviceArray] = None):
        b, h, w = x.shape
        self.L.check(
            self.L.lib.lm_forward_dev(self.h, slot, x.ptr, b, h, w, labels.ptr if labels else None, logp.ptr if logp else None),
            "lm_forward_dev",
        )

    def forward(self, slot: int, x: np.ndarray, want_logp: bool = True):
        """x: f32 [b,h,w] (or [b,1,h,w]) host -> (labels u8 [b,h,w], logp f32 [b,C,h,w] or None)."""
        x = np.asarray(x, dtype=np.float32)
        if x.ndim == 4:
            x = x[:, 0]
        b, h, w = x.shape
        c = self.n_classes(slot)
        with self.scope() as dev:
            xd = dev.upload(x)
            ld = dev.empty((b, h, w), np.uint8)
            pd = dev.empty((b, c, h, w), np.float32) if want_logp else None
            self.forward_dev(slot, xd, ld, pd)
            self.sync()
            return ld.download(), (pd.download() if pd else None)

    # -- pre-processing
    def preprocess_dev(self, vol: DeviceArray, bbox: DeviceArray, x_f32: Optional[DeviceArray] = None,
                       x_i16: Optional[DeviceArray] = None, bmask: Optional[DeviceArray] = None, resolution=(256, 256)):
        n, h, w = vol.shape
        self.L.check(
            self.L.lib.lm_preprocess_dev(self.h, vol.ptr, self._lm_dtype(vol.dtype), n, h, w, int(resolution[0]), int(resolution[1]), bbox.ptr,
                                         x_f32.ptr if x_f32 else None, x_i16.ptr if x_i16 else None, bmask.ptr if bmask else None),
            "lm_preprocess_dev",
        )

    def preprocess(self, vol: np.ndarray, resolution=(256, 256), want_bmask: bool = False):
        """== utils.preprocess + normalisation: returns (x_i16 [n,oh,ow], x_f32, bbox int32 [n,4], bmask|None)."""
        vol = np.ascontiguousarray(vol)
        n, h, w = vol.shape
        with self.scope() as dev:
            vd = dev.upload(vol)
            bb = dev.empty((n, 4), np.int32)
            xf = dev.empty((n, resolution[0], resolution[1]), np.float32)
            xi = dev.empty((n, resolution[0], resolution[1]), np.int16) if vol.dtype.kind == "i" else None
            bm = dev.empty((n, h, w), np.uint8) if want_bmask else None
            self.preprocess_dev(vd, bb, xf, xi, bm, resolution)
            self.sync()
            return (xi.download() if xi else None), xf.download(), bb.download(), (bm.download() if bm else None)

    def reshape_mask_dev(self, mask: DeviceArray, bbox: DeviceArray, out: DeviceArray):
        n, mh, mw = mask.shape
        _, h, w = out.shape
        self.L.check(self.L.lib.lm_reshape_mask_dev(self.h, mask.ptr, bbox.ptr, n, mh, mw, h, w, out.ptr), "lm_reshape_mask_dev")

    def reshape_mask(self, mask: np.ndarray, bbox: np.ndarray, origsize) -> np.ndarray:
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        if mask.ndim == 2:
            mask, bbox = mask[None], np.asarray(bbox)[None]
        n = mask.shape[0]
        with self.scope() as dev:
            md = dev.upload(mask)
            bd = dev.upload(np.ascontiguousarray(bbox, dtype=np.int32).reshape(n, 4))
            od = dev.empty((n, int(origsize[0]), int(origsize[1])), np.uint8)
            self.reshape_mask_dev(md, bd, od)
            self.sync()
            return od.download()

    # -- probability maps (include/lungmask_hip.h: lm_uncrop_probs_dev)
    def uncrop_probs_dev(self, logp: DeviceArray, bbox: DeviceArray, out: DeviceArray):
        """logp f32 [n][C][mh][mw] (the forward's log-softmax), bbox int32 [n][4] -> out [C][n][h][w] float32 or float16:
        exp, ndimage.zoom(order=1) into each slice's box, background fill outside it."""
        n, c, mh, mw = logp.shape
        c2, n2, h, w = out.shape
        if (c2, n2) != (c, n) or out.dtype not in LM_PROB_DTYPES or logp.dtype != np.float32:
            raise LMError(f"uncrop_probs_dev: logp f32 [n][C][mh][mw] and out float32 / float16 [C][n][h][w] (got {logp.shape} "
                          f"{logp.dtype}, {out.shape} {out.dtype})")
        self.L.check(self.L.lib.lm_uncrop_probs_dev(self.h, logp.ptr, bbox.ptr, n, c, mh, mw, h, w, LM_PROB_DTYPES[out.dtype], out.ptr),
                     "lm_uncrop_probs_dev")

    def uncrop_probs(self, logp: np.ndarray, bbox: np.ndarray, origsize, dtype=np.float32) -> np.ndarray:
        """Host form of uncrop_probs_dev: -> [C][n][h][w] of `dtype`."""
        logp = np.ascontiguousarray(logp, dtype=np.float32)
        n, c = logp.shape[:2]
        with self.scope() as dev:
            ld = dev.upload(logp)
            bd = dev.upload(np.ascontiguousarray(bbox, dtype=np.int32).reshape(n, 4))
            od = dev.empty((c, n, int(origsize[0]), int(origsize[1])), dtype)
            self.uncrop_probs_dev(ld, bd, od)
            self.sync()
            return od.download()

    def apply_probs_dev(self, slot: int, vol: DeviceArray, probs: DeviceArray, labels: Optional[DeviceArray] = None, batch_size: int = 20,
                        volume_postprocessing: bool = True):
        """lm_apply_probs_dev: labels u8 [n][h][w] (== apply_dev with no fill model; may be None) and the probability maps
        probs [C][n][h][w] (float32 or float16) of one model."""
        n, h, w = vol.shape
        code = self._lm_dtype(vol.dtype)
        if probs.dtype not in LM_PROB_DTYPES:
            raise LMError(f"probability maps are float32 or float16, not {probs.dtype}")
        self.L.check(
            self.L.lib.lm_apply_probs_dev(self.h, slot, vol.ptr, code, n, h, w, int(batch_size), int(bool(volume_postprocessing)),
                                          labels.ptr if labels is not None else None, LM_PROB_DTYPES[probs.dtype], probs.ptr),
            "lm_apply_probs_dev",
        )

    def apply_probs(self, slot: int, vol: np.ndarray, batch_size: int = 20, volume_postprocessing: bool = True, dtype=np.float32,
                    labels_out: Optional[np.ndarray] = None, probs_out: Optional[np.ndarray] = None):
        """numpy -> (labels u8 [n][h][w], probs [C][n][h][w] of `dtype`) through device buffers.  The maps are the big transfer
        (C x the volume's voxels x 4 bytes: 1.9 GB for a 6-class model at 300 x 512^2); `labels_out` / `probs_out` may be
        caller-owned C-contiguous arrays -- page-locked ones (lm_host_alloc, LMInferer's result pool) take the copy at link speed."""
        vol = np.ascontiguousarray(vol)
        self._lm_dtype(vol.dtype)
        dt = np.dtype(dtype)
        if dt not in LM_PROB_DTYPES:
            raise LMError(f"probability maps are float32 or float16, not {dt}")
        n, h, w = vol.shape
        c = self.n_classes(slot)
        if labels_out is None:
            labels_out = np.empty((n, h, w), np.uint8)
        if probs_out is None:
            probs_out = np.empty((c, n, h, w), dt)
        if labels_out.dtype != np.uint8 or labels_out.shape != (n, h, w) or not labels_out.flags.c_contiguous:
            raise LMError("apply_probs(labels_out=...): need a C-contiguous uint8 array of the volume's shape")
        if probs_out.dtype != dt or probs_out.shape != (c, n, h, w) or not probs_out.flags.c_contiguous:
            raise LMError(f"apply_probs(probs_out=...): need a C-contiguous {dt} array of shape {(c, n, h, w)}")
        with self.scope() as dev:
            vd, ld, pd = dev.upload(vol), dev.empty((n, h, w), np.uint8), dev.empty((c, n, h, w), dt)
            self.apply_probs_dev(slot, vd, pd, ld, batch_size=batch_size, volume_postprocessing=volume_postprocessing)
            ld.download_into(labels_out)
            pd.download_into(probs_out)
        return labels_out, probs_out

    # -- orientation
    def reorient_dev(self, src: DeviceArray, axes, flips, out: Optional[DeviceArray] = None) -> DeviceArray:
        """out = src.transpose(axes) with out-axis k reversed where flips[k] (device index transform).  `out`: an existing
        destination of the permuted shape (e.g. a DeviceView into a stack), else a new allocation."""
        in_strides = [int(np.prod(src.shape[a + 1:], dtype=np.int64)) for a in range(3)]
        shape, strides, base = [], [], 0
        for k in range(3):
            a = int(axes[k])
            shape.append(src.shape[a])
            if flips[k]:
                strides.append(-in_strides[a])
                base += (src.shape[a] - 1) * in_strides[a]
            else:
                strides.append(in_strides[a])
        if out is None:
            out = self.empty(tuple(shape), src.dtype)
        elif tuple(out.shape) != tuple(shape) or out.dtype != src.dtype:
            raise LMError(f"reorient_dev(out=...): need {tuple(shape)} {src.dtype}, got {out.shape} {out.dtype}")
        self.L.check(self.L.lib.lm_reorient_dev(self.h, src.ptr, out.ptr, np.dtype(src.dtype).itemsize, *shape, *strides, base),
                     "lm_reorient_dev")
        return out

    # -- post-processing
    def postprocess_dev(self, lab: DeviceArray, spare: Sequence[int] = (), skip_below: int = 3):
        n, h, w = lab.shape
        sp = (C.c_int * max(len(spare), 1))(*[int(s) for s in spare])
        self.L.check(self.L.lib.lm_postprocess_dev(self.h, lab.ptr, n, h, w, sp, len(spare), int(skip_below)), "lm_postprocess_dev")

    def postprocess(self, lab: np.ndarray, spare: Sequence[int] = (), skip_below: int = 3) -> np.ndarray:
        """== utils.postprocessing(label_image, spare, skip_below=...)."""
        with self.scope() as dev:
            ld = dev.upload(lab, np.uint8)
            self.postprocess_dev(ld, spare, skip_below)
            self.sync()
            return ld.download()

    def bbox_3d(self, mask: np.ndarray, margin: int = 2):
        """== utils.bbox_3D(labelmap, margin) for a [n, h, w] volume (non-zero = set): 6 ints, or None for an empty mask."""
        bb = (C.c_int32 * 6)()
        with self.scope() as dev:
            md = dev.upload(np.asarray(mask) != 0, np.uint8)
            n, h, w = md.shape
            self.L.check(self.L.lib.lm_bbox3d_dev(self.h, md.ptr, n, h, w, int(margin), bb), "lm_bbox3d_dev")
        return None if bb[1] < 0 else [int(v) for v in bb]

    def keep_largest_dev(self, mask: DeviceArray) -> int:
        n, h, w = mask.shape
        area = C.c_int64()
        self.L.check(self.L.lib.lm_keep_largest_dev(self.h, mask.ptr, n, h, w, C.byref(area)), "lm_keep_largest_dev")
        return int(area.value)

    def keep_largest(self, mask: np.ndarray):
        """== utils.keep_largest_connected_component(mask) for a [n, h, w] u8 volume -> (bool volume, area); area 0 = no region."""
        with self.scope() as dev:
            md = dev.upload(mask, np.uint8)
            area = self.keep_largest_dev(md)
            self.sync()
            return md.download().astype(bool), area

    # -- per-label statistics (include/lungmask_hip.h: lm_label_stats_dev)
    def label_stats_dev(self, lab: DeviceArray, vol: DeviceArray, n_labels: int, hist: bool = True) -> dict:
        """lab u8 [n][h][w] and vol [n][h][w] (int16 / int32 / int64 / float32 / float64) on the device -> the raw accumulators as
        numpy arrays over labels 0 .. n_labels-1: voxels, nonfinite, clipped_low, clipped_high, hu_min, hu_max (int64 [n_labels]),
        index_sum (int64 [n_labels][3]), bbox (int32 [n_labels][6]), hist (int64 [n_labels][4096], bin b = HU b - 1024; row 0 zero;
        None with hist=False) and other (voxels with a label >= n_labels).  Returns once the result is on the host."""
        self._check_labels_and_volume("label_stats_dev", lab, vol)
        code = self._lm_dtype(vol.dtype, "label_stats_dev")
        n, h, w = lab.shape
        k = int(n_labels)
        st = (LabelStats * max(k, 1))()
        hs = np.zeros((max(k, 1), STATS_BINS), np.int64) if hist else None
        other = C.c_int64()
        self.L.check(self.L.lib.lm_label_stats_dev(self.h, lab.ptr, vol.ptr, code, n, h, w, k, st,
                                                   hs.ctypes.data if hs is not None else None, C.byref(other)), "lm_label_stats_dev")
        out = {f: np.array([getattr(st[i], f) for i in range(k)], np.int64)
               for f in ("voxels", "nonfinite", "clipped_low", "clipped_high", "hu_min", "hu_max")}
        out["index_sum"] = np.array([list(st[i].index_sum) for i in range(k)], np.int64).reshape(k, 3)
        out["bbox"] = np.array([list(st[i].bbox) for i in range(k)], np.int32).reshape(k, 6)
        out["hist"] = hs
        out["other"] = int(other.value)
        return out

    def label_stats(self, lab: np.ndarray, vol: np.ndarray, n_labels: int, hist: bool = True) -> dict:
        """Host form of label_stats_dev: both volumes are copied to the device first."""
        lab = np.ascontiguousarray(lab, dtype=np.uint8)
        vol = np.ascontiguousarray(vol)
        self._lm_dtype(vol.dtype, "label_stats")
        if lab.ndim != 3 or lab.shape != vol.shape:
            raise LMError(f"label_stats: need two 3-D volumes of the same shape (got {lab.shape}, {vol.shape})")
        with self.scope() as dev:
            return self.label_stats_dev(dev.upload(lab), dev.upload(vol), n_labels, hist=hist)

    # -- per-label texture matrices (include/lungmask_hip.h: lm_texture_dev)
    def texture_dev(self, lab: DeviceArray, vol: DeviceArray, n_labels: int, lo: int = -1000, hi: int = 199, bin_width: int = 25,
                    distance: int = 1, nr: int = 64, glrlm: bool = True) -> dict:
        """lab u8 [n][h][w] and vol [n][h][w] (int16 / int32 / int64 / float32 / float64) on the device -> the raw texture matrices as
        numpy arrays over labels 0 .. n_labels-1: glcm (int64 [n_labels][13][Ng][Ng], ordered pairs), glrlm (int64
        [n_labels][13][Ng][nr], the last column absorbing longer runs; None with glrlm=False), the counts voxels, valid, nonfinite,
        below, above, longest_run (int64 [n_labels]) and levels (Ng).  Row 0 of everything is zero.  Returns once the result is on
        the host."""
        self._check_labels_and_volume("texture_dev", lab, vol)
        code = self._lm_dtype(vol.dtype, "texture_dev")
        n, h, w = lab.shape
        k = int(n_labels)
        vals = [int(v) for v in (lo, hi, bin_width, distance, nr)]
        if any(not -2 ** 31 <= v < 2 ** 31 for v in vals):
            raise LMError(f"texture_dev: lo, hi, bin_width, distance and nr must fit in int32 (got {vals})")
        p = TextureParams(*vals)
        ng = (p.hi - p.lo) // p.bin_width + 1 if p.bin_width > 0 and p.hi >= p.lo else 1
        ng = ng if 1 <= ng <= 64 else 1  # (refused below; the buffers only have to exist)
        cols = p.nr if 1 <= p.nr <= 8192 else 1
        cnt = (TextureCounts * max(k, 1))()
        gc = np.zeros((max(k, 1), len(TEXTURE_DIRECTIONS), ng, ng), np.int64)
        gr = np.zeros((max(k, 1), len(TEXTURE_DIRECTIONS), ng, cols), np.int64) if glrlm else None
        self.L.check(self.L.lib.lm_texture_dev(self.h, lab.ptr, vol.ptr, code, n, h, w, k, C.byref(p), cnt, gc.ctypes.data,
                                               gr.ctypes.data if gr is not None else None), "lm_texture_dev")
        out = {f: np.array([getattr(cnt[i], f) for i in range(k)], np.int64) for f in TEXTURE_COUNT_FIELDS}
        out["glcm"], out["glrlm"], out["levels"] = gc, gr, ng
        return out

    def texture(self, lab: np.ndarray, vol: np.ndarray, n_labels: int, **kw) -> dict:
        """Host form of texture_dev: both volumes are copied to the device first."""
        lab = np.ascontiguousarray(lab, dtype=np.uint8)
        vol = np.ascontiguousarray(vol)
        self._lm_dtype(vol.dtype, "texture")
        if lab.ndim != 3 or lab.shape != vol.shape:
            raise LMError(f"texture: need two 3-D volumes of the same shape (got {lab.shape}, {vol.shape})")
        with self.scope() as dev:
            return self.texture_dev(dev.upload(lab), dev.upload(vol), n_labels, **kw)

    # -- label agreement metrics (include/lungmask_hip.h: lm_edt_dev, lm_label_agreement_dev)
    @staticmethod
    def _spacing3(spacing, who):
        if spacing is None:
            return None
        sp = [float(v) for v in spacing]
        if len(sp) != 3:
            raise LMError(f"{who}: spacing needs three values in the array's axis order (got {spacing!r})")
        return (C.c_double * 3)(*sp)

    def edt_dev(self, feat: DeviceArray, spacing=None, out: Optional[DeviceArray] = None) -> DeviceArray:
        """feat u8 [n][h][w] on the device -> float32 [n][h][w]: the squared distance (spacing in the array's axis order, None =
        voxels) to the nearest voxel with feat != 0, exactly as lm_edt_dev defines it in float32.  `out`: a float32 DeviceArray
        of the same shape to receive it (default: a new one).  Enqueued on the engine's stream."""
        if feat.dtype != np.uint8 or len(feat.shape) != 3:
            raise LMError(f"edt_dev: need a 3-D u8 volume (got {feat.shape} {feat.dtype})")
        n, h, w = feat.shape
        sp = self._spacing3(spacing, "edt_dev")
        if out is not None and (out.dtype != np.float32 or tuple(out.shape) != tuple(feat.shape)):
            raise LMError(f"edt_dev: out must be float32 {feat.shape} (got {out.dtype} {out.shape})")
        if out is None:
            self._check_size("edt_dev", feat.shape)
        with self._out_or_new(out, feat.shape, np.float32) as out:
            self.L.check(self.L.lib.lm_edt_dev(self.h, feat.ptr, n, h, w, sp, out.ptr), "lm_edt_dev")
        return out

    def edt(self, feat: np.ndarray, spacing=None) -> np.ndarray:
        """Host form of edt_dev: numpy [n][h][w] (non-zero = feature) -> float32 squared distances."""
        feat = np.asarray(feat)
        if feat.ndim != 3:
            raise LMError(f"edt: need a 3-D volume (got {feat.shape})")
        with self.scope() as dev:
            out = dev.add(self.edt_dev(dev.upload(feat != 0, np.uint8), spacing))
            self.sync()
            return out.download()

    def label_agreement_dev(self, a: DeviceArray, b: DeviceArray, n_labels: int, spacing=None, percentiles: Sequence[float] = (95,)) -> dict:
        """a, b u8 [n][h][w] on the device -> the raw rows of lm_label_agreement_dev as numpy arrays over rows 0 .. n_labels-1 (row
        0 = every label >= 1 together): voxels_a, voxels_b, intersection, surface_a, surface_b (int64), bbox (int32 [rows][6]),
        max_d2_ab, max_d2_ba (float32), sum_d_ab, sum_d_ba (float64), order_ab, order_ba, order_pooled (float32 [rows][len(
        percentiles)][2]: the order statistics at the floor / ceil rank of each percentile), and other_a, other_b (ints),
        percentiles (the list).  Rows with an empty surface have -1 in the distance fields.  Returns once the result is on the host."""
        if a.dtype != np.uint8 or b.dtype != np.uint8 or len(a.shape) != 3 or tuple(a.shape) != tuple(b.shape):
            raise LMError(f"label_agreement_dev: need two u8 volumes of the same 3-D shape (got {a.shape} {a.dtype}, {b.shape} {b.dtype})")
        qs = [float(q) for q in percentiles]
        if len(qs) > AGREEMENT_MAX_PERCENTILES:
            raise LMError(f"label_agreement_dev: at most {AGREEMENT_MAX_PERCENTILES} percentiles (got {len(qs)})")
        n, h, w = a.shape
        k = int(n_labels)
        rows = (LabelAgreement * max(k, 1))()
        qa = (C.c_double * max(len(qs), 1))(*qs)
        self.L.check(self.L.lib.lm_label_agreement_dev(self.h, a.ptr, b.ptr, n, h, w, k, self._spacing3(spacing, "label_agreement_dev"),
                                                       qa, len(qs), rows), "lm_label_agreement_dev")
        out = {f: np.array([getattr(rows[i], f) for i in range(k)], np.int64)
               for f in ("voxels_a", "voxels_b", "intersection", "surface_a", "surface_b")}
        out["bbox"] = np.array([list(rows[i].bbox) for i in range(k)], np.int32).reshape(k, 6)
        for f in ("max_d2_ab", "max_d2_ba"):
            out[f] = np.array([getattr(rows[i], f) for i in range(k)], np.float32)
        for f in ("sum_d_ab", "sum_d_ba"):
            out[f] = np.array([getattr(rows[i], f) for i in range(k)], np.float64)
        for f in ("order_ab", "order_ba", "order_pooled"):
            out[f] = np.array([np.ctypeslib.as_array(getattr(rows[i], f))[:len(qs)] for i in range(k)], np.float32).reshape(k, len(qs), 2)
        out["other_a"], out["other_b"] = int(rows[0].other_a), int(rows[0].other_b)
        out["percentiles"] = qs
        return out

    def label_agreement(self, a: np.ndarray, b: np.ndarray, n_labels: int, spacing=None, percentiles: Sequence[float] = (95,)) -> dict:
        """Host form of label_agreement_dev: both volumes are copied to the device first."""
        a = np.ascontiguousarray(a, dtype=np.uint8)
        b = np.ascontiguousarray(b, dtype=np.uint8)
        if a.ndim != 3 or a.shape != b.shape:
            raise LMError(f"label_agreement: need two 3-D volumes of the same shape (got {a.shape}, {b.shape})")
        with self.scope() as dev:
            return self.label_agreement_dev(dev.upload(a), dev.upload(b), n_labels, spacing, percentiles)

    # -- lung ROI (include/lungmask_hip.h: lm_roi_plan_dev, lm_roi_dev)
    @staticmethod
    def _keep_table(keep):
        """The 256-entry table of `keep` (an iterable of label values in 1..255; None: every label >= 1)."""
        table = (C.c_uint8 * 256)()
        if keep is None:
            for k in range(1, 256):
                table[k] = 1
            return table
        for k in keep:
            if int(k) != k or not 1 <= int(k) <= 255:
                raise ValueError(f"keep: label values in 1..255, got {k!r}")
            table[int(k)] = 1
        return table

    def roi_plan_dev(self, lab: DeviceArray, keep=None):
        """The box (zmin, zmax, ymin, ymax, xmin, xmax; exclusive maxima, no margin) of the voxels of the device labels whose value is
        in `keep` (None: every label >= 1).  ValueError when there is no such voxel."""
        if lab.dtype != np.uint8 or len(lab.shape) != 3:
            raise LMError(f"roi_plan_dev: need a 3-D u8 label volume (got {lab.shape} {lab.dtype})")
        n, h, w = lab.shape
        bb = (C.c_int32 * 6)()
        rc = self.L.lib.lm_roi_plan_dev(self.h, lab.ptr, n, h, w, self._keep_table(keep), bb)
        self._check_kept(rc, "lm_roi_plan_dev", ValueError, "ROI: the labels hold no voxel of the kept label values", keep)
        return [int(v) for v in bb]

    @staticmethod
    def roi_grid(shape, bbox0, spacing=None, spacing_out=None, margin_mm: float = 5.0):
        """Steps 1 and 2 of lm_roi_dev's definition on the host: the margin-0 box grown by ceil(margin_mm / s_i) voxels (margin_mm
        voxels without a spacing) and clipped to `shape`, step_i = t_i / s_i and N_i = floor((e_i - 1) / step_i) + 1.
        -> (bbox, out_dims, step, spacing_out in array axis order or None)."""
        import math

        if not (margin_mm >= 0 and math.isfinite(margin_mm)):
            raise ValueError(f"margin_mm must be >= 0 and finite, got {margin_mm!r}")
        sp = None if spacing is None else [float(v) for v in spacing]
        if sp is not None and (len(sp) != 3 or not all(v > 0 and math.isfinite(v) for v in sp)):
            raise ValueError(f"spacing needs three positive values in the array's axis order, got {spacing!r}")
        if spacing_out is None:
            t = sp
        else:
            if sp is None:
                raise ValueError("spacing_out needs the source spacing: pass spacing= with a bare numpy array")
            t = [float(spacing_out)] * 3 if np.ndim(spacing_out) == 0 else [float(v) for v in spacing_out]
            if len(t) != 3 or not all(v > 0 and math.isfinite(v) for v in t):
                raise ValueError(f"spacing_out: one positive value or three in the array's axis order, got {spacing_out!r}")
        bbox, dims, step = [], [], []
        for i in range(3):
            m = int(math.ceil(margin_mm / sp[i])) if sp is not None else int(math.ceil(margin_mm))
            lo, hi = max(int(bbox0[2 * i]) - m, 0), min(int(bbox0[2 * i + 1]) + m, int(shape[i]))
            st = 1.0 if spacing_out is None else t[i] / sp[i]
            bbox += [lo, hi]
            step.append(st)
            dims.append(int(math.floor((hi - lo - 1) / st)) + 1)
        return bbox, dims, step, t

    def roi_dev(self, vol: DeviceArray, lab: DeviceArray, spacing=None, spacing_out=None, margin_mm: float = 5.0, keep=None,
                dilate_mm: float = 0.0, mask_outside: bool = True, fill=-1024, window=None, dtype=np.float32, out=None):
        """The lung ROI of the device-resident volume and labels (lm_roi_dev's definition, include/lungmask_hip.h): -> (image
        DeviceArray of `dtype`, labels DeviceArray u8, info) with info = {bbox, out_dims, step, spacing_mm}.  Nothing but the box
        (six ints) crosses to the host.  `out`: a callable (out_dims) -> (image DeviceArray of `dtype`, labels DeviceArray u8), both of
        shape out_dims, that provides the two results (default: new allocations).  Enqueued on the engine's stream."""
        import math

        self._check_labels_and_volume("roi_dev", lab, vol)
        code = self._lm_dtype(vol.dtype, "roi_dev", signed_only=True)
        dt = np.dtype(dtype)
        if dt not in LM_ROI_DTYPES:
            raise TypeError(f"ROI dtype float32, float16 or int16, not {dt}")
        if dt == np.int16 and (vol.dtype.kind == "f" or window is not None):
            raise ValueError("ROI dtype int16 needs an integer volume and no window")
        if not (0.0 <= dilate_mm <= margin_mm):
            raise ValueError(f"0 <= dilate_mm <= margin_mm is required (got dilate_mm {dilate_mm!r}, margin_mm {margin_mm!r})")
        if window is not None:
            lo, hi = (float(v) for v in window)
            if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo):
                raise ValueError(f"window=(lo, hi) needs finite lo < hi, got {window!r}")
        table = self._keep_table(keep)
        n, h, w = lab.shape
        if n == 0:
            raise ValueError("ROI: the labels hold no voxel of the kept label values")
        bbox0 = self.roi_plan_dev(lab, keep)
        bbox, dims, step, t = self.roi_grid(lab.shape, bbox0, spacing, spacing_out, margin_mm)
        p = RoiParams()
        p.bbox[:] = bbox
        p.out_dims[:] = dims
        p.step[:] = step
        C.memmove(p.keep, table, 256)
        p.dilate_mm = float(dilate_mm)
        p.spacing[:] = [1.0, 1.0, 1.0] if spacing is None else [float(v) for v in spacing]
        p.fill = float(fill)
        p.window_lo, p.window_hi = (0.0, 0.0) if window is None else (float(window[0]), float(window[1]))
        p.flags = (ROI_MASK_OUTSIDE if mask_outside else 0) | (ROI_WINDOW if window is not None else 0)
        p.out_dtype = LM_ROI_DTYPES[dt]
        if int(np.prod(dims, dtype=np.int64)) >= 2 ** 31 - 1:
            raise LMError("roi_dev: output too large (N_0 * N_1 * N_2 must stay below 2^31)")
        given = (None, None) if out is None else out(tuple(dims))
        with self._out_or_new(given[0], dims, dt) as img, self._out_or_new(given[1], dims, np.uint8) as out_lab:
            if (img.dtype, out_lab.dtype) != (dt, np.uint8) or tuple(img.shape) != tuple(dims) or tuple(out_lab.shape) != tuple(dims):
                raise LMError(f"roi_dev(out=...): need a {dt} and a uint8 array of shape {tuple(dims)}")
            self.L.check(self.L.lib.lm_roi_dev(self.h, vol.ptr, code, lab.ptr, n, h, w, C.byref(p), img.ptr, out_lab.ptr), "lm_roi_dev")
        return img, out_lab, {"bbox": bbox, "out_dims": dims, "step": step, "spacing_mm": t}

    def roi(self, vol: np.ndarray, lab: np.ndarray, **kw):
        """Host form of roi_dev: both volumes are copied to the device first -> (image, labels, info) as numpy arrays."""
        lab = np.ascontiguousarray(lab, dtype=np.uint8)
        vol = np.ascontiguousarray(vol)
        if lab.ndim != 3 or lab.shape != vol.shape:
            raise LMError(f"roi: need two 3-D volumes of the same shape (got {lab.shape}, {vol.shape})")
        self._lm_dtype(vol.dtype, "roi")
        with self.scope() as dev:
            ld, vd = dev.upload(lab), dev.upload(vol)
            img, out_lab, info = self.roi_dev(vd, ld, **kw)
            dev.add(img, out_lab)
            self.sync()
            return img.download(), out_lab.download(), info

    # -- resampling onto any grid (include/lungmask_hip.h: lm_spline_prefilter_dev, lm_resample_dev)
    def spline_prefilter_dev(self, vol: DeviceArray, out: Optional[DeviceArray] = None) -> DeviceArray:
        """The float64 cubic B-spline coefficients of the device-resident volume (lm_spline_prefilter_dev).  Enqueued on the engine's
        stream."""
        if len(vol.shape) != 3 or vol.shape[0] < 1:
            raise LMError(f"spline_prefilter_dev: need a 3-D volume with at least one slice (got {vol.shape})")
        code = self._lm_dtype(vol.dtype, "spline_prefilter_dev", signed_only=True)
        self._check_size("spline_prefilter_dev", vol.shape)
        n, h, w = vol.shape
        with self._out_or_new(out, vol.shape, np.float64) as coef:
            if coef.dtype != np.float64 or tuple(coef.shape) != tuple(vol.shape):
                raise LMError(f"spline_prefilter_dev(out=...): need a float64 array of shape {tuple(vol.shape)}")
            self.L.check(self.L.lib.lm_spline_prefilter_dev(self.h, vol.ptr, code, n, h, w, coef.ptr), "lm_spline_prefilter_dev")
        return coef

    def _resample_params(self, who: str, src: DeviceArray, A, b, out_shape, mode: str, fill, dtype, coef_source: bool = False,
                         field: Optional[DeviceArray] = None):
        """What resample_dev and warp_dev (`who`: "resample" / "warp") check and fill in alike -> (ResampleParams, the source's dtype
        code, the output dtype, the output extents).  `coef_source`: "cubic" takes the float64 coefficients of spline_prefilter_dev as
        its source; `field`: warp_dev's, checked against the output grid."""
        if mode not in RESAMPLE_MODES:
            raise ValueError(f"mode: one of {sorted(RESAMPLE_MODES)}, got {mode!r}")
        if len(src.shape) != 3 or src.shape[0] < 1:
            raise LMError(f"{who}_dev: need a 3-D source with at least one slice (got {src.shape})")
        code = self._lm_dtype(src.dtype, f"{who}_dev")
        if code == 5:
            raise LMError(f"{who}_dev: unsupported source dtype uint16")
        dims = [int(v) for v in out_shape]
        if len(dims) != 3 or min(dims) < 1:
            raise ValueError(f"out_shape: three extents >= 1, got {out_shape!r}")
        self._check_size(f"{who}_dev", src.shape)
        self._check_size(f"{who}_dev (output)", dims)
        self._check_field(f"{who}_dev", field, dims)  # (resample_dev has no field: nothing is checked)
        coef = coef_source and mode == "cubic"
        if mode in ("nearest", "label_linear"):
            dt = np.dtype(src.dtype if dtype is None else dtype)
            if dt != src.dtype:
                raise ValueError(f"{who} mode {mode!r} returns the source's raw values: dtype must be {src.dtype}, not {dt}")
            if mode == "label_linear" and dt != np.uint8:
                raise ValueError(f"{who} mode 'label_linear' needs uint8 labels")
            out_code = code
        else:
            dt = np.dtype(np.float32 if dtype is None else dtype)
            if src.dtype == np.uint8:
                raise ValueError(f"{who} mode {mode!r} needs an image volume, not uint8 labels")
            if coef and src.dtype != np.float64:
                raise ValueError(f"{who} mode 'cubic' takes the float64 coefficients of spline_prefilter_dev as its source")
            if dt not in LM_ROI_DTYPES:
                raise TypeError(f"{who} dtype float32, float16 or int16, not {dt}")
            if dt == np.int16 and src.dtype.kind == "f" and not coef:
                raise ValueError(f"{who} dtype int16 needs an integer volume")
            out_code = LM_ROI_DTYPES[dt]
        if dt == np.uint8 and not 0 <= float(fill) <= 255:
            raise ValueError(f"fill of uint8 labels must lie in 0..255, got {fill!r}")
        p = ResampleParams()
        p.out_dims[:] = dims
        p.mode = RESAMPLE_MODES[mode]
        _affine_into(p, A, b)
        p.fill = float(fill)
        p.out_dtype = out_code
        return p, code, dt, dims

    def _two_volumes(self, who: str, fixed: DeviceArray, moving: DeviceArray, signed_only: bool = True, sized: bool = False):
        """The dtype codes of the two 3-D volumes of a paired entry point.  `signed_only`: uint8 is refused like uint16; `sized`: at
        least one slice and lm_edt_dev's limits, checked here."""
        codes = []
        for name, arr in (("fixed", fixed), ("moving", moving)):
            if len(arr.shape) != 3 or (sized and arr.shape[0] < 1):
                raise LMError(f"{who}: need a 3-D {name} volume (got {arr.shape})")
            code = self._lm_dtype(arr.dtype, who, signed_only=signed_only)
            if code == 5:  # (joint_hist_dev only: with signed_only _lm_dtype has refused uint16 already)
                raise LMError(f"{who}: unsupported volume dtype uint16")
            codes.append(code)
            if sized:
                self._check_size(f"{who} ({name})", arr.shape)
        return codes

    def resample_dev(self, src: DeviceArray, A, b, out_shape, mode: str = "linear", fill=-1024, dtype=None,
                     out: Optional[DeviceArray] = None) -> DeviceArray:
        """The device-resident volume (or u8 labels) `src` sampled at `A @ o + b` for every index o of an output of `out_shape`
        (lm_resample_dev's definition, include/lungmask_hip.h; `A` 3 x 3 and `b` 3 in float64, array axis order: resample.index_map)
        -> DeviceArray of `dtype`.  `mode`: "nearest" (any dtype; the result has the source's), "linear" or "cubic" (float32 --
        the default --, float16, or int16 for integer volumes), "label_linear" (u8).  Enqueued on the engine's stream."""
        p, code, dt, dims = self._resample_params("resample", src, A, b, out_shape, mode, fill, dtype)
        n, h, w = src.shape
        with self._out_or_new(out, dims, dt) as res:
            if res.dtype != dt or tuple(res.shape) != tuple(dims):
                raise LMError(f"resample_dev(out=...): need a {dt} array of shape {tuple(dims)}")
            self.L.check(self.L.lib.lm_resample_dev(self.h, src.ptr, code, n, h, w, C.byref(p), res.ptr), "lm_resample_dev")
        return res

    def resample(self, src: np.ndarray, A, b, out_shape, mode: str = "linear", fill=-1024, dtype=None) -> np.ndarray:
        """Host form of resample_dev: the source is copied to the device first -> numpy array."""
        src = np.ascontiguousarray(src)
        with self.scope() as dev:
            res = dev.add(self.resample_dev(dev.upload(src), A, b, out_shape, mode, fill, dtype))
            self.sync()
            return res.download()

    def spline_prefilter(self, vol: np.ndarray) -> np.ndarray:
        """Host form of spline_prefilter_dev -> float64 numpy array."""
        with self.scope() as dev:
            coef = dev.add(self.spline_prefilter_dev(dev.upload(np.ascontiguousarray(vol))))
            self.sync()
            return coef.download()

    # -- joint histogram under an affine map (include/lungmask_hip.h: lm_joint_hist_dev)
    def joint_hist_dev(self, fixed: DeviceArray, moving: DeviceArray, A, b, bins: int = 32, fixed_bins=(-1024, 64), moving_bins=(-1024, 64),
                       start=(0, 0, 0), step=(1, 1, 1), mode: str = "linear", labels: Optional[DeviceArray] = None, keep=None,
                       out: Optional[DeviceArray] = None) -> DeviceArray:
        """The joint histogram of the device-resident `fixed` and `moving` volumes, `moving` sampled at `A @ o + b` for the fixed
        indices o = start + k * step (lm_joint_hist_dev's definition, include/lungmask_hip.h) -> DeviceArray int64 [bins * bins + 4]:
        the histogram, row = fixed bin, followed by the four counts (`split_joint_hist`).  `fixed_bins`, `moving_bins`: (lowest HU,
        HU per bin).  `labels`: u8 of the fixed shape, only voxels whose label is in `keep` (None: every label >= 1) are sampled.
        `out`: an int64 DeviceArray of that size to receive the result.  Enqueued on the engine's stream."""
        if mode not in JOINT_HIST_MODES:
            raise ValueError(f"mode: one of {sorted(JOINT_HIST_MODES)}, got {mode!r}")
        codes = self._two_volumes("joint_hist_dev", fixed, moving, signed_only=False)
        if labels is not None:
            self._check_labels_and_volume("joint_hist_dev", labels, fixed)
        p = JointHistParams()
        _affine_into(p, A, b)
        p.start[:] = [int(v) for v in start]
        p.step[:] = [int(v) for v in step]
        p.bins, p.mode = int(bins), JOINT_HIST_MODES[mode]
        (p.f_lo, p.f_width), (p.m_lo, p.m_width) = (int(v) for v in fixed_bins), (int(v) for v in moving_bins)
        C.memmove(p.keep, self._keep_table(keep), 256)
        size = max(int(bins), 0) ** 2 + 4
        with self._out_or_new(out, (size,), np.int64) as res:
            if res.dtype != np.int64 or res.nbytes < size * 8:
                raise LMError(f"joint_hist_dev(out=...): need an int64 array of {size} values")
            self.L.check(self.L.lib.lm_joint_hist_dev(self.h, fixed.ptr, codes[0], *fixed.shape, labels.ptr if labels is not None else None,
                                                      moving.ptr, codes[1], *moving.shape, C.byref(p), res.ptr, res.ptr + (size - 4) * 8),
                         "lm_joint_hist_dev")
        return res

    @staticmethod
    def split_joint_hist(values: np.ndarray, bins: int):
        """(hist int64 [bins][bins], counts dict) of the downloaded result of joint_hist_dev."""
        nb = int(bins) ** 2
        c = values[nb:nb + 4]
        counts = {"sampled": int(c[0]), "contributed": int(c[1]), "outside": int(c[2]), "nan": int(c[3])}
        return values[:nb].reshape(bins, bins).copy(), counts

    def joint_hist(self, fixed: np.ndarray, moving: np.ndarray, A, b, bins: int = 32, labels: Optional[np.ndarray] = None, **kw):
        """Host form of joint_hist_dev: the volumes are copied to the device first -> (hist, counts)."""
        with self.scope() as dev:
            ld = dev.upload(labels, np.uint8) if labels is not None else None
            res = dev.add(self.joint_hist_dev(dev.upload(np.ascontiguousarray(fixed)), dev.upload(np.ascontiguousarray(moving)), A, b, bins,
                                              labels=ld, **kw))
            self.sync()
            return self.split_joint_hist(res.download(), bins)

    # -- deformable registration (include/lungmask_hip.h: lm_warp_dev, lm_demons_step_dev, lm_jacobian_dev)
    @staticmethod
    def field_scale(spacing=None):
        """field_scale of the header: 1 / spacing_i in float64 (array axis order), 1.0 without a spacing -> ctypes double[3]."""
        sp = [1.0, 1.0, 1.0] if spacing is None else [float(v) for v in spacing]
        if len(sp) != 3 or not all(v > 0 and np.isfinite(v) for v in sp):
            raise ValueError(f"spacing: three positive values in the array's axis order, got {spacing!r}")
        return (C.c_double * 3)(*[1.0 / v for v in sp])

    @staticmethod
    def _check_field(who: str, field: Optional[DeviceArray], shape):
        if field is not None and (field.dtype != np.float32 or tuple(field.shape) != (3,) + tuple(int(v) for v in shape)):
            raise LMError(f"{who}: the field must be float32 {(3,) + tuple(shape)} (got {field.dtype} {field.shape})")

    def warp_dev(self, src: DeviceArray, field: Optional[DeviceArray], A, b, out_shape, mode: str = "linear", fill=-1024, dtype=None,
                 spacing=None, out: Optional[DeviceArray] = None) -> DeviceArray:
        """`resample_dev` through a displacement field (lm_warp_dev's definition, include/lungmask_hip.h): `src` sampled at
        `A @ (o + field[:, o] / spacing) + b` for every index o of an output of `out_shape`.  `field`: float32 [3, *out_shape] on the
        output grid, in the units of `spacing` (array axis order; None: voxels), or None for no displacement.  `mode` "cubic" takes
        the float64 coefficients of `spline_prefilter_dev` as `src`.  Everything else is `resample_dev`'s."""
        p, code, dt, dims = self._resample_params("warp", src, A, b, out_shape, mode, fill, dtype, coef_source=True, field=field)
        fs = self.field_scale(spacing)
        n, h, w = src.shape
        with self._out_or_new(out, dims, dt) as res:
            if res.dtype != dt or tuple(res.shape) != tuple(dims):
                raise LMError(f"warp_dev(out=...): need a {dt} array of shape {tuple(dims)}")
            self.L.check(self.L.lib.lm_warp_dev(self.h, src.ptr, code, n, h, w, field.ptr if field is not None else None, C.byref(p), fs,
                                                res.ptr), "lm_warp_dev")
        return res

    def warp(self, src: np.ndarray, field: Optional[np.ndarray], A, b, out_shape, mode: str = "linear", fill=-1024, dtype=None,
             spacing=None) -> np.ndarray:
        """Host form of warp_dev: source and field are copied to the device first, and for "cubic" the source is prefiltered there
        -> numpy array."""
        src = np.ascontiguousarray(src)
        with self.scope() as dev:
            sd = dev.upload(src)
            if mode == "cubic":
                sd = dev.add(self.spline_prefilter_dev(sd))
                if dtype is not None and np.dtype(dtype) == np.int16 and src.dtype.kind == "f":
                    raise ValueError("warp dtype int16 needs an integer volume")
            fd = dev.upload(np.ascontiguousarray(field, dtype=np.float32)) if field is not None else None
            res = dev.add(self.warp_dev(sd, fd, A, b, out_shape, mode, fill, dtype, spacing))
            self.sync()
            return res.download()

    def demons_step_dev(self, fixed: DeviceArray, moving: DeviceArray, u: DeviceArray, out: DeviceArray, counts: DeviceArray, A, b,
                        spacing=None, inv_k2: float = 1.0, den_min: float = 1e-9, labels: Optional[DeviceArray] = None, keep=None):
        """One additive demons iteration (lm_demons_step_dev's definition, include/lungmask_hip.h): the field `u` (float32
        [3, *fixed.shape], in the units of `spacing`) -> `out` (another array of the same kind) and `counts` (int64, at least five
        values: DEMONS_COUNTS).  `moving` is sampled at `A @ (o + u / spacing) + b`; `labels`, `keep`: only the fixed voxels whose
        label is in `keep` (None: every label >= 1) move.  grad_scale is field_scale / 2.  Enqueued on the engine's stream."""
        codes = self._two_volumes("demons_step_dev", fixed, moving)
        if labels is not None:
            self._check_labels_and_volume("demons_step_dev", labels, fixed)
        self._check_field("demons_step_dev", u, fixed.shape)
        self._check_field("demons_step_dev (out)", out, fixed.shape)
        if u is None or out is None or out.ptr == u.ptr:
            raise LMError("demons_step_dev: u and out must be two different field arrays (the step is not in-place)")
        if counts.dtype != np.int64 or counts.nbytes < 40:
            raise LMError("demons_step_dev: counts must be an int64 array of at least five values")
        p = DemonsParams()
        _affine_into(p, A, b)
        fs = self.field_scale(spacing)
        p.field_scale[:] = list(fs)
        p.grad_scale[:] = [v / 2.0 for v in fs]
        p.inv_k2, p.den_min = float(inv_k2), float(den_min)
        C.memmove(p.keep, self._keep_table(keep), 256)
        self.L.check(self.L.lib.lm_demons_step_dev(self.h, fixed.ptr, codes[0], *fixed.shape, labels.ptr if labels is not None else None,
                                                   moving.ptr, codes[1], *moving.shape, u.ptr, C.byref(p), out.ptr, counts.ptr),
                     "lm_demons_step_dev")
        return out

    def jacobian_dev(self, field: DeviceArray, spacing=None, out: Optional[DeviceArray] = None, counts: Optional[DeviceArray] = None):
        """det(I + G) of the displacement field `field` (float32 [3, n, h, w], in the units of `spacing`; lm_jacobian_dev's definition,
        include/lungmask_hip.h) -> DeviceArray float32 [n, h, w].  `counts`: an int64 DeviceArray of at least two values that receives
        the numbers of folded (det <= 0) and NaN voxels.  Enqueued on the engine's stream."""
        if len(field.shape) != 4 or field.shape[0] != 3 or field.dtype != np.float32 or field.shape[1] < 1:
            raise LMError(f"jacobian_dev: the field must be float32 [3, n, h, w] (got {field.dtype} {field.shape})")
        shape = field.shape[1:]
        self._check_size("jacobian_dev", shape)
        if counts is not None and (counts.dtype != np.int64 or counts.nbytes < 16):
            raise LMError("jacobian_dev: counts must be an int64 array of at least two values")
        fs = self.field_scale(spacing)
        with self._out_or_new(out, shape, np.float32) as det:
            if det.dtype != np.float32 or tuple(det.shape) != tuple(shape):
                raise LMError(f"jacobian_dev(out=...): need a float32 array of shape {tuple(shape)}")
            self.L.check(self.L.lib.lm_jacobian_dev(self.h, field.ptr, *shape, fs, det.ptr, counts.ptr if counts is not None else None),
                         "lm_jacobian_dev")
        return det

    def jacobian(self, field: np.ndarray, spacing=None):
        """Host form of jacobian_dev -> (det float32 [n, h, w], folded, nan)."""
        field = np.ascontiguousarray(field, dtype=np.float32)
        with self.scope() as dev:
            counts = dev.empty((2,), np.int64)
            det = dev.add(self.jacobian_dev(dev.upload(field), spacing, counts=counts))
            self.sync()
            c = counts.download()
            return det.download(), int(c[0]), int(c[1])

    # -- local-correlation metric (include/lungmask_hip.h: lm_local_moments_dev, lm_lcc_step_dev)
    def _lcc_pair(self, who: str, f: DeviceArray, m: DeviceArray):
        for name, arr in (("f", f), ("m", m)):
            if arr.dtype != np.float32 or len(arr.shape) != 3 or arr.shape[0] < 1:
                raise LMError(f"{who}: {name} must be a float32 volume [n, h, w] (got {arr.dtype} {arr.shape})")
        if tuple(f.shape) != tuple(m.shape):
            raise LMError(f"{who}: f and m must share one grid (got {f.shape} and {m.shape}): m is the moving volume warped onto f's")
        self._check_size(who, f.shape)

    @staticmethod
    def _lcc_radius(radius):
        given = [radius] * 3 if np.ndim(radius) == 0 else list(radius)
        if len(given) != 3 or any(int(v) != v for v in given):
            raise ValueError(f"radius: one whole number or three in the array's axis order, got {radius!r}")
        r = [int(v) for v in given]
        if any(v < 0 or v > LCC_MAX_RADIUS for v in r):
            raise ValueError(f"radius: every window radius must lie in 0 .. {LCC_MAX_RADIUS} voxels, got {r}")
        return (C.c_int32 * 3)(*r)

    def local_moments_dev(self, f: DeviceArray, m: DeviceArray, radius, out: Optional[DeviceArray] = None) -> DeviceArray:
        """The six window sums of lm_local_moments_dev (include/lungmask_hip.h) of the float32 volumes `f` and `m` (the moving volume
        warped onto f's grid, NaN where it sampled outside) -> DeviceArray float64 [6, n, h, w]: the sums of 1, f, m, f*f, m*m, f*m
        over the valid voxels of the box of `radius` (one value or three, 0 .. 8, array axis order) clipped to the volume.  Enqueued
        on the engine's stream."""
        self._lcc_pair("local_moments_dev", f, m)
        r = self._lcc_radius(radius)
        shape = (6,) + tuple(f.shape)
        with self._out_or_new(out, shape, np.float64) as res:
            if res.dtype != np.float64 or tuple(res.shape) != shape:
                raise LMError(f"local_moments_dev(out=...): need a float64 array of shape {shape}")
            self.L.check(self.L.lib.lm_local_moments_dev(self.h, f.ptr, m.ptr, *f.shape, r, res.ptr), "lm_local_moments_dev")
        return res

    def local_moments(self, f: np.ndarray, m: np.ndarray, radius) -> np.ndarray:
        """Host form of local_moments_dev -> numpy float64 [6, n, h, w]."""
        with self.scope() as dev:
            res = dev.add(self.local_moments_dev(dev.upload(np.ascontiguousarray(f)), dev.upload(np.ascontiguousarray(m)), radius))
            self.sync()
            return res.download()

    def lcc_step_dev(self, f: DeviceArray, m: DeviceArray, moments: DeviceArray, u: DeviceArray, out: DeviceArray, counts: DeviceArray, A, b,
                     moving_shape, spacing=None, inv_k2: float = 1.0, den_min: float = 1e-9, var_eps: float = 25.0, a_max: float = 4.0,
                     labels: Optional[DeviceArray] = None, keep=None):
        """One additive demons iteration on the local-correlation residual (lm_lcc_step_dev's definition, include/lungmask_hip.h): `f`,
        `m` and `moments` as for / from `local_moments_dev`, the field `u` (float32 [3, *f.shape], in the units of `spacing`) -> `out`
        (another array of the same kind) and `counts` (int64, at least six values: LCC_COUNTS).  `A`, `b`, `moving_shape`: the map and
        the extents of the moving volume `m` was warped from -- the outside test only.  `labels`, `keep`: as `demons_step_dev`.
        Enqueued on the engine's stream."""
        self._lcc_pair("lcc_step_dev", f, m)
        if moments.dtype != np.float64 or tuple(moments.shape) != (6,) + tuple(f.shape):
            raise LMError(f"lcc_step_dev: moments must be float64 {(6,) + tuple(f.shape)} (got {moments.dtype} {moments.shape})")
        if labels is not None:
            self._check_labels_and_volume("lcc_step_dev", labels, f)
        self._check_field("lcc_step_dev", u, f.shape)
        self._check_field("lcc_step_dev (out)", out, f.shape)
        if u is None or out is None or out.ptr == u.ptr:
            raise LMError("lcc_step_dev: u and out must be two different field arrays (the step is not in-place)")
        if counts.dtype != np.int64 or counts.nbytes < 48:
            raise LMError("lcc_step_dev: counts must be an int64 array of at least six values")
        dims = [int(v) for v in moving_shape]
        if len(dims) != 3:
            raise ValueError(f"moving_shape: three extents, got {moving_shape!r}")
        p = LccParams()
        _affine_into(p, A, b)
        fs = self.field_scale(spacing)
        p.field_scale[:] = list(fs)
        p.grad_scale[:] = [v / 2.0 for v in fs]
        p.inv_k2, p.den_min, p.var_eps, p.a_max = float(inv_k2), float(den_min), float(var_eps), float(a_max)
        p.moving_dims[:] = dims
        C.memmove(p.keep, self._keep_table(keep), 256)
        self.L.check(self.L.lib.lm_lcc_step_dev(self.h, f.ptr, m.ptr, moments.ptr, labels.ptr if labels is not None else None, *f.shape,
                                                u.ptr, C.byref(p), out.ptr, counts.ptr), "lm_lcc_step_dev")
        return out

    def lcc_step(self, f: np.ndarray, m: np.ndarray, moments: np.ndarray, u: np.ndarray, A, b, moving_shape, labels=None, **kw):
        """Host form of lcc_step_dev -> (out float32 [3, n, h, w], counts: six Python integers)."""
        with self.scope() as dev:
            ud = dev.upload(np.ascontiguousarray(u, dtype=np.float32))
            out, counts = dev.empty(ud.shape, np.float32), dev.empty((6,), np.int64)
            ld = dev.upload(labels, np.uint8) if labels is not None else None
            self.lcc_step_dev(dev.upload(np.ascontiguousarray(f)), dev.upload(np.ascontiguousarray(m)),
                              dev.upload(np.ascontiguousarray(moments)), ud, out, counts, A, b, moving_shape, labels=ld, **kw)
            self.sync()
            return out.download(), [int(v) for v in counts.download()[:6]]

    # -- fields as operands (include/lungmask_hip.h: lm_field_combine_dev)
    def field_combine_dev(self, src: DeviceArray, out_shape, A, b, R=None, add: Optional[DeviceArray] = None,
                          coord: Optional[DeviceArray] = None, ref: Optional[DeviceArray] = None, alpha: float = 1.0, beta: float = 1.0,
                          spacing=None, out: Optional[DeviceArray] = None, counts: Optional[DeviceArray] = None) -> DeviceArray:
        """`alpha * add + beta * R @ src(A @ (o + coord[:, o] / spacing) + b)` for every index o of an output grid of `out_shape`
        (lm_field_combine_dev's definition, include/lungmask_hip.h) -> DeviceArray float32 [3, *out_shape].  `src`: float32
        [3, n, h, w], sampled trilinearly and extended by its edge values; `add`, `coord`, `ref`: float32 [3, *out_shape] or None
        (no term, no displacement, zeros), and they may be one another or `src`; `R`: 3 x 3 on the sampled vector (None: the
        identity); `spacing`: the OUTPUT grid's, in array axis order, the unit of `coord` (None: voxels).  `counts`: an int64
        DeviceArray of at least four values that receives FIELD_COUNTS -- the voxels sampled outside `src`, those whose difference
        from `ref` is a NaN, and the sum and the maximum of the squared length of that difference in units of 2^-22.  `out` must be
        none of the inputs.  Enqueued on the engine's stream."""
        if len(src.shape) != 4 or src.shape[0] != 3 or src.dtype != np.float32 or src.shape[1] < 1:
            raise LMError(f"field_combine_dev: the source must be a float32 field [3, n, h, w] (got {src.dtype} {src.shape})")
        dims = [int(v) for v in out_shape]
        if len(dims) != 3 or min(dims) < 1:
            raise ValueError(f"out_shape: three extents >= 1, got {out_shape!r}")
        self._check_size("field_combine_dev", src.shape[1:])
        self._check_size("field_combine_dev (output)", dims)
        for name, arr in (("add", add), ("coord", coord), ("ref", ref)):
            self._check_field(f"field_combine_dev ({name})", arr, dims)
        if counts is not None and (counts.dtype != np.int64 or counts.nbytes < 32):
            raise LMError("field_combine_dev: counts must be an int64 array of at least four values")
        p = FieldCombineParams()
        p.out_dims[:] = dims
        _affine_into(p, A, b)
        p.R[:] = _mat9(np.eye(3) if R is None else R)
        p.field_scale[:] = list(self.field_scale(spacing))
        p.alpha, p.beta = float(alpha), float(beta)
        with self._out_or_new(out, [3] + dims, np.float32) as res:
            self._check_field("field_combine_dev(out=...)", res, dims)
            if any(a is not None and a.ptr == res.ptr for a in (src, add, coord, ref)):
                raise LMError("field_combine_dev: out must not be one of the inputs (the call is not in-place)")
            self.L.check(self.L.lib.lm_field_combine_dev(self.h, _ptr(add), _ptr(coord), src.ptr, *src.shape[1:], _ptr(ref), C.byref(p), res.ptr,
                                                         _ptr(counts)), "lm_field_combine_dev")
        return res

    def field_combine(self, src: np.ndarray, out_shape, A, b, R=None, add=None, coord=None, ref=None, alpha: float = 1.0, beta: float = 1.0,
                      spacing=None):
        """Host form of field_combine_dev -> (array float32 [3, *out_shape], counts: a dict of FIELD_COUNTS).  Arguments that are the
        same numpy object are uploaded once and alias on the device."""
        with self.scope() as dev:
            seen = {}

            def up(a):
                if a is None:
                    return None
                if id(a) not in seen:
                    seen[id(a)] = dev.upload(np.ascontiguousarray(a, dtype=np.float32))
                return seen[id(a)]

            counts = dev.empty((4,), np.int64)
            res = dev.add(self.field_combine_dev(up(src), out_shape, A, b, R, up(add), up(coord), up(ref), alpha, beta, spacing, counts=counts))
            self.sync()
            return res.download(), dict(zip(FIELD_COUNTS, (int(v) for v in counts.download()[:4])))

    # -- paired-CT analysis (include/lungmask_hip.h: lm_pair_map_dev)
    def pair_map_dev(self, fixed: DeviceArray, labels: DeviceArray, moving: DeviceArray, field: Optional[DeviceArray], A, b, table: DeviceArray,
                     n_labels: int, spacing=None, jac_scale: float = 1.0, air: float = -1000.0, fixed_thr: float = -950.0,
                     moving_thr: float = -856.0, lo: float = -1000.0, hi: float = -500.0, keep=None, classes: Optional[DeviceArray] = None,
                     change: Optional[DeviceArray] = None, jacobian: Optional[DeviceArray] = None) -> DeviceArray:
        """The paired analysis of `fixed` and `moving` (lm_pair_map_dev's definition, include/lungmask_hip.h): per fixed voxel o with a
        kept label below `n_labels`, f = fixed[o], m = `moving` sampled trilinearly at `A @ (o + field[:, o] / spacing) + b`,
        J = jac_scale * det(I + grad field), the mass-corrected change J (m - air) + air - f and the class
        1 + (f < fixed_thr) + 2 * (m < moving_thr) where both values lie in [lo, hi] -> `table` (int64, at least n_labels x
        LM_PAIR_COLS values: PAIR_COLS per label, zeroed by the call).  `field`: float32 [3, *fixed.shape] in the units of `spacing`
        (array axis order; None: voxels), or None.  `keep`: the label values analysed (None: every label >= 1).  `classes` (uint8),
        `change`, `jacobian` (float32), each of fixed's shape or None: the maps, fully written.  Enqueued on the engine's stream."""
        codes = self._two_volumes("pair_map_dev", fixed, moving, sized=True)
        self._check_labels_and_volume("pair_map_dev", labels, fixed)
        self._check_field("pair_map_dev", field, fixed.shape)
        if int(n_labels) != n_labels or not 1 <= int(n_labels) <= 16:
            raise ValueError(f"n_labels must lie in 1..16, got {n_labels!r}")
        if table.dtype != np.int64 or table.nbytes < 8 * LM_PAIR_COLS * int(n_labels):
            raise LMError(f"pair_map_dev: table must be an int64 array of at least {int(n_labels)} x {LM_PAIR_COLS} values")
        for name, arr, dt in (("classes", classes, np.uint8), ("change", change, np.float32), ("jacobian", jacobian, np.float32)):
            if arr is not None and (arr.dtype != dt or tuple(arr.shape) != tuple(fixed.shape)):
                raise LMError(f"pair_map_dev({name}=...): need a {np.dtype(dt)} array of shape {tuple(fixed.shape)}")
        p = PairParams()
        _affine_into(p, A, b)
        p.field_scale[:] = list(self.field_scale(spacing))
        p.jac_scale, p.air = float(jac_scale), float(air)
        p.fixed_thr, p.moving_thr, p.lo, p.hi = float(fixed_thr), float(moving_thr), float(lo), float(hi)
        p.n_labels = int(n_labels)
        for k in (range(1, 256) if keep is None else keep):  # (label 0 may be analysed too: the table has a row for it)
            if int(k) != k or not 0 <= int(k) <= 255:
                raise ValueError(f"keep: label values in 0..255, got {k!r}")
            p.keep[int(k)] = 1
        self.L.check(self.L.lib.lm_pair_map_dev(self.h, fixed.ptr, codes[0], *fixed.shape, labels.ptr, moving.ptr, codes[1], *moving.shape,
                                                _ptr(field), C.byref(p), _ptr(classes), _ptr(change), _ptr(jacobian), table.ptr), "lm_pair_map_dev")
        return table

    def pair_map(self, fixed: np.ndarray, labels: np.ndarray, moving: np.ndarray, field: Optional[np.ndarray], A, b, n_labels: int,
                 maps=("classes", "change", "jacobian"), **kw):
        """Host form of pair_map_dev -> (table int64 [n_labels, LM_PAIR_COLS], {name: array} for the `maps` asked for).  `kw`:
        pair_map_dev's spacing, jac_scale, air, thresholds, lo, hi and keep."""
        unknown = set(maps) - {"classes", "change", "jacobian"}
        if unknown:
            raise ValueError(f"maps: any of 'classes', 'change', 'jacobian', got {sorted(unknown)}")
        fixed = np.ascontiguousarray(fixed)
        with self.scope() as dev:
            fd = dev.upload(fixed)
            ud = dev.upload(np.ascontiguousarray(field, dtype=np.float32)) if field is not None else None
            table = dev.empty((int(n_labels), LM_PAIR_COLS), np.int64)
            out = {name: dev.empty(fixed.shape, np.uint8 if name == "classes" else np.float32) for name in maps}
            self.pair_map_dev(fd, dev.upload(labels, np.uint8), dev.upload(np.ascontiguousarray(moving)), ud, A, b, table, n_labels,
                              classes=out.get("classes"), change=out.get("change"), jacobian=out.get("jacobian"), **kw)
            self.sync()
            return table.download(), {name: arr.download() for name, arr in out.items()}

    # -- label morphology (include/lungmask_hip.h: lm_nearest_label_dev, lm_morph_dev)
    @staticmethod
    def _into_table(into):
        """The 256-entry table of `into` (an iterable of label values in 0..255 that a grown voxel may overwrite)."""
        table = (C.c_uint8 * 256)()
        for k in into:
            if int(k) != k or not 0 <= int(k) <= 255:
                raise ValueError(f"into: label values in 0..255, got {k!r}")
            table[int(k)] = 1
        return table

    def nearest_label_dev(self, lab: DeviceArray, spacing=None, keep=None, return_distance: bool = False,
                          out: Optional[DeviceArray] = None, d2_out: Optional[DeviceArray] = None):
        """lab u8 [n][h][w] on the device -> the u8 DeviceArray of lm_nearest_label_dev: per voxel the label of the nearest voxel whose
        value is in `keep` (None: every label >= 1), ties by the header's rule; 0 everywhere without such a voxel.  With
        `return_distance` -> (near, d2): the float32 squared distances as well (lm_edt_dev's, bit for bit).  `out` / `d2_out`: a u8 / float32
        DeviceArray of the labels' shape to receive them (default: new ones).  Enqueued on the engine's stream."""
        if lab.dtype != np.uint8 or len(lab.shape) != 3:
            raise LMError(f"nearest_label_dev: need a 3-D u8 label volume (got {lab.shape} {lab.dtype})")
        n, h, w = lab.shape
        table = self._keep_table(keep)
        sp = self._spacing3(spacing, "nearest_label_dev")
        self._check_size("nearest_label_dev", lab.shape)
        for o, dt in ((out, np.uint8), (d2_out, np.float32)):
            if o is not None and (o.dtype != dt or tuple(o.shape) != tuple(lab.shape)):
                raise LMError(f"nearest_label_dev: out / d2_out must be uint8 / float32 {lab.shape} (got {o.dtype} {o.shape})")
        want_d2 = return_distance or d2_out is not None
        with self._out_or_new(out, lab.shape, np.uint8) as near, \
                (self._out_or_new(d2_out, lab.shape, np.float32) if want_d2 else contextlib.nullcontext()) as d2:
            self.L.check(self.L.lib.lm_nearest_label_dev(self.h, lab.ptr, n, h, w, table, sp, d2.ptr if d2 is not None else None,
                                                         near.ptr), "lm_nearest_label_dev")
        return (near, d2) if return_distance or d2_out is not None else near

    def nearest_label(self, lab: np.ndarray, spacing=None, keep=None, return_distance: bool = False):
        """Host form of nearest_label_dev: the labels are copied to the device first -> numpy array(s)."""
        lab = np.ascontiguousarray(lab, dtype=np.uint8)
        if lab.ndim != 3:
            raise LMError(f"nearest_label: need a 3-D label volume (got {lab.shape})")
        with self.scope() as dev:
            res = self.nearest_label_dev(dev.upload(lab), spacing, keep, return_distance)
            near, d2 = dev.add(*res) if return_distance else (dev.add(res), None)
            self.sync()
            return (near.download(), d2.download()) if return_distance else near.download()

    def morph_dev(self, lab: DeviceArray, op: str, radius_mm: float, spacing=None, keep=None, into=(0,),
                  out: Optional[DeviceArray] = None):
        """lm_morph_dev on device-resident labels: `op` "dilate", "erode", "open" or "close" of the voxels whose label is in `keep`
        (None: every label >= 1) by a ball of `radius_mm` (voxels without a spacing; +inf for "dilate" only) -> (out DeviceArray u8,
        (added, removed)).  `into`: the label values a grown voxel may overwrite.  `out`: a u8 DeviceArray of the same shape to
        receive the result (may be `lab`; default: a new one).  NoKeptVoxel (a ValueError) when no voxel is selected.  Returns once the two counts
        are on the host."""
        import math

        if op not in MORPH_OPS:
            raise ValueError(f"op: one of {sorted(MORPH_OPS)}, got {op!r}")
        if lab.dtype != np.uint8 or len(lab.shape) != 3:
            raise LMError(f"morph_dev: need a 3-D u8 label volume (got {lab.shape} {lab.dtype})")
        r = float(radius_mm)
        if not r >= 0 or (math.isinf(r) and op != "dilate"):
            raise ValueError(f"radius_mm must be >= 0 and finite (+inf for a dilation only), got {radius_mm!r}")
        if out is not None and (out.dtype != np.uint8 or tuple(out.shape) != tuple(lab.shape)):
            raise LMError(f"morph_dev: out must be uint8 {lab.shape} (got {out.dtype} {out.shape})")
        p = MorphParams()
        p.op = MORPH_OPS[op]
        p.radius_mm = r
        sp = [1.0, 1.0, 1.0] if spacing is None else [float(v) for v in spacing]
        if len(sp) != 3:
            raise LMError(f"morph_dev: spacing needs three values in the array's axis order (got {spacing!r})")
        p.spacing[:] = sp
        C.memmove(p.keep, self._keep_table(keep), 256)
        C.memmove(p.into, self._into_table(into), 256)
        n, h, w = lab.shape
        if n == 0:
            raise NoKeptVoxel("morphology: the labels hold no voxel of the kept label values")
        self._check_size("morph_dev", lab.shape)
        changed = (C.c_int64 * 2)()
        with self._out_or_new(out, lab.shape, np.uint8) as out:
            rc = self.L.lib.lm_morph_dev(self.h, lab.ptr, n, h, w, C.byref(p), out.ptr, changed)
            self._check_kept(rc, "lm_morph_dev", NoKeptVoxel, "morphology: the labels hold no voxel of the kept label values", keep)
        return out, (int(changed[0]), int(changed[1]))

    def morph(self, lab: np.ndarray, op: str, radius_mm: float, **kw):
        """Host form of morph_dev: the labels are copied to the device first -> (labels as a numpy array, (added, removed))."""
        lab = np.ascontiguousarray(lab, dtype=np.uint8)
        if lab.ndim != 3:
            raise LMError(f"morph: need a 3-D label volume (got {lab.shape})")
        with self.scope() as dev:
            ld = dev.upload(lab)
            _, changed = self.morph_dev(ld, op, radius_mm, out=ld, **kw)
            self.sync()
            return ld.download(), changed

    # -- connected components (include/lungmask_hip.h: lm_components_dev, lm_component_table_dev, lm_relabel_dev)
    @staticmethod
    def _components_params(hu_range, keep, per_label, connectivity, has_image):
        if connectivity not in (6, 26):
            raise ValueError(f"connectivity: 6 or 26, got {connectivity!r}")
        p = ComponentsParams()
        # label 0 may be kept when the key is not the label (the header's rule): the components of what lies OUTSIDE the labels
        zero = keep is not None and not per_label and any(np.ndim(k) == 0 and k == 0 for k in keep)
        table = Engine._keep_table([k for k in keep if not (np.ndim(k) == 0 and k == 0)] if zero else keep)
        table[0] = 1 if zero else 0
        C.memmove(p.keep, table, 256)
        lo, hi = (None, None) if hu_range is None else hu_range
        if (lo is not None or hi is not None) and not has_image:
            raise ValueError("hu_range needs an image")
        for name, v in (("lo", lo), ("hi", hi)):
            if v is None:
                continue
            if int(v) != v or not -2 ** 31 <= int(v) < 2 ** 31:
                raise ValueError(f"hu_range: integer HU bounds in the int32 range or None, got {hu_range!r}")
            setattr(p, name, int(v))
            setattr(p, "has_" + name, 1)
        if lo is not None and hi is not None and lo > hi:
            raise ValueError(f"hu_range: lo <= hi, got {hu_range!r}")
        p.per_label = int(bool(per_label))
        p.connectivity = int(connectivity)
        return p

    def _components_check(self, who, lab, vol, ids=None):
        if lab.dtype != np.uint8 or len(lab.shape) != 3:
            raise LMError(f"{who}: need a 3-D u8 label volume (got {lab.shape} {lab.dtype})")
        code = 0
        if vol is not None:
            text = (f"{who}: the image must have the labels' shape {lab.shape} and dtype int16 / int32 / int64 / float32 / float64 "
                    f"(got {vol.shape} {vol.dtype})")
            if tuple(vol.shape) != tuple(lab.shape):
                raise LMError(text)
            code = self._lm_dtype(vol.dtype, signed_only=True, text=text)
        if ids is not None and (ids.dtype != np.int32 or tuple(ids.shape) != tuple(lab.shape)):
            raise LMError(f"{who}: ids must be int32 {lab.shape} (got {ids.dtype} {ids.shape})")
        self._check_size(who, lab.shape)
        return (*lab.shape, code)

    def components_dev(self, lab: DeviceArray, vol: Optional[DeviceArray] = None, hu_range=None, keep=None, per_label: bool = True,
                       connectivity: int = 6, out: Optional[DeviceArray] = None):
        """lm_components_dev on device-resident labels (u8) and, optionally, image: the connected components of the voxels whose label
        is in `keep` (None: every label >= 1) and whose HU value lies in `hu_range` = (lo, hi), inclusive, either None for open ->
        (ids DeviceArray int32, count, counts int64 [3][256]: voxels / nonfinite / selected per label).  Components are numbered 1 ..
        count by their first voxel in raster order.  `out`: an int32 DeviceArray of the labels' shape to receive the ids."""
        n, h, w, code = self._components_check("components_dev", lab, vol, out)
        p = self._components_params(hu_range, keep, per_label, connectivity, vol is not None)
        total = C.c_int64()
        counts = np.zeros((3, 256), np.int64)
        with self._out_or_new(out, lab.shape, np.int32) as out:
            self.L.check(self.L.lib.lm_components_dev(self.h, lab.ptr, vol.ptr if vol is not None else None, code, n, h, w, C.byref(p),
                                                      out.ptr, C.byref(total), counts.ctypes.data), "lm_components_dev")
        return out, int(total.value), counts

    def component_table_dev(self, ids: DeviceArray, lab: DeviceArray, vol: Optional[DeviceArray] = None, cap: Optional[int] = None):
        """lm_component_table_dev -> (rows, total): `rows` a numpy record array (COMPONENT_DTYPE) of min(total, cap) rows, row i - 1 for
        id i; `total` the largest id present.  cap None: every component (one more pass when there are more than 65536)."""
        n, h, w, code = self._components_check("component_table_dev", lab, vol, ids)
        total = C.c_int64()

        def run(c):
            rows = np.zeros(max(c, 1), COMPONENT_DTYPE)
            self.L.check(self.L.lib.lm_component_table_dev(self.h, ids.ptr, lab.ptr, vol.ptr if vol is not None else None, code, n, h, w,
                                                           rows.ctypes.data, c, C.byref(total)), "lm_component_table_dev")
            return rows[:min(int(total.value), c)]

        if cap is not None:
            if int(cap) != cap or not 0 <= cap < 2 ** 31 - 1:
                raise ValueError(f"cap: an integer in 0 .. 2^31 - 2, got {cap!r}")
            return run(int(cap)), int(total.value)
        rows = run(65536)
        if total.value > 65536:
            rows = run(int(total.value))
        return rows, int(total.value)

    def component_table_launch(self, nvox: int):
        """(workgroups, voxels per workgroup) of the table kernel for a volume of nvox voxels."""
        g, per = C.c_int64(), C.c_int64()
        self.L.check(self.L.lib.lm_component_table_launch(int(nvox), C.byref(g), C.byref(per)), "lm_component_table_launch")
        return int(g.value), int(per.value)

    def relabel_dev(self, ids: DeviceArray, lut, out: Optional[DeviceArray] = None):
        """out[v] = lut[ids[v]] (lm_relabel_dev).  `lut`: an int32 DeviceArray or array-like; `out`: an int32 DeviceArray of ids' shape
        (may be `ids`; default: a new one).  LMError when an id lies outside the table."""
        if ids.dtype != np.int32:
            raise LMError(f"relabel_dev: ids must be int32 (got {ids.dtype})")
        if out is not None and (out.dtype != np.int32 or tuple(out.shape) != tuple(ids.shape)):
            raise LMError(f"relabel_dev: out must be int32 {ids.shape} (got {out.dtype} {out.shape})")
        with self.scope() as dev:
            ld = lut if isinstance(lut, DeviceArray) else dev.upload(np.ascontiguousarray(lut, dtype=np.int32).reshape(-1))
            if ld.dtype != np.int32:
                raise LMError(f"relabel_dev: lut must be int32 (got {ld.dtype})")
            with self._out_or_new(out, ids.shape, np.int32) as out:
                self.L.check(self.L.lib.lm_relabel_dev(self.h, ids.ptr, ld.ptr, int(np.prod(ld.shape, dtype=np.int64)),
                                                       int(np.prod(ids.shape, dtype=np.int64)), out.ptr), "lm_relabel_dev")
        return out

    def components(self, lab: np.ndarray, vol: Optional[np.ndarray] = None, hu_range=None, keep=None, per_label: bool = True,
                   connectivity: int = 6, table: bool = True, cap: Optional[int] = None):
        """Host form of components_dev + component_table_dev: the volumes are copied to the device first -> (ids int32, count, counts,
        rows); rows is None with table=False."""
        lab = np.ascontiguousarray(lab, dtype=np.uint8)
        if lab.ndim != 3:
            raise LMError(f"components: need a 3-D label volume (got {lab.shape})")
        if vol is not None:
            vol = np.ascontiguousarray(vol)
            if vol.shape != lab.shape:
                raise LMError(f"components: need two volumes of the same shape (got {lab.shape}, {vol.shape})")
        with self.scope() as dev:
            ld = dev.upload(lab)
            vd = dev.upload(vol) if vol is not None else None
            ids, total, counts = self.components_dev(ld, vd, hu_range, keep, per_label, connectivity)
            dev.add(ids)
            rows = self.component_table_dev(ids, ld, vd, cap=total if cap is None else cap)[0] if table else None
            return ids.download(), total, counts, rows

    # -- image filters (include/lungmask_hip.h: lm_filter_dev)
    @staticmethod
    def _filter_params(kind, size=3, taps=None, masked=False, keep=None, fill=None, indicator=None) -> FilterParams:
        """lm_filter_params of kind "median" (`size`: one window size or three, each 1, 3 or 5) or "separable" (`taps`: three float32
        arrays of odd length <= 65 in array axis order, None for the identity).  `indicator` = (lo, hi), either None for open."""
        p = FilterParams()
        if kind == "median":
            p.kind = FILTER_MEDIAN
            sz = [size] * 3 if np.ndim(size) == 0 else list(size)
            if len(sz) != 3 or any(int(v) != v or int(v) not in (1, 3, 5) for v in sz):
                raise ValueError(f"size: 1, 3 or 5, one value or one per axis, got {size!r}")
            p.size[:] = [int(v) for v in sz]
            if indicator is not None:
                raise ValueError("indicator belongs to the separable filter")
        elif kind == "separable":
            p.kind = FILTER_SEPARABLE
            if taps is None or len(taps) != 3:
                raise ValueError("taps: three arrays in array axis order (None: the identity)")
            for i, t in enumerate(taps):
                t = np.ones(1, np.float32) if t is None else np.ascontiguousarray(t, dtype=np.float32).reshape(-1)
                if t.size % 2 != 1 or t.size > 2 * FILTER_MAX_RADIUS + 1:
                    raise ValueError(f"taps[{i}]: an odd number of taps, radius at most {FILTER_MAX_RADIUS} (got {t.size} taps)")
                if masked and not (np.all(t >= 0) and t[t.size // 2] > 0):
                    raise ValueError(f"taps[{i}]: the masked form needs taps >= 0 and a centre tap > 0")
                p.radius[i] = t.size // 2
                C.memmove(p.taps[i], t.ctypes.data, t.nbytes)
        else:
            raise ValueError(f"kind: 'median' or 'separable', got {kind!r}")
        C.memmove(p.keep, Engine._keep_table(keep), 256)
        p.flags = FILTER_MASKED if masked else 0
        if fill is not None:
            if not masked:
                raise ValueError("fill needs labels: without them every voxel is filtered")
            p.flags |= FILTER_FILL_OUTSIDE
            p.fill = float(fill)
        if indicator is not None:
            lo, hi = indicator
            for v in (lo, hi):
                if v is not None and (int(v) != v or not -2 ** 31 <= int(v) < 2 ** 31):
                    raise ValueError(f"indicator: integer HU bounds in the int32 range or None, got {indicator!r}")
            p.flags |= FILTER_INDICATOR
            p.ind_lo = -2 ** 31 if lo is None else int(lo)
            p.ind_hi = 2 ** 31 - 1 if hi is None else int(hi)
        return p

    def filter_dev(self, vol: DeviceArray, lab: Optional[DeviceArray] = None, kind: str = "median", size=3, taps=None, keep=None,
                   fill=None, indicator=None, out: Optional[DeviceArray] = None) -> DeviceArray:
        """lm_filter_dev on a device-resident volume: the median of a `size` window (int16, int32 or float32 -> the same dtype) or the
        separable convolution with `taps` (int16, int32, int64, float32 or float64 -> float32), over the whole volume (`lab` None:
        indices clamped) or confined to the voxels of the u8 labels `lab` whose value is in `keep` (None: every label >= 1); the
        other voxels keep their value or take `fill`.  `indicator` = (lo, hi): the separable filter sees 1 where lo <= hu <= hi and 0
        elsewhere.  `out`: a DeviceArray of the result's dtype and the volume's shape (not `vol`; default: a new one).  NoKeptVoxel
        (a ValueError) when labels are given and none is selected.  Enqueued on the engine's stream."""
        masked = lab is not None
        p = self._filter_params(kind, size, taps, masked, keep, fill, indicator)
        text = f"filter_dev: need a 3-D volume of dtype int16 / int32 / int64 / float32 / float64 (got {vol.shape} {vol.dtype})"
        if len(vol.shape) != 3:
            raise LMError(text)
        code = self._lm_dtype(vol.dtype, signed_only=True, text=text)
        if kind == "median" and vol.dtype not in (np.int16, np.int32, np.float32):
            raise ValueError(f"median: dtype int16, int32 or float32, not {vol.dtype} (cast the volume first)")
        if masked and (lab.dtype != np.uint8 or tuple(lab.shape) != tuple(vol.shape)):
            raise LMError(f"filter_dev: the labels must be uint8 {vol.shape} (got {lab.dtype} {lab.shape})")
        n, h, w = vol.shape
        self._check_size("filter_dev", vol.shape)
        dt = vol.dtype if kind == "median" else np.dtype(np.float32)
        if out is not None and (out is vol or out.dtype != dt or tuple(out.shape) != tuple(vol.shape)):
            raise LMError(f"filter_dev: out must be another {dt} array of shape {vol.shape} (got {out.dtype} {out.shape})")
        if masked and n == 0:
            raise NoKeptVoxel("filter: the labels hold no voxel of the kept label values")
        with self._out_or_new(out, vol.shape, dt) as out:
            rc = self.L.lib.lm_filter_dev(self.h, vol.ptr, code, lab.ptr if masked else None, n, h, w, C.byref(p), out.ptr)
            self._check_kept(rc, "lm_filter_dev", NoKeptVoxel, "filter: the labels hold no voxel of the kept label values", keep)
        return out

    def filter(self, vol: np.ndarray, lab: Optional[np.ndarray] = None, **kw) -> np.ndarray:
        """Host form of filter_dev: the volume (and the labels) are copied to the device first -> the result as a numpy array."""
        vol = np.ascontiguousarray(vol)
        if vol.ndim != 3 or (lab is not None and tuple(np.shape(lab)) != vol.shape):
            raise LMError(f"filter: need a 3-D volume and labels of the same shape (got {vol.shape}, {None if lab is None else np.shape(lab)})")
        self._lm_dtype(vol.dtype, "filter")
        with self.scope() as dev:
            vd = dev.upload(vol)
            ld = dev.upload(lab, np.uint8) if lab is not None else None
            out = dev.add(self.filter_dev(vd, ld, **kw))
            self.sync()
            return out.download()

    # -- Hessian and vesselness (include/lungmask_hip.h: lm_hessian_dev, lm_vesselness_dev, lm_vessel_counts_dev)
    @staticmethod
    def _vessel_params(sigmas_vox, truncate=4.0, masked=False, keep=None, alpha=0.5, beta=0.5, c=100.0, bright=True) -> VesselParams:
        """lm_vessel_params of the scales `sigmas_vox`: per scale three sigmas in voxels, in array axis order.  The taps are
        `filters.gaussian_taps(sigma, order, truncate)` for the orders 0, 1, 2; nrm_ab = float32(sigma_a * sigma_b)."""
        import math

        from .filters import gaussian_taps

        scales = [list(s) for s in sigmas_vox]
        if not 1 <= len(scales) <= VESSEL_MAX_SCALES:
            raise ValueError(f"between 1 and {VESSEL_MAX_SCALES} scales are needed, got {len(scales)}")
        for name, v in (("alpha", alpha), ("beta", beta), ("c", c)):
            if not (float(v) > 0 and math.isfinite(float(v))):
                raise ValueError(f"{name} must be > 0 and finite, got {v!r}")
        p = VesselParams()
        C.memmove(p.keep, Engine._keep_table(keep), 256)
        p.flags = (VESSEL_MASKED if masked else 0) | (0 if bright else VESSEL_DARK)
        p.ka, p.kb, p.kc = (float(np.float32(1.0 / (2.0 * float(v) * float(v)))) for v in (alpha, beta, c))
        p.n_scales = len(scales)
        for k, sig in enumerate(scales):
            if len(sig) != 3 or not all(float(v) > 0 and math.isfinite(float(v)) for v in sig):
                raise ValueError(f"a scale needs three sigmas > 0 in voxels of the array's axes, got {sig!r}")
            sz, sy, sx = (float(v) for v in sig)
            for i, sv in enumerate((sz, sy, sx)):
                for o in range(3):
                    t = gaussian_taps(sv, o, truncate)
                    p.scales[k].radius[i] = t.size // 2
                    C.memmove(p.scales[k].taps[i][o], t.ctypes.data, t.nbytes)
            p.scales[k].nrm[:] = [float(np.float32(a * b)) for a, b in ((sx, sx), (sy, sy), (sz, sz), (sx, sy), (sx, sz), (sy, sz))]
        return p

    def _vessel_inputs(self, who: str, vol: DeviceArray, lab: Optional[DeviceArray]):
        text = f"{who}: need a 3-D volume of dtype int16 / int32 / int64 / float32 / float64 (got {vol.shape} {vol.dtype})"
        if len(vol.shape) != 3:
            raise LMError(text)
        code = self._lm_dtype(vol.dtype, signed_only=True, text=text)
        if lab is not None and (lab.dtype != np.uint8 or tuple(lab.shape) != tuple(vol.shape)):
            raise LMError(f"{who}: the labels must be uint8 {vol.shape} (got {lab.dtype} {lab.shape})")
        self._check_size(who, vol.shape)
        if lab is not None and vol.shape[0] == 0:
            raise NoKeptVoxel("vessels: the labels hold no voxel of the kept label values")
        return code

    def hessian_dev(self, vol: DeviceArray, sigma_vox, truncate: float = 4.0, lab: Optional[DeviceArray] = None, keep=None,
                    eigenvalues: bool = False, out: Optional[DeviceArray] = None, eig_out: Optional[DeviceArray] = None):
        """lm_hessian_dev on a device-resident volume at ONE scale (`sigma_vox`: three sigmas in voxels, array axis order) ->
        (components DeviceArray float32 [6][n][h][w] in the order xx, yy, zz, xy, xz, yz, scale-normalised; eigenvalues DeviceArray
        float32 [3][n][h][w] by ascending |lambda|, or None).  With the u8 labels `lab` only the voxels whose label is in `keep` (None:
        every label >= 1) are analysed and the others are 0.  `out`: a float32 [6][n][h][w] DeviceArray for the components;
        `eig_out`: a float32 [3][n][h][w] DeviceArray for the eigenvalues (it asks for them).
        NoKeptVoxel when labels are given and none is selected.  Enqueued on the engine's stream."""
        masked = lab is not None
        p = self._vessel_params([sigma_vox], truncate, masked, keep)
        code = self._vessel_inputs("hessian_dev", vol, lab)
        n, h, w = vol.shape
        if out is not None and (out.dtype != np.float32 or tuple(out.shape) != (6, n, h, w)):
            raise LMError(f"hessian_dev: out must be a float32 array of shape {(6, n, h, w)} (got {out.dtype} {out.shape})")
        if eig_out is not None and (eig_out.dtype != np.float32 or tuple(eig_out.shape) != (3, n, h, w)):
            raise LMError(f"hessian_dev: eig_out must be a float32 array of shape {(3, n, h, w)} (got {eig_out.dtype} {eig_out.shape})")
        eigenvalues = eigenvalues or eig_out is not None
        with self._out_or_new(out, (6, n, h, w), np.float32) as out, self._optional_new(eigenvalues, (3, n, h, w), np.float32, eig_out) as eig:
            rc = self.L.lib.lm_hessian_dev(self.h, vol.ptr, code, lab.ptr if masked else None, n, h, w, C.byref(p), out.ptr,
                                           eig.ptr if eigenvalues else None)
            self._check_kept(rc, "lm_hessian_dev", NoKeptVoxel, "vessels: the labels hold no voxel of the kept label values", keep)
        return out, eig

    def vesselness_dev(self, vol: DeviceArray, sigmas_vox, alpha: float = 0.5, beta: float = 0.5, c: float = 100.0, bright: bool = True,
                       truncate: float = 4.0, lab: Optional[DeviceArray] = None, keep=None, return_scale: bool = False,
                       out: Optional[DeviceArray] = None, scale_out: Optional[DeviceArray] = None):
        """lm_vesselness_dev on a device-resident volume: Frangi's vesselness, the maximum over the scales `sigmas_vox` (1 to 8, each
        three sigmas in voxels in array axis order) -> (V DeviceArray float32 [n][h][w], scale DeviceArray u8 [n][h][w] or None: the
        1-based index of the scale that gave V, 0 where V == 0).  With the u8 labels `lab` only the voxels whose label is in `keep`
        (None: every label >= 1) are analysed and the others are 0.  `out`: a float32 DeviceArray of the volume's shape for V;
        `scale_out`: a u8 DeviceArray of that shape for the scale (it asks for it).
        NoKeptVoxel when labels are given and none is selected.  Enqueued on the engine's stream."""
        masked = lab is not None
        p = self._vessel_params(sigmas_vox, truncate, masked, keep, alpha, beta, c, bright)
        code = self._vessel_inputs("vesselness_dev", vol, lab)
        n, h, w = vol.shape
        if out is not None and (out is vol or out.dtype != np.float32 or tuple(out.shape) != tuple(vol.shape)):
            raise LMError(f"vesselness_dev: out must be another float32 array of shape {vol.shape} (got {out.dtype} {out.shape})")
        if scale_out is not None and (scale_out is vol or scale_out is lab or scale_out.dtype != np.uint8 or tuple(scale_out.shape) != tuple(vol.shape)):
            raise LMError(f"vesselness_dev: scale_out must be another uint8 array of shape {vol.shape} (got {scale_out.dtype} {scale_out.shape})")
        return_scale = return_scale or scale_out is not None
        with self._out_or_new(out, vol.shape, np.float32) as out, self._optional_new(return_scale, vol.shape, np.uint8, scale_out) as sc:
            rc = self.L.lib.lm_vesselness_dev(self.h, vol.ptr, code, lab.ptr if masked else None, n, h, w, C.byref(p), out.ptr,
                                              sc.ptr if return_scale else None)
            self._check_kept(rc, "lm_vesselness_dev", NoKeptVoxel, "vessels: the labels hold no voxel of the kept label values", keep)
        return out, sc

    def vesselness(self, vol: np.ndarray, sigmas_vox, lab: Optional[np.ndarray] = None, return_scale: bool = False, **kw):
        """Host form of vesselness_dev: the volume (and the labels) are copied to the device first -> V as a numpy array, or
        (V, scale) with `return_scale`."""
        vol = np.ascontiguousarray(vol)
        if vol.ndim != 3 or (lab is not None and tuple(np.shape(lab)) != vol.shape):
            raise LMError(f"vesselness: need a 3-D volume and labels of the same shape (got {vol.shape}, {None if lab is None else np.shape(lab)})")
        self._lm_dtype(vol.dtype, "vesselness")
        with self.scope() as dev:
            vd = dev.upload(vol)
            ld = dev.upload(lab, np.uint8) if lab is not None else None
            v, sc = dev.add(*self.vesselness_dev(vd, sigmas_vox, lab=ld, return_scale=return_scale, **kw))
            self.sync()
            return (v.download(), sc.download()) if return_scale else v.download()

    def hessian(self, vol: np.ndarray, sigma_vox, lab: Optional[np.ndarray] = None, eigenvalues: bool = False, **kw):
        """Host form of hessian_dev -> the components [6][n][h][w] as a numpy array, or (components, eigenvalues [3][n][h][w])."""
        vol = np.ascontiguousarray(vol)
        if vol.ndim != 3 or (lab is not None and tuple(np.shape(lab)) != vol.shape):
            raise LMError(f"hessian: need a 3-D volume and labels of the same shape (got {vol.shape}, {None if lab is None else np.shape(lab)})")
        self._lm_dtype(vol.dtype, "hessian")
        with self.scope() as dev:
            vd = dev.upload(vol)
            ld = dev.upload(lab, np.uint8) if lab is not None else None
            comp, eig = dev.add(*self.hessian_dev(vd, sigma_vox, lab=ld, eigenvalues=eigenvalues, **kw))
            self.sync()
            return (comp.download(), eig.download()) if eigenvalues else comp.download()

    def vessel_counts_dev(self, v: DeviceArray, scale: DeviceArray, lab: DeviceArray, threshold: float, n_labels: int = 16) -> np.ndarray:
        """lm_vessel_counts_dev: int64 [n_labels][9], counts[l][s] = the voxels with label l (1 .. n_labels - 1), scale index s and
        V >= threshold.  Returns once the counts are on the host."""
        if v.dtype != np.float32 or len(v.shape) != 3 or scale.dtype != np.uint8 or lab.dtype != np.uint8 or \
                tuple(scale.shape) != tuple(v.shape) or tuple(lab.shape) != tuple(v.shape):
            raise LMError(f"vessel_counts_dev: need float32 V, u8 scale and u8 labels of one 3-D shape (got {v.dtype} {v.shape}, "
                          f"{scale.dtype} {scale.shape}, {lab.dtype} {lab.shape})")
        if not 1 <= int(n_labels) <= 16:
            raise ValueError(f"n_labels: 1..16, got {n_labels!r}")
        self._check_size("vessel_counts_dev", v.shape)
        n, h, w = v.shape
        counts = np.zeros((int(n_labels), VESSEL_COUNT_COLUMNS), np.int64)
        self.L.check(self.L.lib.lm_vessel_counts_dev(self.h, v.ptr, scale.ptr, lab.ptr, n, h, w, int(n_labels), float(threshold),
                                                     counts.ctypes.data_as(_PTR(_I64))), "lm_vessel_counts_dev")
        return counts

    # -- skeleton and calibre classes (include/lungmask_hip.h: lm_skeleton_dev, lm_skeleton_points_dev, lm_calibre_dev)
    def _u8_volume(self, who: str, arr: DeviceArray, shape=None):
        if arr.dtype != np.uint8 or len(arr.shape) != 3 or (shape is not None and tuple(arr.shape) != tuple(shape)):
            raise LMError(f"{who}: need a 3-D u8 volume{'' if shape is None else f' of shape {tuple(shape)}'} (got {arr.shape} {arr.dtype})")
        self._check_size(who, arr.shape)

    def skeleton_dev(self, sel: DeviceArray, keep=None, out: Optional[DeviceArray] = None):
        """lm_skeleton_dev on a device-resident u8 volume: the topology-preserving curve skeleton of the voxels whose value is in
        `keep` (None: every value >= 1) -> (codes DeviceArray u8: 0, or 1 + the number of skeleton voxels among the 26 neighbours --
        1 isolated, 2 end, 3 curve, >= 4 junction; info dict: selected, skeleton, passes).  `out`: a u8 DeviceArray of the same shape
        to receive the codes (may be `sel`; default: a new one).  NoKeptVoxel when no voxel is selected.  Returns once the counts are
        on the host."""
        self._u8_volume("skeleton_dev", sel)
        table = self._keep_table(keep)
        if out is not None:
            self._u8_volume("skeleton_dev", out, sel.shape)
        n, h, w = sel.shape
        if n == 0:
            raise NoKeptVoxel("skeleton: the volume holds no voxel of the kept values")
        info = (C.c_int64 * 4)()
        with self._out_or_new(out, sel.shape, np.uint8) as out:
            rc = self.L.lib.lm_skeleton_dev(self.h, sel.ptr, n, h, w, table, out.ptr, info)
            self._check_kept(rc, "lm_skeleton_dev", NoKeptVoxel, "skeleton: the volume holds no voxel of the kept values", keep)
        return out, {"selected": int(info[0]), "skeleton": int(info[1]), "passes": int(info[2])}

    def skeleton(self, sel: np.ndarray, keep=None, return_info: bool = False):
        """Host form of skeleton_dev: the volume is copied to the device first -> the codes as a numpy array (or (codes, info))."""
        sel = np.ascontiguousarray(sel, dtype=np.uint8)
        if sel.ndim != 3:
            raise LMError(f"skeleton: need a 3-D volume (got {sel.shape})")
        with self.scope() as dev:
            sd = dev.upload(sel)
            _, info = self.skeleton_dev(sd, keep, out=sd)
            codes = sd.download()
        return (codes, info) if return_info else codes

    def skeleton_points_dev(self, skel: DeviceArray, d2: Optional[DeviceArray] = None, cap: Optional[int] = None,
                            index_out: Optional[DeviceArray] = None, code_out: Optional[DeviceArray] = None,
                            d2_out: Optional[DeviceArray] = None):
        """lm_skeleton_points_dev: the non-zero voxels of the device code volume `skel` in ascending raster order -> (index int32
        [m], code u8 [m], d2 float32 [m] or None, total) as numpy arrays, m = min(total, cap); `d2`: a float32 DeviceArray of the same
        shape sampled at the points.  cap None: as many as there are (counted first).  `index_out` / `code_out` / `d2_out`: 1-D
        int32 / u8 / float32 DeviceArrays of one length >= cap for the device to write the list into (default: new ones, freed
        again); given together, `d2_out` exactly when `d2` is.  Only their first m entries are written."""
        self._u8_volume("skeleton_points_dev", skel)
        if d2 is not None and (d2.dtype != np.float32 or tuple(d2.shape) != tuple(skel.shape)):
            raise LMError(f"skeleton_points_dev: d2 must be float32 {skel.shape} (got {d2.dtype} {d2.shape})")
        if cap is not None and (int(cap) != cap or cap < 0):
            raise ValueError(f"cap: an integer >= 0 or None, got {cap!r}")
        outs = ((index_out, np.int32), (code_out, np.uint8), (d2_out, np.float32))
        given = any(o is not None for o, _ in outs)
        if given:
            if index_out is None or code_out is None or (d2_out is None) != (d2 is None):
                raise LMError("skeleton_points_dev: index_out and code_out are given together, d2_out exactly when d2 is")
            for o, dt in outs:
                if o is not None and (o.dtype != dt or len(o.shape) != 1 or o.shape[0] != index_out.shape[0]):
                    raise LMError(f"skeleton_points_dev: index_out / code_out / d2_out must be int32 / uint8 / float32 arrays of one length "
                                  f"(got {o.dtype} {o.shape})")
        n, h, w = skel.shape
        total = C.c_int64()
        fn = self.L.lib.lm_skeleton_points_dev
        if given:
            if cap is not None and cap > index_out.shape[0]:
                raise LMError(f"skeleton_points_dev: cap = {cap} exceeds the {index_out.shape[0]} entries of index_out")
            cap = index_out.shape[0] if cap is None else cap
        if cap is None:
            self.L.check(fn(self.h, skel.ptr, None, n, h, w, 0, None, None, None, C.byref(total)), "lm_skeleton_points_dev")
            cap = int(total.value)
        cap = int(cap)
        if cap == 0:
            self.L.check(fn(self.h, skel.ptr, None, n, h, w, 0, None, None, None, C.byref(total)), "lm_skeleton_points_dev")
            return np.zeros(0, np.int32), np.zeros(0, np.uint8), None if d2 is None else np.zeros(0, np.float32), int(total.value)
        with self.scope() as dev:
            if given:
                idx, code, dd = index_out, code_out, d2_out
            else:
                idx, code = dev.empty((cap,), np.int32), dev.empty((cap,), np.uint8)
                dd = dev.empty((cap,), np.float32) if d2 is not None else None
            self.L.check(fn(self.h, skel.ptr, d2.ptr if d2 is not None else None, n, h, w, cap, idx.ptr, code.ptr,
                            dd.ptr if dd is not None else None, C.byref(total)), "lm_skeleton_points_dev")
            m = min(int(total.value), cap)
            return idx.download()[:m], code.download()[:m], None if dd is None else dd.download()[:m], int(total.value)

    @staticmethod
    def _calibre_edges(edges_mm):
        import math

        edges = [float(v) for v in edges_mm]
        if not 1 <= len(edges) <= CALIBRE_MAX_EDGES or not all(math.isfinite(v) and 0 < v < 1e15 for v in edges) or \
                any(b <= a for a, b in zip(edges, edges[1:])):
            raise ValueError(f"edges_mm: 1 to {CALIBRE_MAX_EDGES} strictly ascending values > 0 and < 1e15, got {edges_mm!r}")
        return edges

    def calibre_dev(self, skel: DeviceArray, sel: DeviceArray, edges_mm, spacing=None, keep=None, lab: Optional[DeviceArray] = None,
                    n_labels: int = 16, return_distance: bool = False, out: Optional[DeviceArray] = None,
                    d2_out: Optional[DeviceArray] = None):
        """lm_calibre_dev: the calibre class of every voxel of the mask M (the voxels of `sel` whose value is in `keep`; None: every
        value >= 1) -> (classes DeviceArray u8, counts int64 [n_labels][9], d2 DeviceArray float32 or None).  A skeleton voxel
        (`skel`, skeleton_dev's codes) gets the class 1 + the number of `edges_mm` its distance to the outside of M reaches; every
        voxel of M takes the class of the nearest skeleton voxel (nearest_label_dev's rule); counts[k][c] = the voxels of M with
        label k (`lab`; None: all in row 1) and class c.  `out` / `d2_out`: a u8 / float32 DeviceArray of the volume's shape to
        receive the classes / the squared distances (`d2_out` asks for them).  Returns once the counts are on the host."""
        self._u8_volume("calibre_dev", skel)
        self._u8_volume("calibre_dev", sel, skel.shape)
        if lab is not None:
            self._u8_volume("calibre_dev", lab, skel.shape)
        if out is not None:
            self._u8_volume("calibre_dev", out, skel.shape)
            if out is skel or out is sel or out is lab:
                raise LMError("calibre_dev: out must not be one of the inputs")
        if d2_out is not None and (d2_out.dtype != np.float32 or tuple(d2_out.shape) != tuple(skel.shape)):
            raise LMError(f"calibre_dev: d2_out must be a float32 array of shape {tuple(skel.shape)} (got {d2_out.dtype} {d2_out.shape})")
        return_distance = return_distance or d2_out is not None
        edges = self._calibre_edges(edges_mm)
        if not 2 <= int(n_labels) <= 16:
            raise ValueError(f"n_labels: 2..16, got {n_labels!r}")
        table = self._keep_table(keep)
        sp = self._spacing3(spacing, "calibre_dev")
        n, h, w = skel.shape
        counts = np.zeros((int(n_labels), CALIBRE_COLUMNS), np.int64)
        with self._out_or_new(out, skel.shape, np.uint8) as out, self._optional_new(return_distance, skel.shape, np.float32, d2_out) as d2:
            self.L.check(self.L.lib.lm_calibre_dev(self.h, skel.ptr, sel.ptr, table, lab.ptr if lab is not None else None, n, h, w, sp,
                                                   (C.c_double * len(edges))(*edges), len(edges), int(n_labels), out.ptr,
                                                   d2.ptr if d2 is not None else None, counts.ctypes.data_as(_PTR(_I64))),
                         "lm_calibre_dev")
        return out, counts, d2

    def calibre(self, skel: np.ndarray, sel: np.ndarray, edges_mm, lab: Optional[np.ndarray] = None, return_distance: bool = False, **kw):
        """Host form of calibre_dev -> (classes, counts) as numpy arrays, or (classes, counts, d2) with `return_distance`."""
        skel = np.ascontiguousarray(skel, dtype=np.uint8)
        if skel.ndim != 3 or np.shape(sel) != skel.shape or (lab is not None and np.shape(lab) != skel.shape):
            raise LMError(f"calibre: need 3-D volumes of one shape (got {skel.shape}, {np.shape(sel)})")
        with self.scope() as dev:
            kd, sd = dev.upload(skel), dev.upload(sel, np.uint8)
            ld = dev.upload(lab, np.uint8) if lab is not None else None
            cls, counts, d2 = self.calibre_dev(kd, sd, edges_mm, lab=ld, return_distance=return_distance, **kw)
            dev.add(cls, d2)
            return (cls.download(), counts, d2.download()) if return_distance else (cls.download(), counts)

    def vessel_mask_dev(self, v: DeviceArray, lab: DeviceArray, threshold: float, out: Optional[DeviceArray] = None) -> DeviceArray:
        """lm_vessel_mask_dev: u8 DeviceArray, 1 where the device labels `lab` are not 0 and the float32 map `v` reaches `threshold`.
        `out`: a u8 DeviceArray of the same shape (may be `lab`; default: a new one).  Enqueued on the engine's stream."""
        self._u8_volume("vessel_mask_dev", lab)
        if v.dtype != np.float32 or tuple(v.shape) != tuple(lab.shape):
            raise LMError(f"vessel_mask_dev: v must be float32 {lab.shape} (got {v.dtype} {v.shape})")
        if out is not None:
            self._u8_volume("vessel_mask_dev", out, lab.shape)
        n, h, w = lab.shape
        with self._out_or_new(out, lab.shape, np.uint8) as out:
            self.L.check(self.L.lib.lm_vessel_mask_dev(self.h, v.ptr, lab.ptr, n, h, w, float(threshold), out.ptr), "lm_vessel_mask_dev")
        return out

    # -- seeded minimax flood and the airway mask (include/lungmask_hip.h: lm_seed_cost_dev, lm_airway_mask_dev)
    @staticmethod
    def _seed_indices(who: str, seeds, shape):
        """The raster indices (int64) of `seeds`: one (z, y, x) or a sequence of 1 to 64 of them, inside a volume of `shape`."""
        try:
            arr = np.asarray(seeds)
        except ValueError:
            arr = np.zeros(0)
        if arr.dtype.kind not in "iu" or arr.size == 0 or arr.ndim not in (1, 2) or arr.shape[-1] != 3:
            raise ValueError(f"{who}: seeds must be one (z, y, x) of integers or a sequence of them, got {seeds!r}")
        zyx = arr.reshape(-1, 3).astype(np.int64)
        if len(zyx) > SEED_MAX:
            raise ValueError(f"{who}: 1 to {SEED_MAX} seeds, got {len(zyx)}")
        if (zyx < 0).any() or (zyx >= np.asarray(shape)).any():
            raise ValueError(f"{who}: a seed lies outside the volume of shape {tuple(shape)}: {seeds!r}")
        return np.ascontiguousarray((zyx[:, 0] * shape[1] + zyx[:, 1]) * shape[2] + zyx[:, 2], dtype=np.int64)

    def seed_cost_bricks(self, shape):
        """(number of bricks, (bz, by, bx)) of lm_seed_cost_dev's tiling of a volume of `shape`."""
        b, br = C.c_int64(), (C.c_int32 * 3)()
        self.L.check(self.L.lib.lm_seed_cost_bricks(int(shape[0]), int(shape[1]), int(shape[2]), C.byref(b), br), "lm_seed_cost_bricks")
        return int(b.value), tuple(int(v) for v in br)

    def seed_cost_dev(self, vol: DeviceArray, seeds, cap_hu: int = -800, max_rounds: Optional[int] = None, out: Optional[DeviceArray] = None):
        """lm_seed_cost_dev on a device-resident image: the minimax cost from the seeds -- per voxel the smallest threshold at which
        it connects to a seed through 6-connected voxels with HU <= cap_hu, 32767 where it never does -> (cost DeviceArray int16,
        curve int64 [cap_hu + 1025]: the voxels with cost == -1024 + k, info dict: rounds, reached, seeds_passable, converged).
        `seeds`: one (z, y, x) or a sequence of 1 to 64 of them.  `max_rounds`: None = the
        number of voxels + 1, which no converging run can reach -- after round j + 1 every voxel whose best path crosses brick faces j
        times is final, and a path that repeats no voxel crosses fewer faces than there are voxels; a smaller value bounds the latency
        and raises LMError ("max_rounds") when it is spent first.  `out`: an int16 DeviceArray of the image's shape."""
        if len(vol.shape) != 3:
            raise LMError(f"seed_cost_dev: need a 3-D volume (got {vol.shape})")
        code = self._lm_dtype(vol.dtype, "seed_cost_dev", signed_only=True)
        self._check_size("seed_cost_dev", vol.shape)
        if int(cap_hu) != cap_hu or not -1023 <= cap_hu <= 3071:
            raise ValueError(f"cap_hu: an integer in -1023 .. 3071, got {cap_hu!r}")
        n, h, w = vol.shape
        if n * h * w == 0:
            raise ValueError("seed_cost_dev: the volume is empty")
        flat = self._seed_indices("seed_cost_dev", seeds, vol.shape)
        if max_rounds is None:
            max_rounds = n * h * w + 1
        if int(max_rounds) != max_rounds or max_rounds < 0:
            raise ValueError(f"max_rounds: an integer >= 0 or None, got {max_rounds!r}")
        if out is not None and (out.dtype != np.int16 or tuple(out.shape) != tuple(vol.shape) or out is vol):
            raise LMError(f"seed_cost_dev: out must be another int16 DeviceArray of shape {tuple(vol.shape)} (got {out.dtype} {out.shape})")
        curve = np.zeros(int(cap_hu) + 1025, np.int64)
        info = (C.c_int64 * 4)()
        with self._out_or_new(out, vol.shape, np.int16) as out:
            self.L.check(self.L.lib.lm_seed_cost_dev(self.h, vol.ptr, code, n, h, w, flat.ctypes.data_as(_PTR(_I64)), int(flat.size), int(cap_hu),
                                                     int(max_rounds), out.ptr, curve.ctypes.data, info), "lm_seed_cost_dev")
        return out, curve, {"rounds": int(info[0]), "reached": int(info[1]), "seeds_passable": int(info[2]), "converged": bool(info[3])}

    def seed_cost(self, vol: np.ndarray, seeds, cap_hu: int = -800, max_rounds: Optional[int] = None):
        """Host form of seed_cost_dev: the volume is copied to the device first -> (cost int16 numpy array, curve, info)."""
        vol = np.ascontiguousarray(vol)
        if vol.ndim != 3:
            raise LMError(f"seed_cost: need a 3-D volume (got {vol.shape})")
        with self.scope() as dev:
            vd = dev.upload(vol)
            cost, curve, info = self.seed_cost_dev(vd, seeds, cap_hu, max_rounds)
            dev.add(cost)
            return cost.download(), curve, info

    def airway_mask_dev(self, cost: DeviceArray, threshold: int, lab: Optional[DeviceArray] = None, out: Optional[DeviceArray] = None):
        """lm_airway_mask_dev: (mask DeviceArray u8 = 1 where the int16 `cost` <= threshold, counts int64 [256]: the mask voxels per
        value of the u8 labels `lab`, all in entry 0 without labels).  `out`: a u8 DeviceArray of the same shape, not an input."""
        if cost.dtype != np.int16 or len(cost.shape) != 3:
            raise LMError(f"airway_mask_dev: cost must be a 3-D int16 volume (got {cost.shape} {cost.dtype})")
        self._check_size("airway_mask_dev", cost.shape)
        if lab is not None:
            self._u8_volume("airway_mask_dev", lab, cost.shape)
        if out is not None:
            self._u8_volume("airway_mask_dev", out, cost.shape)
            if out is lab:
                raise LMError("airway_mask_dev: out must not be one of the inputs")
        if int(threshold) != threshold or not -32768 <= threshold <= 32766:
            raise ValueError(f"threshold: an integer in -32768 .. 32766, got {threshold!r}")
        n, h, w = cost.shape
        counts = np.zeros(256, np.int64)
        with self._out_or_new(out, cost.shape, np.uint8) as out:
            self.L.check(self.L.lib.lm_airway_mask_dev(self.h, cost.ptr, lab.ptr if lab is not None else None, n, h, w, int(threshold), out.ptr,
                                                       counts.ctypes.data), "lm_airway_mask_dev")
        return out, counts

    # -- surface mesh (include/lungmask_hip.h: lm_mesh_plan_dev, lm_mesh_dev)
    def mesh_plan_dev(self, lab: DeviceArray, keep=None):
        """(bbox, n_vertices, n_quads) of the surface-nets mesh of the voxels of the device labels whose value is in `keep` (None:
        every label >= 1).  ValueError when there is no such voxel."""
        if lab.dtype != np.uint8 or len(lab.shape) != 3:
            raise LMError(f"mesh_plan_dev: need a 3-D u8 label volume (got {lab.shape} {lab.dtype})")
        n, h, w = lab.shape
        bb = (C.c_int32 * 6)()
        nv, nq = C.c_int64(0), C.c_int64(0)
        rc = self.L.lib.lm_mesh_plan_dev(self.h, lab.ptr, n, h, w, self._keep_table(keep), bb, C.byref(nv), C.byref(nq))
        self._check_kept(rc, "lm_mesh_plan_dev", ValueError, "mesh: the labels hold no voxel of the kept label values", keep)
        return [int(v) for v in bb], int(nv.value), int(nq.value)

    def mesh_dev(self, lab: DeviceArray, keep=None, smooth: int = 0, lam: float = 0.5, mu: float = -0.53, out=None):
        """The surface-nets mesh of the device-resident labels (lm_mesh_dev's definition, include/lungmask_hip.h): -> (vertices
        DeviceArray float32 [V][3] in array index coordinates (z, y, x), quads DeviceArray int32 [Q][4], info) with info = {bbox,
        n_vertices, n_quads}.  Nothing but the box and the two counts crosses to the host.  `out`: a callable (n_vertices, n_quads) ->
        (float32 [V][3] DeviceArray, int32 [Q][4] DeviceArray) that provides the two results (default: new allocations).  Enqueued on
        the engine's stream."""
        import math

        if int(smooth) != smooth or not 0 <= int(smooth) <= 100000:
            raise ValueError(f"smooth: a number of iterations in 0..100000, got {smooth!r}")
        if not (math.isfinite(lam) and math.isfinite(mu)):
            raise ValueError(f"lam and mu must be finite, got {lam!r}, {mu!r}")
        if len(lab.shape) == 3 and lab.shape[0] == 0:
            raise ValueError("mesh: the labels hold no voxel of the kept label values")
        table = self._keep_table(keep)
        bbox, nv, nq = self.mesh_plan_dev(lab, keep)
        n, h, w = lab.shape
        given = (None, None) if out is None else out(nv, nq)
        with self._out_or_new(given[0], (nv, 3), np.float32) as verts, self._out_or_new(given[1], (nq, 4), np.int32) as quads:
            if (verts.dtype, quads.dtype) != (np.float32, np.int32) or tuple(verts.shape) != (nv, 3) or tuple(quads.shape) != (nq, 4):
                raise LMError(f"mesh_dev(out=...): need float32 {(nv, 3)} and int32 {(nq, 4)}")
            self.L.check(self.L.lib.lm_mesh_dev(self.h, lab.ptr, n, h, w, table, int(smooth), float(lam), float(mu), verts.ptr, nv,
                                                quads.ptr, nq), "lm_mesh_dev")
        return verts, quads, {"bbox": bbox, "n_vertices": nv, "n_quads": nq}

    def mesh(self, lab: np.ndarray, **kw):
        """Host form of mesh_dev: the labels are copied to the device first -> (vertices, quads, info) as numpy arrays."""
        lab = np.ascontiguousarray(lab, dtype=np.uint8)
        if lab.ndim != 3:
            raise LMError(f"mesh: need a 3-D label volume (got {lab.shape})")
        with self.scope() as dev:
            verts, quads, info = self.mesh_dev(dev.upload(lab), **kw)
            dev.add(verts, quads)
            self.sync()
            return verts.download(), quads.download(), info

    def postprocess_info(self) -> dict:
        buf = (C.c_int64 * 5)()
        self.L.check(self.L.lib.lm_postprocess_info(self.h, buf))
        return dict(regions=buf[0], boundary_records=buf[1], processed=buf[2], merged=buf[3], host_replay_ms=buf[4] / 1000.0)

    def fuse(self, res_l: np.ndarray, res_r: np.ndarray):
        """mask.py:228-230 -> (fused volume incl. spare label, spare value)."""
        sp = C.c_int()
        with self.scope() as dev:
            ld, rd = dev.upload(res_l, np.uint8), dev.upload(res_r, np.uint8)
            self.L.check(self.L.lib.lm_fuse_dev(self.h, ld.ptr, rd.ptr, ld.nbytes, C.byref(sp)), "lm_fuse_dev")
            self.sync()
            return ld.download(), sp.value

    # -- the whole hot path
    def apply_dev(self, slot: int, vol: DeviceArray, out: DeviceArray, fill_slot: int = -1, batch_size: int = 20, volume_postprocessing: bool = True):
        n, h, w = vol.shape
        self.L.check(
            self.L.lib.lm_apply_dev(self.h, slot, fill_slot, vol.ptr, self._lm_dtype(vol.dtype), n, h, w, int(batch_size), int(bool(volume_postprocessing)), out.ptr),
            "lm_apply_dev",
        )

    # -- volumes queued through the engine (lm_pipe_*; LMInferer.apply_async drives them from two threads)
    def pipe_upload(self, k: int, vol: Optional[np.ndarray]):
        if vol is None:
            self.L.check(self.L.lib.lm_pipe_upload(self.h, k, None, 0), "lm_pipe_upload")
        else:
            self.L.check(self.L.lib.lm_pipe_upload(self.h, k, vol.ctypes.data, vol.nbytes), "lm_pipe_upload")

    def pipe_apply(self, k: int, slot: int, shape, dtype, fill_slot: int = -1, batch_size: int = 20, volume_postprocessing: bool = True):
        n, h, w = (int(v) for v in shape)
        self.L.check(self.L.lib.lm_pipe_apply(self.h, k, slot, fill_slot, LM_DTYPES[np.dtype(dtype)], n, h, w, int(batch_size), int(bool(volume_postprocessing))),
                     "lm_pipe_apply")

    def pipe_download(self, k: int, out: np.ndarray):
        self.L.check(self.L.lib.lm_pipe_download(self.h, k, out.ctypes.data, out.nbytes), "lm_pipe_download")

    def pipe_wait(self, k: int):
        self.L.check(self.L.lib.lm_pipe_wait(self.h, k), "lm_pipe_wait")

    def pipe_query(self, k: int) -> bool:
        """Whether the copy-back last enqueued on result buffer k has arrived (never blocks)."""
        return self.L.check(self.L.lib.lm_pipe_query(self.h, k), "lm_pipe_query") > 0

    def apply(self, slot: int, vol: np.ndarray, fill_slot: int = -1, batch_size: int = 20, volume_postprocessing: bool = True,
              out: Optional[np.ndarray] = None, out_scratch: bool = False) -> np.ndarray:
        """numpy -> numpy (lm_apply_host).  `out`: an optional caller-owned uint8 C-contiguous array of the volume's shape to
        receive the labels (a reused buffer spares the page faults and the unmapping of a fresh 79 MB array per volume).
        `out_scratch`: the contents of `out` are of no value (LM_APPLY_OUT_SCRATCH): it is zero-filled while the network runs and
        only the slab that carries labels is copied back; always so for an array allocated here."""
        vol = np.ascontiguousarray(vol)
        code = self._lm_dtype(vol.dtype)
        n, h, w = vol.shape
        if out is None:
            out, out_scratch = np.empty((n, h, w), dtype=np.uint8), True
        elif out.dtype != np.uint8 or out.shape != (n, h, w) or not out.flags.c_contiguous:
            raise LMError("apply(out=...): need a C-contiguous uint8 array of the volume's shape")
        args = (self.h, slot, fill_slot, vol.ctypes.data, code, n, h, w, int(batch_size), int(bool(volume_postprocessing)), out.ctypes.data)
        if out_scratch and hasattr(self.L.lib, "lm_apply_host_ex"):
            self.L.check(self.L.lib.lm_apply_host_ex(*args, 1), "lm_apply_host_ex")
        else:
            self.L.check(self.L.lib.lm_apply_host(*args), "lm_apply_host")
        return out

    # -- profiling
    def profile(self, on):
        """on: False/True, or 2 for one entry per conv layer shape."""
        self.L.check(self.L.lib.lm_profile_enable(self.h, int(on)))

    def profile_reset(self):
        self.L.check(self.L.lib.lm_profile_reset(self.h))

    def profile_timeline(self, cap: int = 4096):
        """After profile(4): [(name, lane, start_ms, end_ms)] of every launch since the last reset."""
        buf = (LaunchSpan * cap)()
        n = self.L.check(self.L.lib.lm_profile_timeline(self.h, buf, cap))
        return [(buf[i].name.decode(), buf[i].lane, buf[i].start_ms, buf[i].end_ms) for i in range(min(n, cap))]

    def profile_read(self):
        buf = (KernelStat * 96)()
        n = self.L.check(self.L.lib.lm_profile_read(self.h, buf, 96))
        return [
            dict(name=buf[i].name.decode(), launches=buf[i].launches, total_ms=buf[i].total_ms, flops=buf[i].flops, bytes=buf[i].bytes)
            for i in range(min(n, 96))
        ]
