"""Lung ROI: the CT cut down to the lungs with a label mask -- box, margin, resampling, blanking, window -- on the GPU (not in the
reference: what callers do with `scipy.ndimage` right after `LMInferer.apply()`).

The device pass (`lm_roi_dev`, lungmask_amd/csrc/roi_kernels.hip) follows the definition in include/lungmask_hip.h; with s_i the
source spacing and t_i the output spacing of array axis i:

- Box: bbox_3D (margin 0) of the voxels whose label is in `keep`, grown per axis by ceil(margin_mm / s_i) voxels (margin_mm voxels
  without a spacing), clipped to the volume; extents e_i.  No kept voxel: ValueError.
- Grid: step_i = t_i / s_i, N_i = floor((e_i - 1) / step_i) + 1; output index o samples min(o * step_i, e_i - 1) from the box start.
- Intensity: trilinear in float64 (x, then y, then z; lerp(a, b, f) = a * (1 - f) + b * f), one rounding at the end.  Labels: nearest
  neighbour, the raw label values.
- Inside: the voxel's label is in `keep`; with dilate_mm > 0, the exact Euclidean distance (mm) of its nearest source voxel to the
  kept voxels is <= dilate_mm.  `mask_outside` gives every other voxel `fill`.
- window=(lo, hi): clip, then (v - lo) / (hi - lo).  dtype float32, float16 (== the float32 result's astype(float16)) or int16
  (rint, saturated; integer volumes without a window only).

Everything is in the caller's array orientation (no LPS re-orientation), as the statistics are.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _native


class Roi:
    """What `extract_roi` / `LMInferer.apply_roi` return: `image` (the array, of the requested dtype), `labels` (uint8, same shape:
    the labels on the ROI grid), `bbox` (zmin, zmax, ymin, ymax, xmin, xmax in source indices, exclusive maxima), `spacing_mm`
    (array axis order; None without a spacing) and `source_step` (source voxels per output voxel, per axis)."""

    def __init__(self, image: np.ndarray, labels: np.ndarray, bbox, spacing_mm, source_step, geometry=None):
        self.image = image
        self.labels = labels
        self.bbox = [int(v) for v in bbox]
        self.spacing_mm = None if spacing_mm is None else [float(v) for v in spacing_mm]
        self.source_step = [float(v) for v in source_step]
        self._geometry = geometry  # (index_to_physical of the source, its direction 3 x 3, its meta) or None

    def as_volume(self, array: Optional[np.ndarray] = None):
        """The ROI as a `volume_io.Volume` (`array`: `labels` or any array of the ROI's shape instead of `image`): the origin is
        the physical position of the box's first voxel, the direction the input's, the spacing the ROI's."""
        from . import volume_io

        if self._geometry is None or self.spacing_mm is None:
            raise ValueError("as_volume: the ROI of a bare numpy array has no geometry (pass a Volume or a SimpleITK image)")
        to_phys, direction, meta = self._geometry
        arr = self.image if array is None else array
        assert tuple(arr.shape) == tuple(self.image.shape), (arr.shape, self.image.shape)
        origin = to_phys([self.bbox[0], self.bbox[2], self.bbox[4]])
        return volume_io.Volume(arr, tuple(self.spacing_mm[::-1]), tuple(float(v) for v in origin), direction, meta)

    def meta(self) -> dict:
        """The non-array fields, JSON-serialisable."""
        return {"shape": [int(v) for v in self.image.shape], "dtype": str(self.image.dtype), "bbox": list(self.bbox),
                "spacing_mm": None if self.spacing_mm is None else list(self.spacing_mm), "source_step": list(self.source_step)}


def _geometry_of(image):
    """(index_to_physical, direction, meta) of a Volume / SimpleITK image; None for a numpy array."""
    from . import stats as st
    from . import volume_io

    if isinstance(image, np.ndarray):
        return None
    _, _, to_phys = st.geometry(image)
    if isinstance(image, volume_io.Volume):
        return to_phys, np.asarray(image.direction, np.float64).reshape(3, 3).copy(), image.meta
    return to_phys, np.asarray(image.GetDirection(), np.float64).reshape(3, 3), None


def check_arguments(arr_dtype, sp, spacing_out, margin_mm, keep, dilate_mm, window, dtype):
    """The argument errors of extract_roi / apply_roi, raised before anything runs on the device."""
    dt = np.dtype(dtype)
    if dt not in _native.LM_ROI_DTYPES:
        raise TypeError(f"ROI dtype float32, float16 or int16, not {dt}")
    if dt == np.int16 and (np.dtype(arr_dtype).kind == "f" or window is not None):
        raise ValueError("ROI dtype int16 needs an integer volume and no window")
    if spacing_out is not None and sp is None:
        raise ValueError("spacing_out needs the source spacing: pass spacing= with a bare numpy array")
    if not (margin_mm >= 0) or not (0.0 <= dilate_mm <= margin_mm):
        raise ValueError(f"0 <= dilate_mm <= margin_mm is required (got dilate_mm {dilate_mm!r}, margin_mm {margin_mm!r})")
    if window is not None and not (len(window) == 2 and float(window[1]) > float(window[0])):
        raise ValueError(f"window=(lo, hi) needs lo < hi, got {window!r}")
    _native.Engine._keep_table(keep)


def from_device(img, out_lab, info, geometry) -> Roi:
    """The host `Roi` of roi_dev's device arrays (downloaded and freed here)."""
    try:
        img.eng.sync()
        return Roi(img.download(), out_lab.download(), info["bbox"], info["spacing_mm"], info["step"], geometry)
    finally:
        img.free()
        out_lab.free()


def extract_roi(image, labels, spacing=None, spacing_out=None, margin_mm=5.0, keep=None, dilate_mm=0.0, mask_outside=True, fill=-1024,
                window=None, dtype=np.float32, engine=None) -> Roi:
    """The lung ROI of `image` (numpy [n, h, w], a `volume_io.Volume` or a SimpleITK image) under `labels` (u8-valued, same shape: a
    mask from `apply`, from the reference or edited by hand), computed on the GPU -> `Roi`.

    `spacing`: numpy input only, in the array's axis order.  `spacing_out`: one value (isotropic) or three in array axis order; None
    = the source spacing, a pure crop.  `margin_mm`: the box is grown by it on every side.  `keep`: label values (1..255) that make
    up the ROI (default: every label >= 1).  `dilate_mm` (<= margin_mm): voxels within that distance of the kept voxels count as
    inside.  `mask_outside`: voxels that are not inside take `fill`.  `window=(lo, hi)`: clip and scale to [0, 1].  `dtype`: float32,
    float16 or int16 (integer volumes without a window).  `engine`: a _native.Engine (default: a new one on device 0)."""
    from . import stats as st
    from .mask import LMInferer

    arr, sp, _ = st.geometry(image, spacing)
    lab = np.ascontiguousarray(st._label_array(labels))
    if lab.shape != arr.shape or lab.ndim != 3:
        raise ValueError(f"labels {lab.shape} and image {arr.shape} must be 3-D volumes of the same shape")
    if lab.dtype != np.uint8:
        if lab.size and (lab.min() < 0 or lab.max() > 255):
            raise ValueError("labels must lie in 0..255")
        lab = lab.astype(np.uint8)
    vol = np.ascontiguousarray(LMInferer._engine_dtype(np.asarray(arr)))
    check_arguments(vol.dtype, sp, spacing_out, margin_mm, keep, dilate_mm, window, dtype)
    with _native.engine_scope(engine) as eng:
        img, out_lab, info = eng.roi(vol, lab, spacing=sp, spacing_out=spacing_out, margin_mm=margin_mm, keep=keep, dilate_mm=dilate_mm,
                                     mask_outside=mask_outside, fill=fill, window=window, dtype=dtype)
    return Roi(img, out_lab, info["bbox"], info["spacing_mm"], info["step"], _geometry_of(image))
