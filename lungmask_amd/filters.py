"""Lung-aware image filters on the GPU: median, Gaussian (and its derivatives) and the low-attenuation map (not in the reference: what
callers run `scipy.ndimage.median_filter` / `gaussian_filter` on the host for, between two device stages).

The device pass (`lm_filter_dev`, lungmask_amd/csrc/filter_kernels.hip) follows the definitions in include/lungmask_hip.h.  In short:

- Without `labels` a filter sees the whole volume, indices clamped at the border (scipy's mode="nearest").
- With `labels` it is confined to the selection -- the voxels whose label is in `keep` (default: every label >= 1): the window or the
  taps see selected voxels only, nothing exists outside the volume, and chest wall and mediastinum never leak across the pleura.  A
  voxel that is not selected keeps its value, or takes `fill`.
- median: the element of rank (cnt - 1) // 2 of the cnt non-NaN values of the window (the lower median when cnt is even; -0.0 sorts
  before +0.0; cnt == 0 gives NaN).  The result is one of the input values, so integer results are exact.
- gaussian: three float32 passes along x, y, z, each `acc = 0; for k = -r..r: acc = fl32(acc + fl32(in[i + k] * w[k]))`; the masked
  form is the normalised convolution num / den of the masked image and the mask (order 0 only).
- low_attenuation_map: the masked Gaussian of the indicator "hu < threshold" (or hu inside `hu_range`): per lung voxel the
  Gaussian-weighted share of its lung neighbourhood that is low attenuation -- the spatial companion of the statistics' below[-950]
  and of `components.cluster_analysis`, with the same HU value and selection rule.

Everything is in the caller's array orientation (no LPS re-orientation), as the statistics are.
"""
from __future__ import annotations

import math

import numpy as np

from . import _native
from . import stats as _stats

MAX_RADIUS = _native.FILTER_MAX_RADIUS


def gaussian_taps(sigma_vox: float, order: int = 0, truncate: float = 4.0) -> np.ndarray:
    """float32 [2 r + 1]: the taps of a Gaussian of `sigma_vox` voxels, r = int(truncate * sigma_vox + 0.5), tap k - r at index k.
    phi(k) = exp(-k^2 / (2 s^2)) normalised to sum 1 in float64; order 1: (k / s^2) phi(k); order 2: (k^2 / s^4 - 1 / s^2) phi(k)
    (scipy.ndimage's kernels as correlation weights); cast to float32 at the end.  sigma 0 gives [1.0], for order 0 only."""
    s = float(sigma_vox)
    if order not in (0, 1, 2):
        raise ValueError(f"order: 0, 1 or 2, got {order!r}")
    if not (s >= 0 and math.isfinite(s)) or not (float(truncate) > 0 and math.isfinite(float(truncate))):
        raise ValueError(f"sigma must be >= 0 and truncate > 0, both finite (got {sigma_vox!r}, {truncate!r})")
    if s == 0:
        if order != 0:
            raise ValueError("a derivative (order 1 or 2) needs sigma > 0")
        return np.ones(1, np.float32)
    r = int(float(truncate) * s + 0.5)
    if r > MAX_RADIUS:
        raise ValueError(f"sigma {s:g} voxels with truncate {truncate:g} needs a tap radius of {r}: the limit is {MAX_RADIUS} "
                         f"(lower sigma or truncate)")
    k = np.arange(-r, r + 1, dtype=np.float64)
    phi = np.exp(-(k * k) / (2.0 * s * s))
    phi /= phi.sum()
    if order == 1:
        phi = (k / (s * s)) * phi
    elif order == 2:
        phi = ((k * k) / (s ** 4) - 1.0 / (s * s)) * phi
    return phi.astype(np.float32)


def _three(v, name):
    out = [v] * 3 if np.ndim(v) == 0 else list(v)
    if len(out) != 3:
        raise ValueError(f"{name}: one value or three in the array's axis order, got {v!r}")
    return out


def _inputs(image, labels, spacing):
    """(image array in an engine dtype, labels u8 or None, spacing in array axis order or None)."""
    from .mask import LMInferer

    arr, sp, _ = _stats.geometry(image, spacing)
    arr = np.asarray(arr)
    if arr.ndim != 3:
        raise ValueError(f"the image must be a 3-D volume (got shape {arr.shape})")
    if sp is not None and not all(v > 0 and math.isfinite(v) for v in sp):
        raise ValueError(f"spacing needs three positive values in the array's axis order, got {sp!r}")
    arr = np.ascontiguousarray(LMInferer._engine_dtype(arr))
    lab = None
    if labels is not None:
        lab = np.ascontiguousarray(_stats._label_array(labels))
        if lab.shape != arr.shape:
            raise ValueError(f"labels {lab.shape} and image {arr.shape} must be 3-D volumes of the same shape")
        if lab.dtype.kind not in "iub":
            raise ValueError(f"labels must be an integer label volume (got {lab.dtype})")
        if lab.dtype != np.uint8:
            if lab.size and (lab.min() < 0 or lab.max() > 255):
                raise ValueError("labels must lie in 0..255")
            lab = lab.astype(np.uint8)
    return arr, lab, sp


def _run(engine, arr, lab, **kw):
    if arr.shape[0] == 0 and lab is not None:
        raise ValueError("filter: the labels hold no voxel of the kept label values")
    with _native.engine_scope(engine) as eng:
        return eng.filter(arr, lab, **kw)


def separable_taps(sigma_mm, sp, order=0, truncate=4.0):
    """The three tap arrays (array axis order) of a Gaussian of `sigma_mm` (one value or three; voxels without a spacing `sp`)."""
    sig, orders = _three(sigma_mm, "sigma_mm"), _three(order, "order")
    return [gaussian_taps(float(sig[i]) / (sp[i] if sp is not None else 1.0), orders[i], truncate) for i in range(3)]


def gaussian(image, sigma_mm, spacing=None, order=0, truncate: float = 4.0, labels=None, keep=None, fill=None, engine=None) -> np.ndarray:
    """float32 [n][h][w]: `image` (numpy array, `volume_io.Volume` or SimpleITK image) smoothed by a Gaussian of `sigma_mm` -- one
    value or three in the array's axis order; millimetres with a spacing (`spacing`: numpy input only, in the array's axis order; the
    images bring their own), voxels without.  `order` (0, 1 or 2, one value or three): the derivative per axis.  `truncate`: the taps
    reach int(truncate * sigma + 0.5) voxels, 32 at most.  With `labels` the filter is confined to the voxels whose label is in
    `keep` (None: every label >= 1) as a normalised convolution (order 0 only); the other voxels keep their value or take `fill`.
    ValueError when labels are given and nothing is selected.  `engine`: a _native.Engine (default: a new one on device 0)."""
    arr, lab, sp = _inputs(image, labels, spacing)
    taps = separable_taps(sigma_mm, sp, order, truncate)
    if lab is not None and any(o != 0 for o in _three(order, "order")):
        raise ValueError("the masked Gaussian (labels=...) takes order 0 only")
    _native.Engine._filter_params("separable", taps=taps, masked=lab is not None, keep=keep, fill=fill)
    return _run(engine, arr, lab, kind="separable", taps=taps, keep=keep, fill=fill)


def _median_array(arr: np.ndarray) -> np.ndarray:
    """The image in a dtype the median kernel takes: int64 whose values fit int32 is narrowed."""
    if arr.dtype == np.int64:
        if arr.size and (arr.min() < -2 ** 31 or arr.max() >= 2 ** 31):
            raise ValueError("median: integer values beyond the int32 range; cast the image to float32 first")
        return arr.astype(np.int32)
    if arr.dtype == np.float64:
        raise ValueError("median: float64 is not supported; cast the image to float32 first (image.astype(np.float32))")
    return arr


def median(image, size=3, labels=None, keep=None, fill=None, engine=None) -> np.ndarray:
    """[n][h][w] of the input's dtype: the median of a `size` window (1, 3 or 5; one value or three in the array's axis order) around
    every voxel of `image` (numpy array, `volume_io.Volume` or SimpleITK image; integers up to the int32 range or float32).  With
    `labels` the window holds only voxels whose label is in `keep` (None: every label >= 1); the other voxels keep their value or
    take `fill`.  Windows with an even number of values give the lower median.  ValueError when labels are given and nothing is
    selected.  `engine`: a _native.Engine (default: a new one on device 0)."""
    src = np.asarray(_stats.geometry(image, None)[0])
    arr, lab, _ = _inputs(image, labels, None)
    arr = _median_array(arr)
    if fill is not None and src.dtype.kind in "iub" and (int(fill) != fill or not np.iinfo(src.dtype).min <= int(fill) <= np.iinfo(src.dtype).max):
        raise ValueError(f"fill {fill!r} is not a value of the image's dtype {src.dtype}")
    _native.Engine._filter_params("median", size=size, masked=lab is not None, keep=keep, fill=fill)
    out = _run(engine, arr, lab, kind="median", size=size, keep=keep, fill=fill)
    return out if out.dtype == src.dtype else out.astype(src.dtype)


def low_attenuation_map(image, labels, threshold=-950, hu_range=None, sigma_mm=5.0, spacing=None, keep=None, engine=None) -> np.ndarray:
    """float32 [n][h][w]: inside the lung (labels in `keep`; None: every label >= 1) the Gaussian-weighted (`sigma_mm`, one value or
    three) local fraction of lung voxels with hu < threshold (or inside `hu_range` = (lo, hi), inclusive, either None for open: the
    rule of `components.cluster_range`); 0 outside the lung.  Only lung voxels are counted, in numerator and denominator.  The HU
    value of a voxel is the statistics': integers as they are, floats rounded half to even; NaN counts as not low."""
    from . import components as cp

    rng = cp.cluster_range(threshold, hu_range)
    cp.check_arguments(rng, keep, 6)
    if labels is None:
        raise ValueError("low_attenuation_map needs labels")
    arr, lab, sp = _inputs(image, labels, spacing)
    taps = separable_taps(sigma_mm, sp)
    return _run(engine, arr, lab, kind="separable", taps=taps, keep=keep, fill=0.0, indicator=rng)
