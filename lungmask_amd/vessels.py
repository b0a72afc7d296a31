"""Hessian, eigenvalues, Frangi vesselness and the pulmonary vessel analysis on the GPU (not in the reference: the multi-scale Hessian
filter callers run on the host, tens of seconds per CT with scipy).

The device passes (`lm_hessian_dev`, `lm_vesselness_dev`, `lm_vessel_counts_dev`, lungmask_amd/csrc/vessel_kernels.hip) follow the
definitions in include/lungmask_hip.h.  In short:

- Per scale sigma the six second derivatives of the Gaussian-smoothed image are `filters.gaussian(image, sigma, order=...)` bit for
  bit, computed in three fused passes instead of eighteen, and multiplied by sigma_a * sigma_b (sigmas in voxels of their axes: with
  a spacing this is sigma_mm^2 times the derivative per mm).
- The eigenvalues come from four cyclic Jacobi sweeps in float32 and are ordered |l1| <= |l2| <= |l3|.
- vesselness is Frangi's measure for bright tubes (`bright=False`: dark ones), the maximum over the scales; `scale` is the 1-based
  index of the scale that gave it.
- With `labels` only the voxels whose label is in `keep` (default: every label >= 1) are analysed -- the taps still see the whole
  volume, so the values there are the unmasked ones -- and every other voxel is 0.
- vessel_analysis thresholds the map inside the lung eroded by `erode_mm` (the pleural edge is a bright sheet next to the lung and
  takes no part) and counts vessel voxels per label and per scale.

The defaults c = 100 HU and threshold = 0.5 are conventional choices; nothing here validates them clinically.
Everything is in the caller's array orientation (no LPS re-orientation), as the statistics are.
"""
from __future__ import annotations

import math

import numpy as np

from . import _native
from . import filters as _filters

DEFAULT_SIGMAS_MM = (1.0, 1.5, 2.0, 3.0)
MAX_SCALES = _native.VESSEL_MAX_SCALES


def scale_sigmas(sigmas_mm, sp=None):
    """Per scale the three sigmas in voxels (array axis order) of `sigmas_mm` (one value or a sequence) with the spacing `sp`."""
    sig = [sigmas_mm] if np.ndim(sigmas_mm) == 0 else list(sigmas_mm)
    if not 1 <= len(sig) <= MAX_SCALES:
        raise ValueError(f"sigmas_mm: between 1 and {MAX_SCALES} scales, got {len(sig)}")
    for s in sig:
        if np.ndim(s) != 0 or not (float(s) > 0 and math.isfinite(float(s))):
            raise ValueError(f"sigmas_mm: every sigma must be one value > 0 and finite, got {s!r}")
    return [[float(s) / (sp[i] if sp is not None else 1.0) for i in range(3)] for s in sig]


def check_analysis_arguments(threshold, erode_mm):
    if not (float(threshold) > 0 and math.isfinite(float(threshold))):
        raise ValueError(f"threshold must be > 0 and finite, got {threshold!r}")
    if not (float(erode_mm) >= 0 and math.isfinite(float(erode_mm))):
        raise ValueError(f"erode_mm must be >= 0 and finite, got {erode_mm!r}")


def _no_voxel(arr, lab):
    if lab is not None and arr.shape[0] == 0:
        raise ValueError("vessels: the labels hold no voxel of the kept label values")


def hessian(image, sigma_mm, spacing=None, truncate: float = 4.0, labels=None, keep=None, eigenvalues: bool = False, engine=None):
    """float32 [6][n][h][w]: the scale-normalised Hessian of `image` (numpy array, `volume_io.Volume` or SimpleITK image) at the scale
    `sigma_mm` -- millimetres with a spacing (`spacing`: numpy input only, in the array's axis order; the images bring their own),
    voxels without -- in the order xx, yy, zz, xy, xz, yz (x = the last array axis).  With `eigenvalues` -> (components, float32
    [3][n][h][w]: the eigenvalues by ascending magnitude).  `truncate`: the taps reach int(truncate * sigma + 0.5) voxels, 32 at
    most.  With `labels` only the voxels whose label is in `keep` (None: every label >= 1) are analysed; the others are 0.
    ValueError when labels are given and nothing is selected.  `engine`: a _native.Engine (default: a new one on device 0)."""
    arr, lab, sp = _filters._inputs(image, labels, spacing)
    if np.ndim(sigma_mm) != 0:
        raise ValueError(f"sigma_mm: one scale, got {sigma_mm!r}")
    sig = scale_sigmas(sigma_mm, sp)[0]
    _native.Engine._vessel_params([sig], truncate, lab is not None, keep)
    _no_voxel(arr, lab)
    with _native.engine_scope(engine) as eng:
        return eng.hessian(arr, sig, lab, eigenvalues=eigenvalues, truncate=truncate, keep=keep)


def vesselness(image, sigmas_mm=DEFAULT_SIGMAS_MM, spacing=None, alpha: float = 0.5, beta: float = 0.5, c: float = 100.0, bright: bool = True,
               truncate: float = 4.0, labels=None, keep=None, return_scale: bool = False, engine=None):
    """float32 [n][h][w]: Frangi's vesselness of `image` (numpy array, `volume_io.Volume` or SimpleITK image), the maximum over the
    scales `sigmas_mm` (1 to 8; millimetres with a spacing, voxels without).  `alpha`, `beta`: the sensitivities to plate-like and
    blob-like structure; `c`: the structureness scale in the image's units (HU).  `bright=False` looks for dark tubes.  With
    `return_scale` -> (V, uint8 [n][h][w]: the 1-based index of the scale that gave V, 0 where V == 0).  With `labels` only the
    voxels whose label is in `keep` (None: every label >= 1) are analysed; the others are 0.  ValueError when labels are given and
    nothing is selected.  `engine`: a _native.Engine (default: a new one on device 0)."""
    arr, lab, sp = _filters._inputs(image, labels, spacing)
    sig = scale_sigmas(sigmas_mm, sp)
    kw = dict(alpha=alpha, beta=beta, c=c, bright=bright, truncate=truncate, keep=keep)
    _native.Engine._vessel_params(sig, truncate, lab is not None, keep, alpha, beta, c, bright)
    _no_voxel(arr, lab)
    with _native.engine_scope(engine) as eng:
        return eng.vesselness(arr, sig, lab, return_scale=return_scale, **kw)


def _entry(name, voxels, by_scale, voxel_ml):
    out = {"name": name, "voxels": int(voxels), "vessel_voxels": None, "vessel_ml": None, "fraction": None, "by_scale": None}
    if int(voxels) == 0:
        return out
    vessel = int(np.sum(by_scale))
    out["vessel_voxels"] = vessel
    out["vessel_ml"] = None if voxel_ml is None else vessel * voxel_ml
    out["fraction"] = vessel / int(voxels)
    out["by_scale"] = [int(v) for v in by_scale[1:]]
    return out


def finalize_analysis(counts, totals, sigmas_mm, threshold, erode_mm, spacing=None, names=None, params=None) -> dict:
    """The analysis dict from lm_vessel_counts_dev's tables: `counts` at the threshold, `totals` at -inf (every voxel of the eroded
    labels), both int64 [n_labels][9]."""
    names = dict(names or {})
    sig = [float(s) for s in ([sigmas_mm] if np.ndim(sigmas_mm) == 0 else sigmas_mm)]
    sp = None if spacing is None else [float(s) for s in spacing]
    voxel_ml = None if sp is None else float(np.prod(sp)) / 1000.0
    counts, totals = np.asarray(counts, np.int64)[:, :len(sig) + 1], np.asarray(totals, np.int64).sum(axis=1)
    ks = sorted({int(k) for k in names} | {int(k) for k in np.flatnonzero(totals[1:]) + 1})
    labels = {str(k): _entry(names.get(k, f"label {k}"), totals[k] if k < totals.size else 0,
                             counts[k] if k < totals.size else counts[0] * 0, voxel_ml) for k in ks}
    out = {"sigmas_mm": sig, "threshold": float(threshold), "erode_mm": float(erode_mm), "spacing_mm": sp, "voxel_volume_ml": voxel_ml}
    out.update(params or {})
    out["labels"] = labels
    out["lung"] = _entry("lung", totals[1:].sum(), counts[1:].sum(axis=0), voxel_ml)
    return out


def empty_analysis(sigmas_mm, threshold, erode_mm, spacing=None, names=None, params=None) -> dict:
    """The analysis of labels without a voxel."""
    zeros = np.zeros((16, _native.VESSEL_COUNT_COLUMNS), np.int64)
    return finalize_analysis(zeros, zeros, sigmas_mm, threshold, erode_mm, spacing, names, params)


def analysis_dev(eng, vol_dev, lab_dev, sigmas_mm=DEFAULT_SIGMAS_MM, threshold=0.5, erode_mm=2.0, spacing=None, names=None, alpha=0.5,
                 beta=0.5, c=100.0, bright=True, truncate=4.0):
    """The vessel analysis on device-resident arrays -> (V DeviceArray, scale DeviceArray, eroded labels DeviceArray, analysis dict).
    The caller owns the three arrays.  NoKeptVoxel when nothing is labelled."""
    sig = scale_sigmas(sigmas_mm, spacing)
    params = {"alpha": float(alpha), "beta": float(beta), "c": float(c), "bright": bool(bright)}
    v, sc = eng.vesselness_dev(vol_dev, sig, alpha, beta, c, bright, truncate, lab=lab_dev, return_scale=True)
    eroded = None
    try:
        eroded = eng.morph_dev(lab_dev, "erode", float(erode_mm), spacing=spacing)[0]
        counts = eng.vessel_counts_dev(v, sc, eroded, threshold)
        totals = eng.vessel_counts_dev(v, sc, eroded, -math.inf)
    except BaseException:
        for d in (v, sc, eroded):
            if d is not None:
                d.free()
        raise
    return v, sc, eroded, finalize_analysis(counts, totals, sigmas_mm, threshold, erode_mm, spacing, names, params)


def vessel_analysis(image, labels, sigmas_mm=DEFAULT_SIGMAS_MM, threshold: float = 0.5, erode_mm: float = 2.0, spacing=None, names=None,
                    engine=None) -> dict:
    """The pulmonary vessel analysis of `labels` over `image`, computed on the GPU -> a JSON-serialisable dict: sigmas_mm, threshold,
    erode_mm, spacing_mm, voxel_volume_ml, alpha, beta, c, bright, labels {"k": entry} and lung (every label >= 1 together).  An
    entry: name, voxels (of the label inside the lung eroded by `erode_mm`: every label >= 1 together is eroded by a ball, so borders
    between lobes stay), vessel_voxels (those with vesselness >= threshold), vessel_ml, fraction (vessel_voxels / voxels) and
    by_scale (vessel voxels per scale of `sigmas_mm`: small sigmas are small vessels).  The vesselness is `vesselness(image,
    sigmas_mm, labels=labels)`.  Labels without a voxel report None for every derived field."""
    if labels is None:
        raise ValueError("vessel_analysis needs labels")
    check_analysis_arguments(threshold, erode_mm)
    arr, lab, sp = _filters._inputs(image, labels, spacing)
    _native.Engine._vessel_params(scale_sigmas(sigmas_mm, sp), 4.0, True)
    if arr.size == 0 or not lab.any():
        return empty_analysis(sigmas_mm, threshold, erode_mm, sp, names, {"alpha": 0.5, "beta": 0.5, "c": 100.0, "bright": True})
    with _native.engine_scope(engine) as eng, eng.scope() as dev:
        v, sc, eroded, analysis = analysis_dev(eng, dev.upload(arr), dev.upload(lab), sigmas_mm, threshold, erode_mm, sp, names)
        dev.add(v, sc, eroded)
        return analysis


class VesselResult:
    """What `LMInferer.apply_with_vessels` and `vessel_result` return: `vesselness` float32 [n][h][w], `scale` uint8 [n][h][w] (the
    1-based index into `analysis["sigmas_mm"]` of the scale that gave the value, 0 where it is 0), `mask` bool [n][h][w]
    (vesselness >= threshold inside the eroded lung) and `analysis` (the dict of `vessel_analysis`)."""

    def __init__(self, vesselness, scale, mask, analysis):
        self.vesselness, self.scale, self.mask, self.analysis = vesselness, scale, mask, analysis


def empty_result(shape, sigmas_mm, threshold, erode_mm, spacing=None, names=None, params=None) -> VesselResult:
    """Nothing is labelled: zeros and an analysis of empties."""
    return VesselResult(np.zeros(shape, np.float32), np.zeros(shape, np.uint8), np.zeros(shape, bool),
                        empty_analysis(sigmas_mm, threshold, erode_mm, spacing, names, params))


def result_dev(eng, vol_dev, lab_dev, sigmas_mm=DEFAULT_SIGMAS_MM, threshold=0.5, erode_mm=2.0, spacing=None, names=None, alpha=0.5,
               beta=0.5, c=100.0, bright=True) -> VesselResult:
    """`analysis_dev` and the three volumes brought to the host.  NoKeptVoxel when nothing is labelled."""
    v, sc, eroded, analysis = analysis_dev(eng, vol_dev, lab_dev, sigmas_mm, threshold, erode_mm, spacing, names, alpha, beta, c, bright)
    with eng.scope() as dev:
        dev.add(v, sc, eroded)
        eng.sync()
        V = v.download()
        return VesselResult(V, sc.download(), (V >= np.float32(threshold)) & (eroded.download() > 0), analysis)


def vessel_result(image, labels, sigmas_mm=DEFAULT_SIGMAS_MM, threshold: float = 0.5, erode_mm: float = 2.0, spacing=None, names=None,
                  alpha: float = 0.5, beta: float = 0.5, c: float = 100.0, bright: bool = True, engine=None) -> VesselResult:
    """The vesselness map of the labelled voxels, its scale index, the vessel mask and `vessel_analysis`'s dict in one pass over
    `image` and `labels` (what `LMInferer.apply_with_vessels` returns beside the labels)."""
    if labels is None:
        raise ValueError("vessel_result needs labels")
    check_analysis_arguments(threshold, erode_mm)
    arr, lab, sp = _filters._inputs(image, labels, spacing)
    _native.Engine._vessel_params(scale_sigmas(sigmas_mm, sp), 4.0, True, None, alpha, beta, c, bright)
    params = {"alpha": float(alpha), "beta": float(beta), "c": float(c), "bright": bool(bright)}
    if arr.size == 0 or not lab.any():
        return empty_result(arr.shape, sigmas_mm, threshold, erode_mm, sp, names, params)
    with _native.engine_scope(engine) as eng, eng.scope() as dev:
        return result_dev(eng, dev.upload(arr), dev.upload(lab), sigmas_mm, threshold, erode_mm, sp, names, alpha, beta, c, bright)
