"""Label agreement metrics (not in the reference): Dice, Jaccard, Hausdorff distance and surface distances between two label
volumes, and the exact Euclidean distance transform they are built on.

The device passes (`lm_edt_dev`, `lm_label_agreement_dev`, lungmask_amd/csrc/metrics_kernels.hip) return integers, exact float32
squared distances and float64 sums; everything here follows from those:

- Row k compares A = (a == k) with B = (b == k); "lung" compares (a >= 1) with (b >= 1), whatever the label values.
- dice = 2 I / (Va + Vb); jaccard = I / (Va + Vb - I); volumes in mL from the spacing; volume_difference_ml = a - b;
  relative_volume_difference = (Va - Vb) / Vb.
- Surface voxel: a voxel of the label with at least one of its 6 face neighbours outside the label or outside the volume
  (medpy's A ^ binary_erosion(A) with connectivity 1).  a -> b: the distances from the surface voxels of A to the nearest surface
  voxel of B (in mm with a spacing, else in voxels).
- hausdorff = the largest distance of both directions; mean_a_to_b / mean_b_to_a = the directional means (medpy's assd is their
  average); assd = (sum a->b + sum b->a) / (Sa + Sb), the POOLED mean; percentiles[q] = numpy's method="linear" percentile of the
  a -> b list, the b -> a list and the two lists pooled (pooled 95 = medpy's hd95), interpolated in float64 between the square
  roots of the two order statistics the device selects.
- None where a value is undefined: overlap ratios 0 / 0, every distance field when either surface is empty,
  relative_volume_difference when Vb = 0, volumes without a spacing.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import numpy as np

from . import _native
from .stats import MAX_LABELS, _key, geometry, label_names


def _lerp_percentile(lo: float, hi: float, count: int, q: float) -> float:
    """numpy's method="linear" percentile from its two neighbouring order statistics (stats._percentile's formula)."""
    h = (count - 1) * (float(q) / 100.0)
    g = h - math.floor(h)
    d = hi - lo
    return hi - d * (1.0 - g) if g >= 0.5 else lo + d * g


def finalize_row(row: dict, percentiles: Sequence[float], spacing=None, name: Optional[str] = None) -> dict:
    """One row of `compare_labels` from its raw fields: voxels_a, voxels_b, intersection, surface_a, surface_b (ints), bbox (6
    ints), max_d2_ab, max_d2_ba, sum_d_ab, sum_d_ba, order_ab / order_ba / order_pooled ([len(percentiles)][2] squared distances)."""
    va, vb, inter = int(row["voxels_a"]), int(row["voxels_b"]), int(row["intersection"])
    sa, sb = int(row["surface_a"]), int(row["surface_b"])
    vox_ml = None if spacing is None else float(np.prod(np.asarray(spacing, dtype=np.float64))) / 1000.0
    out = {"name": name, "voxels_a": va, "voxels_b": vb, "intersection": inter,
           "volume_a_ml": None if vox_ml is None else va * vox_ml, "volume_b_ml": None if vox_ml is None else vb * vox_ml,
           "volume_difference_ml": None if vox_ml is None else (va - vb) * vox_ml,
           "relative_volume_difference": (va - vb) / vb if vb else None,
           "surface_voxels_a": sa, "surface_voxels_b": sb, "bbox": [int(v) for v in row["bbox"]] if va + vb else None,
           "dice": 2 * inter / (va + vb) if va + vb else None, "jaccard": inter / (va + vb - inter) if va + vb else None,
           "hausdorff": None, "mean_a_to_b": None, "mean_b_to_a": None, "assd": None,
           "percentiles": {_key(q): {"a_to_b": None, "b_to_a": None, "pooled": None} for q in percentiles}}
    if sa == 0 or sb == 0:
        return out
    out["hausdorff"] = math.sqrt(max(float(row["max_d2_ab"]), float(row["max_d2_ba"])))
    sum_ab, sum_ba = float(row["sum_d_ab"]), float(row["sum_d_ba"])
    out["mean_a_to_b"], out["mean_b_to_a"] = sum_ab / sa, sum_ba / sb
    out["assd"] = (sum_ab + sum_ba) / (sa + sb)
    for i, q in enumerate(percentiles):
        entry = {}
        for key, field, count in (("a_to_b", "order_ab", sa), ("b_to_a", "order_ba", sb), ("pooled", "order_pooled", sa + sb)):
            lo, hi = (math.sqrt(float(v)) for v in row[field][i])
            entry[key] = _lerp_percentile(lo, hi, count, q)
        out["percentiles"][_key(q)] = entry
    return out


_ROW_FIELDS = ("voxels_a", "voxels_b", "intersection", "surface_a", "surface_b", "bbox", "max_d2_ab", "max_d2_ba", "sum_d_ab", "sum_d_ba",
               "order_ab", "order_ba", "order_pooled")


def finalize(raw: dict, spacing=None, names: Optional[Dict[int, str]] = None) -> dict:
    """The JSON-serialisable result of `compare_labels` from the raw output of `Engine.label_agreement` / `label_agreement_dev`."""
    n_labels = len(raw["voxels_a"])
    names = dict(names or {})
    qs = list(raw["percentiles"])
    spacing_l = None if spacing is None else [float(s) for s in spacing]
    rows = [finalize_row({f: raw[f][k] for f in _ROW_FIELDS}, qs, spacing_l, "lung" if k == 0 else names.get(k, f"label {k}"))
            for k in range(n_labels)]
    return {"spacing_mm": spacing_l, "unit": "voxel" if spacing_l is None else "mm", "labels": {str(k): rows[k] for k in range(1, n_labels)},
            "lung": rows[0], "other_voxels_a": int(raw["other_a"]), "other_voxels_b": int(raw["other_b"])}


def _direction(image):
    from . import volume_io

    if isinstance(image, np.ndarray):
        return None
    if isinstance(image, volume_io.Volume):
        return np.asarray(image.direction, np.float64).reshape(3, 3)
    return np.asarray(image.GetDirection(), np.float64).reshape(3, 3)


def _u8(arr: np.ndarray, what: str) -> np.ndarray:
    arr = np.asarray(arr)
    if arr.ndim != 3:
        raise ValueError(f"{what} must be a 3-D volume (got shape {arr.shape})")
    if arr.dtype == np.uint8:
        return np.ascontiguousarray(arr)
    if arr.dtype.kind not in "iub":
        raise ValueError(f"{what} must be an integer label volume (got {arr.dtype})")
    if arr.size and (arr.min() < 0 or arr.max() > 255):
        raise ValueError(f"{what}: labels must lie in 0..255")
    return np.ascontiguousarray(arr.astype(np.uint8))


def label_inputs(a, b, spacing=None):
    """(a u8, b u8, spacing in array axis order or None) of two label volumes (numpy integer arrays, volume_io.Volumes or SimpleITK
    images) after the checks of `compare_labels`."""
    arr_a, sp_a, _ = geometry(a, None if not isinstance(a, np.ndarray) else spacing)
    arr_b, sp_b, _ = geometry(b, None if not isinstance(b, np.ndarray) else spacing)
    carried = [not isinstance(v, np.ndarray) for v in (a, b)]
    if spacing is not None and any(carried):
        raise ValueError("spacing is taken from the image (Volume / SimpleITK image): do not pass it as well")
    la, lb = _u8(arr_a, "a"), _u8(arr_b, "b")
    if la.shape != lb.shape:
        raise ValueError(f"a {la.shape} and b {lb.shape} must have the same shape")
    if all(carried):
        if not np.allclose(sp_a, sp_b, rtol=1e-5) or not np.allclose(_direction(a), _direction(b), rtol=1e-5):
            raise ValueError(f"a and b disagree in geometry: spacing {sp_a} / {sp_b}, direction {_direction(a).tolist()} / "
                             f"{_direction(b).tolist()}")
    sp = sp_a if carried[0] else sp_b
    return la, lb, sp


def compare_labels(a, b, spacing=None, n_labels: Optional[int] = None, percentiles: Sequence[float] = (95,),
                   names: Optional[Dict[int, str]] = None, engine=None, resample_b: bool = False, transform=None) -> dict:
    """Agreement of two label volumes of the same shape (numpy integer arrays, volume_io.Volumes or SimpleITK images; e.g. a result
    and a ground truth), computed on the GPU.

    Returns a JSON-serialisable dict: spacing_mm (array axis order), unit ("mm", or "voxel" without a spacing), labels {"k": row},
    lung (every label >= 1 together), other_voxels_a / other_voxels_b (labels >= n_labels).  A row holds name, voxels_a, voxels_b,
    intersection, volume_a_ml, volume_b_ml, volume_difference_ml, relative_volume_difference, surface_voxels_a, surface_voxels_b,
    bbox, dice, jaccard, hausdorff, mean_a_to_b, mean_b_to_a, assd and percentiles {"q": {a_to_b, b_to_a, pooled}} (the module
    docstring has the definitions).  `spacing`: numpy inputs only, in the array's axis order.  `n_labels` (1..16): default the
    largest label of both + 1, at most 16.  `names`: {k: name} (default "label k").  `engine`: a _native.Engine (default: a new one
    on device 0).  `resample_b`: a `b` whose grid (shape, spacing, origin, direction) differs from `a`'s -- both carrying geometry --
    is first resampled onto `a`'s grid with nearest neighbour (lungmask_amd.resample; fill 0); without it such a pair is refused.
    `transform` (with `resample_b`): the `resample.Affine` from `a`'s space to `b`'s that this resampling applies, e.g. the
    `transform` of a `registration.Registration` of `b`'s image onto `a`'s -- `b` is then resampled even onto an equal grid."""
    if transform is not None and not resample_b:
        raise ValueError("compare_labels: transform= is applied by the resampling of b and needs resample_b=True")
    if resample_b:
        b = _onto_grid_of(a, b, engine, transform)
    la, lb, sp = label_inputs(a, b, spacing)
    if n_labels is None:
        n_labels = min(max(int(la.max()) if la.size else 0, int(lb.max()) if lb.size else 0) + 1, MAX_LABELS)
    n_labels = int(n_labels)
    with _native.engine_scope(engine) as eng:
        raw = eng.label_agreement(la, lb, n_labels, sp, percentiles)
    return finalize(raw, sp, names or label_names(None, n_labels))


def _onto_grid_of(a, b, engine=None, transform=None):
    """`b` resampled (nearest neighbour) onto the grid of `a` when both carry geometry and their grids differ, or under `transform`
    (from `a`'s space to `b`'s); else `b` itself."""
    from . import resample as rs

    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        if transform is not None:
            raise ValueError("compare_labels: transform= needs two inputs with geometry (Volumes or SimpleITK images)")
        return b
    grid_a, grid_b = rs.Grid.of(a), rs.Grid.of(b)
    if transform is None and grid_a.same_as(grid_b):
        return b
    return rs.resample_labels(b, grid_a, transform, mode="nearest", fill=0, engine=engine)


def distance_transform(features, spacing=None, squared: bool = False, engine=None) -> np.ndarray:
    """float32 [n][h][w]: the Euclidean distance of every voxel to the nearest non-zero voxel of `features` (3-D numpy array),
    i.e. scipy.ndimage.distance_transform_edt(features == 0, sampling=spacing), computed on the GPU.  `squared`: the squared
    distance d2 exactly as lm_edt_dev defines it in float32; otherwise its float32 square root.  +inf without any feature."""
    feat = np.asarray(features)
    if feat.ndim != 3:
        raise ValueError(f"features must be a 3-D volume (got shape {feat.shape})")
    if spacing is not None and len(tuple(spacing)) != 3:
        raise ValueError(f"spacing needs one value per array axis (3), got {spacing!r}")
    with _native.engine_scope(engine) as eng:
        d2 = eng.edt(feat, spacing)
    return d2 if squared else np.sqrt(d2)
