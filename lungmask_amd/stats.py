"""Per-label lung volume and density statistics (not in the reference: what users compute from a lung or lobe mask).

The device pass (`lm_label_stats_dev`, lungmask_amd/csrc/stats_kernels.hip) reads the label and intensity volumes once and returns
integer accumulators and a 4096-bin HU histogram per label.  Everything here follows exactly from those integers:

- HU value of a voxel: integer volumes hu = v; float volumes hu = rint(v) (round half to even), saturated to the int32 range.  NaN is
  counted in `nonfinite` and left out of every density figure; +-inf saturate like any other value.
- clip(hu, -1024, 3071) goes into the histogram (1-HU bins); `clipped_low` / `clipped_high` count the clipped values.  mean, std,
  percentiles and `below` use the clipped values; `hu_min` / `hu_max` the unclipped hu.
- mean = exact integer sum / N (one division); std (ddof 0) from the exact integers N * sum(x^2) - sum(x)^2; percentiles = numpy's
  default method="linear" on the two order statistics read from the cumulative histogram; below[t] = fraction of finite voxels
  with clipped value < t; volume_ml = voxels * prod(spacing) / 1000; centroid_index = index_sum / voxels in the array's axis
  order; centroid_mm = that point in LPS physical space (None without geometry); bbox = zmin, zmax, ymin, ymax, xmin, xmax with
  exclusive maxima (bbox_3D with margin 0).
- "lung" aggregates every label >= 1 (histograms summed, so it is exact as well).
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import numpy as np

from . import _native

HU_LO, HU_HI = -1024, 3071
MAX_LABELS = 16

# label names (reference README): R231 / R231CovidWeb 1 = right lung, 2 = left lung; LTRCLobes and the fused mode the five lobes
_LUNGS = {1: "right lung", 2: "left lung"}
_LOBES = {1: "left upper lobe", 2: "left lower lobe", 3: "right upper lobe", 4: "right middle lobe", 5: "right lower lobe"}
MODEL_LABEL_NAMES = {"R231": _LUNGS, "R231CovidWeb": _LUNGS, "LTRCLobes": _LOBES, "LTRCLobes_R231": _LOBES}


def label_names(modelname: Optional[str], n_labels: int) -> Dict[int, str]:
    """Names of labels 1 .. n_labels-1 for a model of the zoo; a checkpoint of its own ("label k")."""
    known = MODEL_LABEL_NAMES.get(modelname or "", {})
    return {k: known.get(k, f"label {k}") for k in range(1, n_labels)}


def _key(v: float) -> str:
    return f"{v:g}"


def _order_stat(cum: np.ndarray, k: int) -> int:
    """The k-th smallest (0-based) clipped value of a histogram with cumulative counts `cum`."""
    return int(np.searchsorted(cum, k, side="right")) + HU_LO


def _percentile(cum: np.ndarray, n: int, q: float) -> float:
    """np.percentile(values, q) (method="linear") from the cumulative histogram of the n values."""
    h = (n - 1) * (float(q) / 100.0)
    lo = math.floor(h)
    g = h - lo
    a = float(_order_stat(cum, lo))
    b = float(_order_stat(cum, min(lo + 1, n - 1)))
    d = b - a
    return b - d * (1.0 - g) if g >= 0.5 else a + d * g  # numpy's _lerp


def finalize_label(acc: dict, spacing=None, percentiles: Sequence[float] = (15,), thresholds: Sequence[float] = (-950,),
                   index_to_physical=None, name: Optional[str] = None) -> dict:
    """One label's entry from its accumulators: acc = voxels, nonfinite, clipped_low, clipped_high, hu_min, hu_max (ints),
    index_sum (3 ints, array order), bbox (6 ints) and hist (4096 counts, bin b = HU b - 1024).  `spacing` in array axis order
    (None: no volume); `index_to_physical(index in array order)` -> LPS point (None: no centroid_mm).  Empty labels report
    voxels 0 and None for every derived field; density fields are None when the label has no finite voxel."""
    vox = int(acc["voxels"])
    nonfinite = int(acc["nonfinite"])
    out = {"name": name, "voxels": vox, "nonfinite": nonfinite, "clipped_low": int(acc["clipped_low"]),
           "clipped_high": int(acc["clipped_high"]), "volume_ml": None, "hu_min": None, "hu_max": None, "mean": None, "std": None,
           "percentiles": {_key(q): None for q in percentiles}, "below": {_key(t): None for t in thresholds},
           "centroid_index": None, "centroid_mm": None, "bbox": None}
    if vox == 0:
        return out
    if spacing is not None:
        out["volume_ml"] = vox * float(np.prod(np.asarray(spacing, dtype=np.float64))) / 1000.0
    idx = [int(s) / vox for s in acc["index_sum"]]  # (Python int / int: correctly rounded)
    out["centroid_index"] = idx
    if index_to_physical is not None:
        out["centroid_mm"] = [float(v) for v in index_to_physical(idx)]
    out["bbox"] = [int(v) for v in acc["bbox"]]
    n = vox - nonfinite
    if n == 0:
        return out
    out["hu_min"], out["hu_max"] = int(acc["hu_min"]), int(acc["hu_max"])
    hist = np.asarray(acc["hist"], dtype=np.int64)
    vals = np.arange(HU_LO, HU_HI + 1, dtype=np.int64)
    s = sum(int(c) * int(v) for c, v in zip(hist[hist != 0], vals[hist != 0]))  # exact integers
    s2 = sum(int(c) * int(v) * int(v) for c, v in zip(hist[hist != 0], vals[hist != 0]))
    out["mean"] = s / n
    out["std"] = math.sqrt((n * s2 - s * s) / (n * n))
    cum = np.cumsum(hist)
    out["percentiles"] = {_key(q): _percentile(cum, n, q) for q in percentiles}
    below = {}
    for t in thresholds:
        b = min(max(math.ceil(t) - HU_LO, 0), hist.size)  # bins with value < t
        below[_key(t)] = int(cum[b - 1]) / n if b > 0 else 0.0
    out["below"] = below
    return out


def _aggregate(raw: dict, rows) -> dict:
    """The accumulators of the union of labels `rows` (non-empty ones only for the extremes and boxes)."""
    rows = [k for k in rows if raw["voxels"][k] > 0]
    acc = {f: int(sum(int(raw[f][k]) for k in rows)) for f in ("voxels", "nonfinite", "clipped_low", "clipped_high")}
    fin = [k for k in rows if raw["voxels"][k] > raw["nonfinite"][k]]
    acc["hu_min"] = min((int(raw["hu_min"][k]) for k in fin), default=0)
    acc["hu_max"] = max((int(raw["hu_max"][k]) for k in fin), default=0)
    acc["index_sum"] = [int(sum(int(raw["index_sum"][k][a]) for k in rows)) for a in range(3)]
    bb = [-1] * 6
    if rows:
        bb = [min(int(raw["bbox"][k][0]) for k in rows), max(int(raw["bbox"][k][1]) for k in rows),
              min(int(raw["bbox"][k][2]) for k in rows), max(int(raw["bbox"][k][3]) for k in rows),
              min(int(raw["bbox"][k][4]) for k in rows), max(int(raw["bbox"][k][5]) for k in rows)]
    acc["bbox"] = bb
    acc["hist"] = np.asarray(raw["hist"], dtype=np.int64)[rows].sum(axis=0) if rows else np.zeros(_native.STATS_BINS, np.int64)
    return acc


def finalize(raw: dict, spacing=None, percentiles: Sequence[float] = (15,), thresholds: Sequence[float] = (-950,),
             names: Optional[Dict[int, str]] = None, index_to_physical=None) -> dict:
    """The JSON-serialisable result of `label_statistics` from the raw output of `Engine.label_stats` / `label_stats_dev`."""
    n_labels = len(raw["voxels"])
    names = dict(names or {})
    spacing_l = None if spacing is None else [float(s) for s in spacing]
    labels = {"0": {"name": "background", "voxels": int(raw["voxels"][0])}}
    for k in range(1, n_labels):
        acc = {f: raw[f][k] for f in ("voxels", "nonfinite", "clipped_low", "clipped_high", "hu_min", "hu_max", "index_sum", "bbox")}
        acc["hist"] = raw["hist"][k]
        labels[str(k)] = finalize_label(acc, spacing_l, percentiles, thresholds, index_to_physical, names.get(k, f"label {k}"))
    lung = finalize_label(_aggregate(raw, range(1, n_labels)), spacing_l, percentiles, thresholds, index_to_physical, "lung")
    return {"spacing_mm": spacing_l, "voxel_volume_ml": None if spacing_l is None else float(np.prod(spacing_l)) / 1000.0,
            "hu_window": [HU_LO, HU_HI], "labels": labels, "lung": lung, "other_voxels": int(raw["other"])}


def geometry(image, spacing=None):
    """(array, spacing in array axis order or None, index_to_physical or None) of a numpy array, a volume_io.Volume or a SimpleITK
    image.  `spacing` may only be given for a numpy array: the images carry their own."""
    from . import volume_io

    if isinstance(image, np.ndarray):
        sp = None if spacing is None else tuple(float(s) for s in spacing)
        if sp is not None and len(sp) != image.ndim:
            raise ValueError(f"spacing needs one value per array axis ({image.ndim}), got {spacing!r}")
        return image, sp, None
    if spacing is not None:
        raise ValueError("spacing is taken from the image (Volume / SimpleITK image): do not pass it as well")
    if isinstance(image, volume_io.Volume):
        arr, sp_xyz, origin, direction = image.array, image.spacing, image.origin, image.direction
    else:
        import SimpleITK as sitk

        arr = sitk.GetArrayFromImage(image)
        sp_xyz, origin, direction = image.GetSpacing(), image.GetOrigin(), np.asarray(image.GetDirection(), np.float64).reshape(3, 3)
    o = np.asarray(origin, dtype=np.float64)
    d = np.asarray(direction, dtype=np.float64).reshape(3, 3)
    s = np.asarray(sp_xyz, dtype=np.float64)

    def to_physical(idx_zyx):  # Volume.index_to_physical: the index in (x, y, z) order
        return o + d @ (np.asarray(idx_zyx, dtype=np.float64)[::-1] * s)

    return arr, tuple(float(v) for v in sp_xyz[::-1]), to_physical


def _label_array(labels) -> np.ndarray:
    from . import volume_io

    if isinstance(labels, np.ndarray):
        return labels
    if isinstance(labels, volume_io.Volume):
        return labels.array
    import SimpleITK as sitk

    return sitk.GetArrayFromImage(labels)


def label_statistics(image, labels, spacing=None, percentiles: Sequence[float] = (15,), thresholds: Sequence[float] = (-950,),
                     names: Optional[Dict[int, str]] = None, engine=None, n_labels: Optional[int] = None) -> dict:
    """Volume and density statistics of every label of `labels` (u8-valued [n][h][w]: a mask from `apply`, from the reference or
    edited by hand) over `image` (numpy array, volume_io.Volume or SimpleITK image of the same shape), computed on the GPU.

    Returns a JSON-serialisable dict: spacing_mm (array axis order), voxel_volume_ml, hu_window, labels {"k": {...}} (label 0:
    voxels only), lung (every label >= 1 together) and other_voxels (labels >= n_labels).  `spacing`: numpy input only, in the
    array's axis order (None: volumes are None).  `names`: {k: name} (default "label k").  `n_labels` (1..16): labels counted
    (default: max(names) + 1, else the largest label present + 1, at most 16).  `engine`: a _native.Engine (default: a new one
    on device 0)."""
    from .mask import LMInferer

    arr, sp, to_phys = geometry(image, spacing)
    lab = np.ascontiguousarray(_label_array(labels))
    if lab.shape != arr.shape or lab.ndim != 3:
        raise ValueError(f"labels {lab.shape} and image {arr.shape} must be 3-D volumes of the same shape")
    if lab.dtype != np.uint8:
        if lab.size and (lab.min() < 0 or lab.max() > 255):
            raise ValueError("labels must lie in 0..255")
        lab = lab.astype(np.uint8)
    if n_labels is None:
        if names:
            n_labels = max(int(k) for k in names) + 1
        else:
            n_labels = (int(lab.max()) + 1) if lab.size else 1
        n_labels = max(1, min(n_labels, MAX_LABELS))
    vol = np.ascontiguousarray(LMInferer._engine_dtype(np.asarray(arr)))
    with _native.engine_scope(engine) as eng:
        raw = eng.label_stats(lab, vol, n_labels)
    return finalize(raw, sp, percentiles, thresholds, names or label_names(None, n_labels), to_phys)
