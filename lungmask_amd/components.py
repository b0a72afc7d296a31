"""Connected components of a selection inside the labels, their table, and the low-attenuation cluster analysis built on them (not in
the reference: what users run scipy.ndimage.label and find_objects on the finished mask for).

The device does the voxel work (`lm_components_dev`, `lm_component_table_dev`, `lm_relabel_dev`; lungmask_amd/csrc/component_kernels.hip
and the engine's union-find labelling); include/lungmask_hip.h has the definitions.  In short, all in integers:

- HU value of a voxel: `lm_label_stats_dev`'s -- integers as they are, floats rint (half to even) saturated to int32, NaN nonfinite.
- A voxel is selected iff its label is in `keep` (default: every label >= 1) and, with an image, it is not nonfinite and its HU value
  lies in `hu_range` = (lo, hi), inclusive, either bound None for open.
- Selected voxels are connected when they are 6-adjacent (`connectivity=6`, scipy.ndimage.label's default) or 26-adjacent
  (`connectivity=26`) and, with `per_label=True`, carry the same label: components then never cross a label border.
- `ids`: 0 where unselected, otherwise 1 .. count, numbered by the raster index of each component's first voxel (for a binary selection:
  scipy.ndimage.label's numbering with the matching structure).
- Table row of a component: label (of its first voxel), voxels, first (raster index of the first voxel), bbox (zmin, zmax, ymin, ymax,
  xmin, xmax, exclusive maxima), index_sum, hu_sum / hu_min / hu_max (None without an image), faces = per axis z, y, x the number of
  voxel faces normal to it that bound the component (the other side is outside the volume or not in the component).
- Derived on the host in float64: centroid_index = index_sum / voxels, centroid_mm (LPS, as in lungmask_amd.stats), volume_ml =
  voxels * prod(spacing) / 1000, surface_area_mm2 = faces_z * sy * sx + faces_y * sz * sx + faces_x * sz * sy (the area of the
  voxel-face surface: it does not converge to the smooth surface's area), mean_hu = hu_sum / voxels, equivalent_diameter_mm =
  (6 V / pi)^(1/3) with V in mm^3.  The mm figures are None without a spacing.
- Limits: every dimension <= 4096, fewer than 2^31 voxels.

`cluster_analysis` summarises the clusters of low-attenuation voxels (`hu < threshold`, default -950: the voxels `below[-950]` of the
statistics counts) per label and for the whole lung: count, largest, mean, median, the histogram of sizes in powers of two, and D, the
cumulative cluster-size exponent of the low-attenuation-area literature (Mishima et al., PNAS 1999): with Y(s) the number of clusters
of at least s voxels, minus the least-squares slope of log10 Y(s) against log10 s over the distinct cluster sizes s.  A small D means
that large clusters take a large share -- many specks and one bulla of the same total volume differ in D, not in the emphysema index.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np

from . import _native
from . import stats as _stats

RAW_FIELDS = ("label", "voxels", "first", "bbox", "index_sum", "hu_sum", "hu_min", "hu_max", "faces")


def check_arguments(hu_range, keep, connectivity, min_voxels=1, order="raster", has_image=True):
    """ValueError for arguments that no call accepts (before anything is copied to a device)."""
    _native.Engine._components_params(hu_range, keep, True, connectivity, has_image)
    if int(min_voxels) != min_voxels or min_voxels < 1:
        raise ValueError(f"min_voxels: an integer >= 1, got {min_voxels!r}")
    if order not in ("raster", "size"):
        raise ValueError(f"order: 'raster' or 'size', got {order!r}")


def _volumes(image, labels, spacing):
    """(image array in an engine dtype or None, labels u8, spacing or None, index_to_physical or None)."""
    from .mask import LMInferer

    if image is None:
        lab_arr, sp, to_phys = _stats.geometry(labels, spacing)
        arr = None
    else:
        arr, sp, to_phys = _stats.geometry(image, spacing)
        lab_arr = _stats._label_array(labels)
    lab = np.ascontiguousarray(lab_arr)
    if lab.ndim != 3 or (arr is not None and tuple(arr.shape) != lab.shape):
        raise ValueError(f"labels {lab.shape} and image {None if arr is None else tuple(arr.shape)} must be 3-D volumes of the same shape")
    if lab.dtype != np.uint8:
        if lab.size and (lab.min() < 0 or lab.max() > 255):
            raise ValueError("labels must lie in 0..255")
        lab = lab.astype(np.uint8)
    if arr is not None:
        arr = np.ascontiguousarray(LMInferer._engine_dtype(np.asarray(arr)))
        if arr.dtype in (np.uint8, np.uint16):  # (what apply takes as well; the component kernels read the signed types)
            arr = arr.astype(np.int32)
    return arr, lab, sp, to_phys


def renumbering(voxels: np.ndarray, min_voxels: int = 1, order: str = "raster"):
    """(lut int32 [T + 1], kept old ids in their new order): components below `min_voxels` go to 0, the others are numbered 1 .. in
    raster order or (order="size") by descending size, ties by ascending raster id (a stable sort).  lut is None for the identity."""
    T = int(voxels.shape[0])
    old = np.flatnonzero(voxels >= min_voxels) + 1
    if order == "size":
        old = old[np.argsort(-voxels[old - 1], kind="stable")]
    if old.shape[0] == T and np.array_equal(old, np.arange(1, T + 1)):
        return None, old
    lut = np.zeros(T + 1, np.int32)
    lut[old] = np.arange(1, old.shape[0] + 1, dtype=np.int32)
    return lut, old


def components_dev(eng, lab_dev, vol_dev=None, hu_range=None, keep=None, per_label=True, connectivity=6, min_voxels=1, order="raster",
                   want_ids=True):
    """The device part of `find_components` on device-resident arrays -> (ids DeviceArray or None, rows, counts): the ids renumbered
    by ONE lm_relabel_dev where `min_voxels` / `order` ask for it, the rows permuted on the host to follow them."""
    ids, total, counts = eng.components_dev(lab_dev, vol_dev, hu_range, keep, per_label, connectivity)
    try:
        rows = eng.component_table_dev(ids, lab_dev, vol_dev, cap=total)[0]
        lut, old = renumbering(rows["voxels"], min_voxels, order)
        if lut is not None:
            rows = rows[old - 1]
            if want_ids:
                eng.relabel_dev(ids, lut, out=ids)
    except BaseException:
        ids.free()
        raise
    if not want_ids:
        ids.free()
        ids = None
    return ids, rows, counts


def table_columns(rows, has_image, spacing=None, index_to_physical=None) -> Dict[str, Optional[np.ndarray]]:
    """The raw fields of the rows plus the derived columns (module docstring), as numpy columns."""
    vox = rows["voxels"].astype(np.float64)
    t = {f: np.array(rows[f]) for f in RAW_FIELDS}
    if not has_image:
        t["hu_sum"] = t["hu_min"] = t["hu_max"] = None
    with np.errstate(invalid="ignore", divide="ignore"):
        t["centroid_index"] = rows["index_sum"].astype(np.float64) / vox[:, None]
        t["mean_hu"] = rows["hu_sum"].astype(np.float64) / vox if has_image else None
    t["centroid_mm"] = t["volume_ml"] = t["surface_area_mm2"] = t["equivalent_diameter_mm"] = None
    if index_to_physical is not None:  # an affine map: origin and the images of the three unit steps
        o = np.asarray(index_to_physical([0.0, 0.0, 0.0]), np.float64)
        m = np.stack([np.asarray(index_to_physical([float(a == 0), float(a == 1), float(a == 2)]), np.float64) - o for a in range(3)])
        t["centroid_mm"] = o + t["centroid_index"] @ m
    if spacing is not None:
        sz, sy, sx = (float(s) for s in spacing)
        f = rows["faces"].astype(np.float64)
        t["volume_ml"] = vox * (sz * sy * sx) / 1000.0
        t["surface_area_mm2"] = f[:, 0] * (sy * sx) + f[:, 1] * (sz * sx) + f[:, 2] * (sz * sy)
        t["equivalent_diameter_mm"] = np.cbrt(6.0 * vox * (sz * sy * sx) / math.pi)
    return t


class Components:
    """What `find_components` returns: `.ids` (int32, the caller's orientation), `.count`, `.table` (dict of numpy columns, row i - 1 for
    id i), `.counts` ({"voxels" / "nonfinite" / "selected": int64 [256] per label value}) and `.meta()`."""

    def __init__(self, ids, rows, counts, has_image, spacing, index_to_physical, params):
        self.ids = ids
        self.count = int(rows.shape[0])
        self.table = table_columns(rows, has_image, spacing, index_to_physical)
        self.counts = {"voxels": counts[0].copy(), "nonfinite": counts[1].copy(), "selected": counts[2].copy()}
        self.spacing = None if spacing is None else tuple(float(s) for s in spacing)
        self.params = params

    def meta(self, table: bool = True) -> dict:
        """JSON-serialisable: the parameters, the count, the per-label counts of the labels present and (table=True) the columns."""
        present = np.flatnonzero(self.counts["voxels"])
        out = dict(self.params)
        out.update({"count": self.count, "spacing_mm": None if self.spacing is None else list(self.spacing),
                    "counts": {str(int(k)): {f: int(self.counts[f][k]) for f in ("voxels", "nonfinite", "selected")} for k in present}})
        if table:
            out["table"] = {k: (None if v is None else v.tolist()) for k, v in self.table.items()}
        return out


def label_components(labels, image=None, hu_range=None, keep=None, per_label=True, connectivity=6, engine=None):
    """(ids int32, count): the connected components of the selected voxels of `labels` (module docstring), computed on the GPU."""
    check_arguments(hu_range, keep, connectivity, has_image=image is not None)
    arr, lab, _, _ = _volumes(image, labels, None)
    with _native.engine_scope(engine) as eng:
        ids, total, _, _ = eng.components(lab, arr, hu_range, keep, per_label, connectivity, table=False)
    return ids, total


def find_components(image, labels, hu_range=None, keep=None, per_label=True, connectivity=6, spacing=None, min_voxels=1, order="raster",
                    engine=None) -> Components:
    """The components of the selected voxels of `labels` (u8-valued [n][h][w]) over `image` (numpy array, volume_io.Volume, SimpleITK
    image, or None) with their table.  `spacing`: numpy input only, in the array's axis order.  `min_voxels`: smaller components are
    dropped (their voxels get id 0) and the ids compacted; `order`: "raster" (by first voxel) or "size" (largest first, ties by raster
    order).  `engine`: a _native.Engine (default: a new one on device 0)."""
    check_arguments(hu_range, keep, connectivity, min_voxels, order, has_image=image is not None)
    arr, lab, sp, to_phys = _volumes(image, labels, spacing)
    with _native.engine_scope(engine) as eng, eng.scope() as dev:
        ld = dev.upload(lab)
        vd = dev.upload(arr) if arr is not None else None
        ids, rows, counts = components_dev(eng, ld, vd, hu_range, keep, per_label, connectivity, min_voxels, order)
        host_ids = dev.add(ids).download()
    params = {"hu_range": None if hu_range is None else [None if v is None else int(v) for v in hu_range],
              "keep": None if keep is None else sorted(int(k) for k in set(keep)), "per_label": bool(per_label),
              "connectivity": int(connectivity), "min_voxels": int(min_voxels), "order": order}
    return Components(host_ids, rows, counts, arr is not None, sp, to_phys, params)


# ---- cluster analysis ---------------------------------------------------------------------------------------------------------------
def cluster_exponent(sizes) -> Optional[float]:
    """D of the cumulative cluster-size distribution: with Y(s) = the number of clusters of at least s voxels, minus the least-squares
    slope of log10 Y(s) against log10 s over the distinct sizes s; None with fewer than 3 distinct sizes.  float64 arithmetic."""
    sizes = np.sort(np.asarray(sizes, np.int64))
    s = np.unique(sizes)
    if s.shape[0] < 3:
        return None
    y = sizes.shape[0] - np.searchsorted(sizes, s, side="left")
    lx, ly = np.log10(s.astype(np.float64)), np.log10(y.astype(np.float64))
    dx, dy = lx - lx.mean(), ly - ly.mean()
    return float(-(dx * dy).sum() / (dx * dx).sum())


def summarize_clusters(sizes, voxels, nonfinite, selected, voxel_ml=None, name=None) -> dict:
    """One region's entry of `cluster_analysis` from its cluster sizes (voxels) and its three counts."""
    sizes = np.asarray(sizes, np.int64)
    finite = int(voxels) - int(nonfinite)
    out = {"name": name, "voxels": int(voxels), "nonfinite": int(nonfinite), "selected": int(selected),
           "fraction": None, "clusters": None, "largest_voxels": None, "largest_ml": None, "mean_voxels": None, "median_voxels": None,
           "size_histogram": None, "D": None}
    if int(voxels) == 0:
        return out
    out["fraction"] = int(selected) / finite if finite > 0 else None
    out["clusters"] = int(sizes.shape[0])
    out["size_histogram"] = []
    if sizes.shape[0] == 0:
        return out
    largest = int(sizes.max())
    out["largest_voxels"] = largest
    out["largest_ml"] = None if voxel_ml is None else largest * voxel_ml
    out["mean_voxels"] = int(sizes.sum()) / int(sizes.shape[0])
    out["median_voxels"] = float(np.median(sizes))
    bins = np.array([int(v).bit_length() - 1 for v in np.unique(sizes)])  # 2^b <= voxels < 2^(b+1), exactly
    per_size = np.unique(sizes, return_counts=True)[1]
    out["size_histogram"] = [int(c) for c in np.bincount(bins, weights=per_size, minlength=int(bins.max()) + 1).astype(np.int64)]
    out["D"] = cluster_exponent(sizes)
    return out


def cluster_range(threshold=-950, hu_range=None):
    """The inclusive HU range of the clusters: `hu_range`, or hu < threshold."""
    if hu_range is not None:
        return tuple(hu_range)
    if int(threshold) != threshold:
        raise ValueError(f"threshold: an integer HU value, got {threshold!r}")
    return (None, int(threshold) - 1)


def analysis_dev(eng, lab_dev, vol_dev, rng, connectivity=6, spacing=None, names=None, threshold=None) -> dict:
    """`cluster_analysis` on device-resident arrays: two device calls, per label and (per_label=False) for the whole lung."""
    _, rows, counts = components_dev(eng, lab_dev, vol_dev, rng, None, True, connectivity, want_ids=False)
    _, lung_rows, _ = components_dev(eng, lab_dev, vol_dev, rng, None, False, connectivity, want_ids=False)
    return finalize_analysis(rows, lung_rows, counts, rng, connectivity, spacing, names, threshold)


def finalize_analysis(rows, lung_rows, counts, rng, connectivity, spacing=None, names=None, threshold=None) -> dict:
    names = dict(names or {})
    sp = None if spacing is None else [float(s) for s in spacing]
    voxel_ml = None if sp is None else float(np.prod(sp)) / 1000.0
    ks = sorted({int(k) for k in names} | {int(k) for k in np.flatnonzero(counts[0][1:]) + 1})
    labels = {}
    for k in ks:
        labels[str(k)] = summarize_clusters(rows["voxels"][rows["label"] == k], counts[0][k], counts[1][k], counts[2][k], voxel_ml,
                                            names.get(k, f"label {k}"))
    lung = summarize_clusters(lung_rows["voxels"], counts[0][1:].sum(), counts[1][1:].sum(), counts[2][1:].sum(), voxel_ml, "lung")
    return {"threshold": None if threshold is None else int(threshold), "hu_range": [None if v is None else int(v) for v in rng],
            "connectivity": int(connectivity), "spacing_mm": sp, "voxel_volume_ml": voxel_ml, "labels": labels, "lung": lung}


def cluster_analysis(image, labels, threshold=-950, hu_range=None, connectivity=6, spacing=None, names=None, engine=None) -> dict:
    """The cluster analysis (module docstring) of `labels` over `image`, computed on the GPU -> a JSON-serialisable dict: threshold,
    hu_range, connectivity, spacing_mm, voxel_volume_ml, labels {"k": entry} and lung (every label >= 1 as one region: clusters cross
    label borders there).  An entry: name, voxels, nonfinite, selected, fraction (selected / finite voxels), clusters, largest_voxels,
    largest_ml, mean_voxels, median_voxels, size_histogram (entry b: clusters with 2^b <= voxels < 2^(b+1)) and D.  By default the
    clusters are those of hu < threshold; `hu_range` = (lo, hi) overrides it (e.g. (-300, None): high-attenuation lesions).  Labels
    without a voxel report None for every derived field."""
    if image is None:
        raise ValueError("cluster_analysis needs an image")
    rng = cluster_range(threshold, hu_range)
    check_arguments(rng, None, connectivity)
    arr, lab, sp, _ = _volumes(image, labels, spacing)
    with _native.engine_scope(engine) as eng, eng.scope() as dev:
        return analysis_dev(eng, dev.upload(lab), dev.upload(arr), rng, connectivity, sp, names, None if hu_range is not None else threshold)
