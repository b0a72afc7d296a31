"""Vessel centrelines, calibre classes and the vessel tree on the GPU (not in the reference: what callers run
`skimage.morphology.skeletonize` and a distance transform on the host for, tens of seconds per chest CT).

The device passes (`lm_skeleton_dev`, `lm_skeleton_points_dev`, `lm_calibre_dev`, lungmask_amd/csrc/skeleton_kernels.hip) follow the
definitions in include/lungmask_hip.h.  In short:

- The skeleton is what a directional, 8-subfield parallel thinning leaves: a voxel is deleted when it is a simple point (deleting it
  changes no 26-component of the object, no cavity and no tunnel) and no end point.  The skeleton therefore has the topology of the
  mask exactly; it is a curve skeleton (surfaces thin to curves too).  The result is DEFINED by the order of the sub-steps in the
  header, in integers, and does not depend on the schedule.  The code volume holds 0, or 1 + the number of skeleton voxels among the
  26 neighbours: 1 isolated, 2 end, 3 curve voxel, >= 4 junction voxel.
- The local radius of a skeleton voxel is the square root of `lm_edt_dev`'s squared distance to the nearest voxel outside the mask.
  That is a distance between voxel CENTRES: for thin vessels it overestimates the radius by up to half a voxel.
- The calibre class of a skeleton voxel is 1 + the number of class edges its radius reaches; every voxel of the mask takes the class
  of the nearest skeleton voxel (`lm_nearest_label_dev`'s rule).  `vessel_tree`'s default edges are the radii of circles of 5 and
  10 mm^2, the customary BV5 / BV10 split; they are conventional, and nothing here validates them clinically.
- The graph (junction clusters, segments, lengths) is built on the host from the point list, a few hundred thousand points at most.

Everything is in the caller's array orientation (no LPS re-orientation), as the vessel analysis is.
"""
from __future__ import annotations

import math

import numpy as np

from . import _native
from . import filters as _filters
from . import vessels as _vessels

DEFAULT_CALIBRES_MM2 = (5.0, 10.0)
MAX_CALIBRES = _native.CALIBRE_MAX_EDGES
_OFFSETS = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]


def calibre_edges_mm(calibres_mm2):
    """The class edges as radii in mm: sqrt(A / pi) of the cross-sectional areas `calibres_mm2` (1 to 7, strictly ascending, > 0)."""
    areas = [calibres_mm2] if np.ndim(calibres_mm2) == 0 else list(calibres_mm2)
    if not 1 <= len(areas) <= MAX_CALIBRES or not all(np.ndim(a) == 0 and math.isfinite(float(a)) and float(a) > 0 for a in areas) or \
            any(float(b) <= float(a) for a, b in zip(areas, areas[1:])):
        raise ValueError(f"calibres_mm2: 1 to {MAX_CALIBRES} strictly ascending areas > 0 in mm^2, got {calibres_mm2!r}")
    return _native.Engine._calibre_edges([math.sqrt(float(a) / math.pi) for a in areas])


def _mask_volume(mask):
    arr = np.asarray(getattr(mask, "array", mask))
    if arr.ndim != 3:
        raise ValueError(f"need a 3-D volume, got shape {arr.shape}")
    if arr.dtype == bool:
        return np.ascontiguousarray(arr, dtype=np.uint8)
    if arr.dtype != np.uint8:
        if arr.size and (arr.min() < 0 or arr.max() > 255 or (arr != np.rint(arr)).any()):
            raise ValueError("need a bool mask or label values in 0 .. 255")
        arr = arr.astype(np.uint8)
    return np.ascontiguousarray(arr)


def skeletonize(mask, keep=None, engine=None, return_info: bool = False):
    """uint8 [n][h][w]: the skeleton codes of `mask` (a bool volume, or labels of which the values in `keep` are selected; None:
    every value >= 1) -- 0, or 1 + the number of skeleton voxels among the 26 neighbours (1 isolated, 2 end, 3 curve voxel, >= 4
    junction voxel).  An empty selection gives zeros.  With `return_info` -> (codes, {"selected", "skeleton", "passes"}).
    `engine`: a _native.Engine (default: a new one on device 0)."""
    arr = _mask_volume(mask)
    table = np.frombuffer(bytes(_native.Engine._keep_table(keep)), np.uint8)
    if arr.size == 0 or not table[arr].any():
        out = np.zeros(arr.shape, np.uint8)
        return (out, {"selected": 0, "skeleton": 0, "passes": 0}) if return_info else out
    with _native.engine_scope(engine) as eng:
        return eng.skeleton(arr, keep, return_info=return_info)


# ---- graph ----------------------------------------------------------------------------------------------------------------------------
def graph_from_points(shape, index, code, spacing=None, radius=None) -> dict:
    """The graph of a skeleton given as its point list (`lm_skeleton_points_dev`'s: raster indices ascending, codes, and optionally
    one radius in mm per point).  See `skeleton_graph`."""
    n, h, w = (int(s) for s in shape)
    index = np.asarray(index, np.int64)
    code = np.asarray(code, np.uint8)
    sp = [1.0, 1.0, 1.0] if spacing is None else [float(s) for s in spacing]
    if len(sp) != 3 or not all(s > 0 and math.isfinite(s) for s in sp):
        raise ValueError(f"spacing needs three positive values in the array's axis order, got {spacing!r}")
    if radius is not None:
        radius = np.asarray(radius, np.float64).tolist()
    P = index.size
    z, y, x = index // (h * w), (index // w) % h, index % w
    nbr = np.full((P, 26), -1, np.int64)  # the point number of each of the 26 neighbours, -1: no skeleton voxel there
    for j, (dz, dy, dx) in enumerate(_OFFSETS):
        zz, yy, xx = z + dz, y + dy, x + dx
        ok = (zz >= 0) & (zz < n) & (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        target = (zz * h + yy) * w + xx
        pos = np.searchsorted(index, target)
        pos[pos >= P] = 0
        hit = ok & (index[pos] == target) if P else ok
        nbr[hit, j] = pos[hit]
    # the links as plain lists (a skeleton voxel has few neighbours): those of point q are adj[ptr[q]:ptr[q + 1]], by ascending
    # point number = ascending raster index, with the offset number of each in `via`
    rows, cols = np.nonzero(nbr >= 0)
    order_ = np.lexsort((nbr[rows, cols], rows))
    rows, cols = rows[order_], cols[order_]
    adj, via = nbr[rows, cols].tolist(), cols.tolist()
    ptr = np.searchsorted(rows, np.arange(P + 1)).tolist()
    junction = (code >= 4).tolist()
    raster = index.tolist()
    cluster = [-1] * P
    junctions = []
    for p in range(P):  # ascending raster index: a cluster is numbered by its first voxel
        if not junction[p] or cluster[p] >= 0:
            continue
        cid, stack, members = len(junctions), [p], 0
        cluster[p] = cid
        while stack:
            q = stack.pop()
            members += 1
            for r in adj[ptr[q]:ptr[q + 1]]:
                if junction[r] and cluster[r] < 0:
                    cluster[r] = cid
                    stack.append(r)
        junctions.append({"id": cid, "voxels": members, "index": raster[p]})
    step = [math.sqrt(sum((o * s) ** 2 for o, s in zip(off, sp))) for off in _OFFSETS]
    seen = [False] * P
    segments = []
    for p in range(P):
        if junction[p] or seen[p]:
            continue
        # the 26-component of non-junction voxels that holds p (its first voxel): every voxel has at most two skeleton neighbours,
        # so it is a path or a cycle
        member, stack = [p], [p]
        seen[p] = True
        while stack:
            q = stack.pop()
            for r in adj[ptr[q]:ptr[q + 1]]:
                if not junction[r] and not seen[r]:
                    seen[r] = True
                    member.append(r)
                    stack.append(r)
        links = {q: [(r, j) for r, j in zip(adj[ptr[q]:ptr[q + 1]], via[ptr[q]:ptr[q + 1]]) if not junction[r]] for q in member}
        ends = sorted(q for q in member if len(links[q]) < 2)
        closed = not ends
        start = p if closed else ends[0]
        order, length, prev, cur = [start], 0.0, None, start
        while True:
            nxt = [(r, j) for r, j in links[cur] if r != prev]
            if closed and prev is None:
                nxt = nxt[:1]  # a cycle is walked from its first voxel towards the neighbour with the smaller raster index
            if not nxt:
                break
            r, j = nxt[0]
            length += step[j]
            if r == start:  # the link that closes the cycle
                break
            order.append(r)
            prev, cur = cur, r
        assert len(order) == len(member), "a segment is a path or a cycle"

        def touching(q):
            return sorted({cluster[r] for r in adj[ptr[q]:ptr[q + 1]] if junction[r]})

        if closed:
            attach = [None, None]
        elif len(order) == 1:
            attach = (touching(order[0]) + [None, None])[:2]
        else:
            attach = [(touching(q) + [None])[0] for q in (order[0], order[-1])]
        seg = {"id": len(segments), "voxels": len(order), "length_mm": float(length), "closed": bool(closed), "ends": attach,
               "first_index": raster[p], "radius_mm": None}
        if radius is not None:
            r = [radius[q] for q in order]
            seg["radius_mm"] = {"min": min(r), "mean": math.fsum(r) / len(r), "max": max(r)}
        segments.append(seg)
    return {"shape": [n, h, w], "spacing_mm": None if spacing is None else sp, "voxels": int(P), "end_points": int((code == 2).sum()),
            "isolated": int((code == 1).sum()), "junctions": junctions, "segments": segments}


def skeleton_graph(mask_or_codes, spacing=None, radius=None, engine=None) -> dict:
    """The graph of a skeleton, built on the host from its point list -> a JSON-serialisable dict: shape, spacing_mm, voxels,
    end_points, isolated, junctions and segments.  `mask_or_codes`: a bool volume is a mask and is skeletonised first (`skeletonize`);
    any other volume is taken as the code volume `skeletonize` returns.  `spacing` in the array's axis order (None: voxels).
    `radius`: None, or a volume of radii in mm (the square root of `calibre`'s distances), sampled on the skeleton.

    - junctions: the 26-components of the voxels with code >= 4, numbered by their first raster index: id, voxels, index.
    - segments: the 26-components of the other skeleton voxels, numbered likewise.  Each of those voxels has at most two skeleton
      neighbours, so a segment is a path or a cycle: id, voxels, length_mm (the sum of the Euclidean distances between consecutive
      voxel centres of the segment; the links to a junction are not counted), closed, ends (per end the id of the junction cluster
      that touches it -- the smallest id when several do -- or None for a free end; a path starts at its end with the smaller
      raster index), first_index, and radius_mm {min, mean, max} (None without `radius`).
    The radius is a centre-to-centre distance: for thin vessels it overestimates the true radius by up to half a voxel."""
    arr = np.asarray(getattr(mask_or_codes, "array", mask_or_codes))
    if arr.ndim != 3:
        raise ValueError(f"need a 3-D volume, got shape {arr.shape}")
    codes = skeletonize(arr, engine=engine) if arr.dtype == bool else _mask_volume(arr)
    if radius is not None and np.shape(radius) != codes.shape:
        raise ValueError(f"radius must have the volume's shape {codes.shape}, got {np.shape(radius)}")
    index = np.flatnonzero(codes.ravel())
    pts = None if radius is None else np.asarray(radius, np.float64).ravel()[index]
    return graph_from_points(codes.shape, index, codes.ravel()[index], spacing, pts)


# ---- vessel tree ----------------------------------------------------------------------------------------------------------------------
def _tree_entry(name, row, label_of_point, code, graph, k, voxel_ml):
    """One label's (k; None: the lung, every label >= 1) entry of the tree from its calibre counts `row` [9]."""
    voxels = int(row.sum())
    out = {"name": name, "vessel_voxels": voxels, "skeleton_voxels": None, "segments": None, "length_mm": None, "junctions": None,
           "ends": None, "by_calibre": None}
    if voxels == 0:
        return out
    mine = (label_of_point >= 1) if k is None else (label_of_point == k)
    first = {int(i): bool(m) for i, m in zip(graph["_index"], mine)}
    segs = [s for s in graph["segments"] if first[s["first_index"]]]
    out["skeleton_voxels"] = int(mine.sum())
    out["segments"] = len(segs)
    out["length_mm"] = float(sum(s["length_mm"] for s in segs))
    out["junctions"] = sum(1 for j in graph["junctions"] if first[j["index"]])
    out["ends"] = int((mine & (code == 2)).sum())
    out["by_calibre"] = [{"class": c, "voxels": int(row[c]), "ml": None if voxel_ml is None else int(row[c]) * voxel_ml}
                         for c in range(1, graph["_classes"] + 1)]
    return out


def finalize_tree(shape, index, code, d2_points, lab_points, counts, calibres_mm2, spacing=None, names=None) -> dict:
    """The tree dict from the device results: the point list with its squared distances and labels, and lm_calibre_dev's counts."""
    names = dict(names or {})
    sp = None if spacing is None else [float(s) for s in spacing]
    voxel_ml = None if sp is None else float(np.prod(sp)) / 1000.0
    areas = [float(a) for a in ([calibres_mm2] if np.ndim(calibres_mm2) == 0 else calibres_mm2)]
    graph = graph_from_points(shape, index, code, sp, np.sqrt(np.asarray(d2_points, np.float64)))
    graph["_index"], graph["_classes"] = np.asarray(index, np.int64), len(areas) + 1
    counts = np.asarray(counts, np.int64)
    lab_points, code = np.asarray(lab_points, np.int64), np.asarray(code, np.uint8)
    ks = sorted({int(k) for k in names} | {int(k) for k in np.flatnonzero(counts[1:].sum(axis=1)) + 1})
    labels = {str(k): _tree_entry(names.get(k, f"label {k}"), counts[k] if k < counts.shape[0] else counts[0] * 0, lab_points, code, graph, k,
                                  voxel_ml) for k in ks}
    lung = _tree_entry("lung", counts[1:].sum(axis=0), lab_points, code, graph, None, voxel_ml)
    del graph["_index"], graph["_classes"]
    return {"calibres_mm2": areas, "edges_mm": calibre_edges_mm(areas), "spacing_mm": sp, "voxel_volume_ml": voxel_ml, "labels": labels,
            "lung": lung, "graph": graph}


class VesselTree(_vessels.VesselResult):
    """What `LMInferer.apply_with_vessel_tree` and `vessel_tree` return: `vessels.VesselResult` (vesselness, scale, mask, analysis)
    plus `skeleton` uint8 [n][h][w] (the codes of the vessel mask's skeleton), `calibre` uint8 [n][h][w] (the calibre class of every
    voxel of the mask, 0 elsewhere) and `tree` (the dict of `vessel_tree`)."""

    def __init__(self, vesselness, scale, mask, analysis, skeleton, calibre, tree):
        super().__init__(vesselness, scale, mask, analysis)
        self.skeleton, self.calibre, self.tree = skeleton, calibre, tree


def empty_tree(calibres_mm2, spacing=None, names=None) -> dict:
    """The tree of a vessel mask without a voxel."""
    return finalize_tree((0, 1, 1), np.zeros(0, np.int64), np.zeros(0, np.uint8), np.zeros(0, np.float32), np.zeros(0, np.int64),
                         np.zeros((16, _native.CALIBRE_COLUMNS), np.int64), calibres_mm2, spacing, names)


def tree_dev(eng, vol_dev, lab_dev, calibres_mm2=DEFAULT_CALIBRES_MM2, spacing=None, names=None, **kw) -> VesselTree:
    """`vessels.analysis_dev` and, on its device arrays, the vessel mask, its skeleton, the calibre classes and the point list; the
    volumes are brought to the host once.  NoKeptVoxel when nothing is labelled."""
    edges = calibre_edges_mm(calibres_mm2)
    threshold = kw.get("threshold", 0.5)
    v, sc, eroded, analysis = _vessels.analysis_dev(eng, vol_dev, lab_dev, spacing=spacing, names=names, **kw)
    with eng.scope() as dev:
        dev.add(v, sc, eroded)
        mask = eng.vessel_mask_dev(v, eroded, threshold, out=eroded)  # (the eroded labels are spent)
        shape = mask.shape
        try:
            skel = dev.add(eng.skeleton_dev(mask)[0])
        except _native.NoKeptVoxel:  # no vessel voxel
            eng.sync()
            V = v.download()
            return VesselTree(V, sc.download(), np.zeros(shape, bool), analysis, np.zeros(shape, np.uint8), np.zeros(shape, np.uint8),
                              empty_tree(calibres_mm2, spacing, names))
        cls, counts, d2 = eng.calibre_dev(skel, mask, edges, spacing=spacing, lab=lab_dev, return_distance=True)
        dev.add(cls, d2)
        index, code, d2_points, _ = eng.skeleton_points_dev(skel, d2)
        V, codes = v.download(), skel.download()
        lab_points = lab_dev.download().ravel()[index]
        tree = finalize_tree(shape, index, code, d2_points, lab_points, counts, calibres_mm2, spacing, names)
        return VesselTree(V, sc.download(), mask.download() != 0, analysis, codes, cls.download(), tree)


def vessel_tree(image, labels, sigmas_mm=_vessels.DEFAULT_SIGMAS_MM, threshold: float = 0.5, erode_mm: float = 2.0,
                calibres_mm2=DEFAULT_CALIBRES_MM2, spacing=None, names=None, alpha: float = 0.5, beta: float = 0.5, c: float = 100.0,
                bright: bool = True, engine=None) -> VesselTree:
    """`vessels.vessel_result(image, labels, ...)` plus the centrelines of its vessel mask: `.skeleton` (the code volume of
    `skeletonize(mask)`), `.calibre` (per voxel of the mask the calibre class 1 .. len(calibres_mm2) + 1 of the nearest skeleton voxel:
    class c holds the vessels whose radius reaches c - 1 of the edges sqrt(A / pi) of the cross-sectional areas `calibres_mm2`) and
    `.tree`, a JSON-serialisable dict: calibres_mm2, edges_mm, spacing_mm, voxel_volume_ml, labels {"k": entry}, lung (every label >= 1
    together) and graph (`skeleton_graph`'s dict, with the radii).  An entry: name, vessel_voxels, skeleton_voxels, segments and
    length_mm (a segment belongs to the label of its first voxel), junctions (clusters, likewise), ends (end voxels) and by_calibre
    (voxels and ml per class; the first class of the defaults is BV5, the first two together BV10).  Labels without a vessel voxel
    report None for the derived fields.  The 5 and 10 mm^2 defaults are conventional; nothing here validates them clinically."""
    if labels is None:
        raise ValueError("vessel_tree needs labels")
    _vessels.check_analysis_arguments(threshold, erode_mm)
    calibre_edges_mm(calibres_mm2)
    arr, lab, sp = _filters._inputs(image, labels, spacing)
    _native.Engine._vessel_params(_vessels.scale_sigmas(sigmas_mm, sp), 4.0, True, None, alpha, beta, c, bright)
    kw = dict(sigmas_mm=sigmas_mm, threshold=threshold, erode_mm=erode_mm, alpha=alpha, beta=beta, c=c, bright=bright)
    if arr.size == 0 or not lab.any():
        return empty_vessel_tree(arr.shape, calibres_mm2, sp, names, **kw)
    with _native.engine_scope(engine) as eng, eng.scope() as dev:
        return tree_dev(eng, dev.upload(arr), dev.upload(lab), calibres_mm2, sp, names, **kw)


def empty_vessel_tree(shape, calibres_mm2, spacing=None, names=None, sigmas_mm=_vessels.DEFAULT_SIGMAS_MM, threshold=0.5, erode_mm=2.0,
                      alpha=0.5, beta=0.5, c=100.0, bright=True) -> VesselTree:
    """Nothing is labelled: zeros, an analysis of empties and an empty tree."""
    params = {"alpha": float(alpha), "beta": float(beta), "c": float(c), "bright": bool(bright)}
    r = _vessels.empty_result(shape, sigmas_mm, threshold, erode_mm, spacing, names, params)
    return VesselTree(r.vesselness, r.scale, r.mask, r.analysis, np.zeros(shape, np.uint8), np.zeros(shape, np.uint8),
                      empty_tree(calibres_mm2, spacing, names))
