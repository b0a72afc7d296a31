"""Airway tree segmentation on the GPU (not in the reference, whose networks leave the trachea and the bronchi out of their labels):
a seeded minimax flood from the trachea, an explosion rule on its volume curve, and the airway tree from the mask's skeleton.

The device passes (`lm_seed_cost_dev`, `lm_airway_mask_dev`, lungmask_amd/csrc/airway_kernels.hip) follow the definitions in
include/lungmask_hip.h.  In short:

- `minimax_cost`: per voxel the smallest threshold T at which region growing `HU <= T` from the seed reaches it -- the minimum over
  6-connected paths of the largest HU on the path.  The whole family of region-growing results is `cost <= T`, and the
  volume-against-threshold curve is the cumulative histogram of the cost: ONE flood instead of one labelling per candidate threshold.
- `find_trachea`: the seed, from the connected components of the air outside the lung labels.
- `choose_threshold`: explosion-controlled region growing as exact host arithmetic on the curve.
- `segment_airways`: the three together, with the per-label volumes and the tree.
- `airway_tree`: skeleton, radii and graph of the mask (the vessel tree's device calls), pruned and ordered by generation on the host.

What this is NOT.  It is ONE global threshold: it reaches the generations whose lumen stays below the HU at which the first wall
breaks, typically the lobar to segmental bronchi, and stops there.  There is no per-branch adaptive threshold, no leak repair, no
wall-thickness measurement and no 26-connectivity (thin walls have diagonal gaps, which is exactly where a flood must not pass).  A
scan that includes the mouth or the nose connects the trachea to the outside air: the rule then leaks at once and reports no
threshold.  Every default here (-950 HU seed air, -800 HU cap, 10 HU steps, the leak sizes, the trachea's 20 mm and 600 mm^2) is
conventional and is not validated on patient data.  Diameters are twice a centre-to-centre distance (`skeleton.skeleton_graph`): for
thin airways they overestimate the lumen by up to a voxel.

Everything is in the caller's array orientation (no LPS re-orientation); axis 0 is the slice axis.
"""
from __future__ import annotations

import math

import numpy as np

from . import _native
from . import filters as _filters
from . import skeleton as _skeleton

UNREACHED = 32767
DEFAULT_CAP_HU = -800
RULE_DEFAULTS = dict(start_hu=-950, step_hu=10, leak_ratio=1.5, leak_ml=10.0, max_ml=400.0)


class NoTrachea(ValueError):
    """`find_trachea` found no candidate; the message says what it found."""


# ---- the flood ------------------------------------------------------------------------------------------------------------------------
def _check_cap(cap_hu):
    if np.ndim(cap_hu) != 0 or int(cap_hu) != cap_hu or not -1023 <= cap_hu <= 3071:
        raise ValueError(f"cap_hu: an integer in -1023 .. 3071, got {cap_hu!r}")
    return int(cap_hu)


def _seed_list(seed):
    arr = np.asarray(seed)
    if arr.dtype.kind not in "iu" or arr.size == 0 or arr.ndim not in (1, 2) or arr.shape[-1] != 3:
        raise ValueError(f"seed: one (z, y, x) of integers or a list of them, got {seed!r}")
    return [tuple(int(v) for v in s) for s in arr.reshape(-1, 3)]


def minimax_cost(image, seeds, cap_hu=DEFAULT_CAP_HU, engine=None):
    """(cost int16 [n][h][w], curve int64 [cap_hu + 1025], info) of the minimax flood from `seeds` (one (z, y, x) or up to 64):
    cost[v] is the smallest T at which v is connected to a seed through 6-connected voxels with HU <= T, over voxels with HU <=
    `cap_hu` only (HU = the image value, floats rounded half to even, below -1024 counted as -1024; NaN never passes), and 32767
    where there is no such path.  curve[k] = the voxels with cost == -1024 + k; info = rounds, reached, seeds_passable, converged.
    The building block of any seeded region growing: `cost <= T` IS the region grown at threshold T."""
    arr, _, _ = _filters._inputs(image, None, None)
    cap = _check_cap(cap_hu)
    with _native.engine_scope(engine) as eng:
        return eng.seed_cost(arr, _seed_list(seeds), cap)


# ---- the trachea ----------------------------------------------------------------------------------------------------------------------
def _check_trachea_arguments(seed_hu, min_length_mm, max_area_mm2):
    if np.ndim(seed_hu) != 0 or int(seed_hu) != seed_hu or not -1024 <= seed_hu <= 3071:
        raise ValueError(f"seed_hu: an integer in -1024 .. 3071, got {seed_hu!r}")
    for name, v in (("min_length_mm", min_length_mm), ("max_area_mm2", max_area_mm2)):
        if not (np.ndim(v) == 0 and math.isfinite(float(v)) and float(v) > 0):
            raise ValueError(f"{name}: a number > 0, got {v!r}")


def pick_trachea(rows, shape, lung_box=None, spacing=None, min_length_mm=20.0, max_area_mm2=600.0) -> dict:
    """`find_trachea`'s rule on the component table `rows` (_native.COMPONENT_DTYPE) of the air outside the labels.  `lung_box`:
    (y0, y1, x0, x1), maxima exclusive, of the voxels with a label >= 1, or None."""
    n, h, w = shape
    sp = [1.0, 1.0, 1.0] if spacing is None else [float(s) for s in spacing]
    voxel = sp[0] * sp[1] * sp[2]
    table, why = [], {"touches_border": 0, "too_short": 0, "too_wide": 0, "outside_lung_box": 0}
    for i, r in enumerate(rows):
        vox = int(r["voxels"])
        if vox == 0:
            continue
        z0, z1, y0, y1, x0, x1 = (int(v) for v in r["bbox"])
        length = (z1 - z0) * sp[0]
        cy, cx = int(r["index_sum"][1]) / vox, int(r["index_sum"][2]) / vox
        reason = None
        if y0 == 0 or x0 == 0 or y1 == h or x1 == w:
            reason = "touches_border"
        elif length < min_length_mm:
            reason = "too_short"
        elif vox * voxel / length > max_area_mm2:
            reason = "too_wide"
        elif lung_box is not None and not (lung_box[0] <= cy < lung_box[1] and lung_box[2] <= cx < lung_box[3]):
            reason = "outside_lung_box"
        if reason is not None:
            why[reason] += 1
            continue
        first = int(r["first"])
        table.append({"component": i + 1, "voxels": vox, "length_mm": float(length), "mean_area_mm2": float(vox * voxel / length),
                      "centroid_yx": [cy, cx], "bbox": [z0, z1, y0, y1, x0, x1],
                      "index": [first // (h * w), (first // w) % h, first % w]})
    if not table:
        raise NoTrachea(f"find_trachea: no candidate among {len(rows)} air components outside the labels ({why['touches_border']} touch "
                        f"the y or x border, {why['too_short']} shorter than {min_length_mm} mm along axis 0, {why['too_wide']} wider "
                        f"than {max_area_mm2} mm^2, {why['outside_lung_box']} off the lungs' in-plane box)")
    table.sort(key=lambda c: (-c["length_mm"], -c["voxels"], c["component"]))
    best = table[0]
    return {"index": tuple(best["index"]), "component": best["component"], "candidates": table, "rejected": why,
            "components": int(len(rows))}


def trachea_dev(eng, vol_dev, lab_dev, seed_hu=-950, spacing=None, min_length_mm=20.0, max_area_mm2=600.0) -> dict:
    """`find_trachea` on device-resident image and labels (u8; None: no labels)."""
    shape = tuple(vol_dev.shape)
    with eng.scope() as dev:
        lung_box = None
        if lab_dev is None:
            lab_dev = dev.upload(np.zeros(shape, np.uint8))
        else:
            try:
                bb = eng.roi_plan_dev(lab_dev)
                lung_box = tuple(int(v) for v in bb[2:6])
            except ValueError:  # labels without a voxel >= 1
                lung_box = None
        ids, total, _ = eng.components_dev(lab_dev, vol_dev, hu_range=(None, int(seed_hu)), keep=[0], per_label=False, connectivity=6)
        dev.add(ids)
        rows = eng.component_table_dev(ids, lab_dev, vol_dev, cap=total)[0] if total else np.zeros(0, _native.COMPONENT_DTYPE)
    return pick_trachea(rows, shape, lung_box, spacing, min_length_mm, max_area_mm2)


def find_trachea(image, labels=None, seed_hu=-950, spacing=None, engine=None, min_length_mm=20.0, max_area_mm2=600.0) -> dict:
    """The trachea as a seed for the flood -> {"index": (z, y, x), "component", "candidates", "rejected", "components"}.

    The 6-connected components (`Engine.components_dev`, not per label) of the voxels with HU <= `seed_hu` whose label is 0 (every
    voxel without `labels`) are candidates when (1) their box does not touch the y or x borders of the array -- outside air does;
    axis 0 is the slice axis and touching its ends is allowed, the trachea leaves through the top slice; (2) their extent along axis
    0 is at least `min_length_mm`; (3) their volume divided by that extent is at most `max_area_mm2` -- a tube, not a stomach
    bubble; (4) with labels that hold a voxel >= 1, their in-plane centroid lies inside the in-plane box of those voxels.  The winner
    has the largest extent along axis 0, then the larger volume, then the smaller id; the seed is its first voxel in raster order.
    `candidates` lists them in that order (component, voxels, length_mm, mean_area_mm2, centroid_yx, bbox, index).  Without `spacing`
    millimetres are voxels.  NoTrachea (a ValueError) says what was found when nothing qualifies.  The constants are conventional
    and are not clinically validated."""
    _check_trachea_arguments(seed_hu, min_length_mm, max_area_mm2)
    arr, lab, sp = _filters._inputs(image, labels, spacing)
    if arr.size == 0:
        raise NoTrachea("find_trachea: the volume is empty")
    with _native.engine_scope(engine) as eng, eng.scope() as dev:
        return trachea_dev(eng, dev.upload(arr), None if lab is None else dev.upload(lab), seed_hu, sp, min_length_mm, max_area_mm2)


# ---- the explosion rule ---------------------------------------------------------------------------------------------------------------
def choose_threshold(curve, voxel_ml, start_hu=-950, step_hu=10, leak_ratio=1.5, leak_ml=10.0, max_ml=400.0) -> dict:
    """Explosion-controlled region growing on the flood's curve (curve[k] = the voxels with cost == -1024 + k; the cap is len(curve)
    - 1025) -> {"threshold", "first_leaking", "voxels", "volume_ml", "cap_hu", "curve": [[t, V[t]] ...]}.

    V[t] = the voxels with cost <= t.  For t = start_hu + step_hu, start_hu + 2 step_hu, ... <= cap_hu, t is LEAKING iff V[t] >
    max_ml, or both V[t] - V[t - step_hu] > leak_ml and V[t] > leak_ratio * V[t - step_hu] (volumes as voxel counts: x_ml /
    voxel_ml).  `threshold` is the first leaking t minus step_hu -- the whole window in which the growth happened is given back --
    and cap_hu when no t leaks; a threshold at which V is 0 is reported as None.  Thresholds below start_hu are never tested: the
    trachea itself fills up there.  `curve` samples V at start_hu, start_hu + step_hu, ... and at cap_hu.

    What it cannot avoid: a scan that includes the mouth or the nose connects the trachea to the outside air; the first step then
    leaks (or V[start_hu] is already beyond max_ml, which nothing tests) and the result is None or useless."""
    curve = np.asarray(curve)
    if curve.ndim != 1 or curve.dtype.kind not in "iu" or not 2 <= curve.size <= 3071 + 1025 or (curve < 0).any():
        raise ValueError("curve: the int64 histogram of lm_seed_cost_dev, cap_hu + 1025 entries")
    cap = int(curve.size) - 1025
    if not (np.ndim(voxel_ml) == 0 and math.isfinite(float(voxel_ml)) and float(voxel_ml) > 0):
        raise ValueError(f"voxel_ml: a number > 0, got {voxel_ml!r}")
    if int(start_hu) != start_hu or not -1024 <= start_hu <= cap:
        raise ValueError(f"start_hu: an integer in -1024 .. cap_hu ({cap}), got {start_hu!r}")
    if int(step_hu) != step_hu or step_hu < 1:
        raise ValueError(f"step_hu: an integer >= 1, got {step_hu!r}")
    for name, v, lo in (("leak_ratio", leak_ratio, 1.0), ("leak_ml", leak_ml, 0.0), ("max_ml", max_ml, 0.0)):
        if not (np.ndim(v) == 0 and math.isfinite(float(v)) and float(v) >= lo):
            raise ValueError(f"{name}: a number >= {lo}, got {v!r}")
    start, step = int(start_hu), int(step_hu)
    V = np.cumsum(curve.astype(np.int64))
    at = lambda t: int(V[t + 1024])  # noqa: E731
    leak_voxels, max_voxels = float(leak_ml) / float(voxel_ml), float(max_ml) / float(voxel_ml)
    first = None
    for t in range(start + step, cap + 1, step):
        now, before = at(t), at(t - step)
        if now > max_voxels or (now - before > leak_voxels and now > float(leak_ratio) * before):
            first = t
            break
    threshold = cap if first is None else first - step
    voxels = at(threshold)
    samples = sorted(set(range(start, cap + 1, step)) | {cap})
    return {"threshold": threshold if voxels > 0 else None, "first_leaking": first, "voxels": voxels,
            "volume_ml": voxels * float(voxel_ml), "cap_hu": cap, "curve": [[t, at(t)] for t in samples]}


# ---- the tree -------------------------------------------------------------------------------------------------------------------------
def _nearest_segment(graph, shape, seed, scale):
    """The id of the segment that holds the skeleton voxel (of a segment) nearest to the seed, in mm; ties: the smaller raster index."""
    n, h, w = (int(v) for v in shape)
    owner = {p: s["id"] for s in graph["segments"] for p in s["_points"]}
    pts = np.asarray(sorted(owner), np.int64)
    zyx = np.stack([pts // (h * w), (pts // w) % h, pts % w], axis=1)
    d = (((zyx - np.asarray(seed, np.int64)) * scale) ** 2).sum(axis=1)
    return owner[int(pts[int(np.argmin(d))])]


def _spurs(graph, root, spur_factor):
    """The segments to prune: free-ended ones other than the root with length_mm < spur_factor * their largest radius, at a junction
    cluster that joins three segment ends or more."""
    degree = {}
    for s in graph["segments"]:
        for j in s["ends"]:
            if j is not None:
                degree[j] = degree.get(j, 0) + 1
    out = []
    for s in graph["segments"]:
        if s["id"] == root or s["closed"] or (s["ends"][0] is None) == (s["ends"][1] is None):
            continue
        j = s["ends"][0] if s["ends"][0] is not None else s["ends"][1]
        if s["length_mm"] < spur_factor * s["radius_mm"]["max"] and degree[j] >= 3:
            out.append(s)
    return out


def _rooted_graph(shape, index, code, d2_points, seed, sp):
    """(graph with the segments' voxels, id of the root segment or None) of a skeleton's point list."""
    graph = _graph_with_points(shape, index, code, sp, np.sqrt(np.asarray(d2_points, np.float64)))
    root = _nearest_segment(graph, shape, seed[0], np.asarray(sp or [1.0, 1.0, 1.0])) if graph["segments"] else None
    return graph, root


def _check_spur_factor(spur_factor):
    if not (np.ndim(spur_factor) == 0 and math.isfinite(float(spur_factor)) and float(spur_factor) >= 0):
        raise ValueError(f"spur_factor: a number >= 0, got {spur_factor!r}")
    return float(spur_factor)


def tree_from_points(shape, index, code, d2_points, lab_points, seed, spacing=None, spur_factor=1.5, pruned=0, skeleton_voxels=None) -> dict:
    """`airway_tree`'s dict from the PRUNED skeleton's point list (raster indices ascending, codes, squared distances in mm^2 and
    labels); `pruned` and `skeleton_voxels`: what the pruning removed and started from."""
    spur_factor = _check_spur_factor(spur_factor)
    sp = None if spacing is None else [float(s) for s in spacing]
    pts = np.asarray(index, np.int64)
    empty = {"spacing_mm": sp, "spur_factor": spur_factor, "root": None, "segments": [], "generations": [],
             "totals": {"segments": 0, "end_points": 0, "deepest_generation": None, "pruned_spurs": int(pruned), "cycles": 0,
                        "skeleton_voxels": int(pts.size if skeleton_voxels is None else skeleton_voxels), "unreached_segments": 0}}
    if pts.size == 0:
        return empty
    label_at = dict(zip(pts.tolist(), np.asarray(lab_points, np.int64).tolist()))
    graph, root = _rooted_graph(shape, pts, np.asarray(code, np.uint8), d2_points, seed, sp)
    if root is None:
        return empty
    segs = {s["id"]: s for s in graph["segments"]}
    # generations: breadth first over the junction clusters from the root
    gen, parent, seen_j, cycles = {root: 0}, {root: None}, set(), 0
    frontier = [root]
    while frontier:
        nxt = []
        for i in frontier:
            for j in segs[i]["ends"]:
                if j is None or j in seen_j:
                    continue
                seen_j.add(j)
                for k in sorted(segs):
                    if k != i and j in segs[k]["ends"]:
                        if k in gen:
                            cycles += 1
                            continue
                        gen[k], parent[k] = gen[i] + 1, i
                        nxt.append(k)
        frontier = nxt
    cycles += sum(1 for s in segs.values() if s["closed"] or (s["ends"][0] is not None and s["ends"][0] == s["ends"][1]))
    out = []
    for i in sorted(segs, key=lambda i: (gen.get(i, 1 << 30), i)):
        s = segs[i]
        out.append({"id": i, "generation": gen.get(i), "parent": parent.get(i), "children": sorted(k for k, p in parent.items() if p == i),
                    "voxels": s["voxels"], "length_mm": float(s["length_mm"]), "diameter_mm": float(2.0 * s["radius_mm"]["mean"]),
                    "label": int(label_at[s["first_index"]]), "closed": bool(s["closed"]), "first_index": int(s["first_index"])})
    reached = [s for s in out if s["generation"] is not None]
    gens = []
    for g in range(max(s["generation"] for s in reached) + 1):
        mine = [s for s in reached if s["generation"] == g]
        vox = sum(s["voxels"] for s in mine)
        gens.append({"generation": g, "segments": len(mine), "length_mm": float(sum(s["length_mm"] for s in mine)),
                     "mean_diameter_mm": float(sum(s["diameter_mm"] * s["voxels"] for s in mine) / vox) if vox else None})
    ends = sum(1 for s in reached if not s["closed"] and s["id"] != root and None in segs[s["id"]]["ends"])
    return {"spacing_mm": sp, "spur_factor": spur_factor, "root": root, "segments": out, "generations": gens,
            "totals": {"segments": len(out), "end_points": ends, "deepest_generation": gens[-1]["generation"], "pruned_spurs": int(pruned),
                       "cycles": cycles, "skeleton_voxels": empty["totals"]["skeleton_voxels"], "unreached_segments": len(out) - len(reached)}}


def _graph_with_points(shape, index, code, spacing, radius):
    """`skeleton.graph_from_points` with, per segment, the raster indices of its voxels (`_points`): the graph numbers segments by
    their first voxel and lists none, so the membership is rebuilt as the 26-components of the non-junction voxels."""
    from scipy import ndimage as ndi

    graph = _skeleton.graph_from_points(shape, index, code, spacing, radius)
    n, h, w = (int(s) for s in shape)
    index = np.asarray(index, np.int64)
    plain = index[np.asarray(code, np.uint8) < 4]
    if plain.size:
        z, y, x = plain // (h * w), (plain // w) % h, plain % w
        lo = np.array([z.min(), y.min(), x.min()])
        box = np.zeros((z.max() - lo[0] + 1, y.max() - lo[1] + 1, x.max() - lo[2] + 1), bool)
        box[z - lo[0], y - lo[1], x - lo[2]] = True
        comp = ndi.label(box, structure=np.ones((3, 3, 3), bool))[0][z - lo[0], y - lo[1], x - lo[2]]
        members = {}
        for p, c in zip(plain.tolist(), comp.tolist()):
            members.setdefault(c, []).append(p)
        by_first = {m[0]: m for m in members.values()}  # (ascending raster order: m[0] is the component's first voxel)
    for s in graph["segments"]:
        s["_points"] = by_first[s["first_index"]]
    return graph


MAX_PRUNE_PASSES = 64


def tree_dev(eng, mask_dev, lab_dev, seed, spacing=None, spur_factor=1.5) -> dict:
    """`airway_tree` on a device-resident u8 mask (and labels, or None)."""
    spur_factor = _check_spur_factor(spur_factor)
    shape = tuple(mask_dev.shape)
    sp = None if spacing is None else [float(s) for s in spacing]
    with eng.scope() as dev:
        try:
            skel = dev.add(eng.skeleton_dev(mask_dev)[0])
        except _native.NoKeptVoxel:
            return tree_from_points(shape, [], [], [], [], seed, sp, spur_factor)
        # the radii exactly as the vessel tree gets them: lm_calibre_dev's distance to the complement of the mask
        cls, _, d2 = eng.calibre_dev(skel, mask_dev, [1.0], spacing=sp, return_distance=True)
        dev.add(cls, d2)
        index, code, d2_points, _ = eng.skeleton_points_dev(skel, d2)
        start, pruned, host = int(index.size), 0, None
        for _ in range(MAX_PRUNE_PASSES):
            graph, root = _rooted_graph(shape, index, code, d2_points, seed, sp)
            spurs = _spurs(graph, root, spur_factor) if root is not None else []
            if not spurs:
                break
            # a pass removes the spurs' voxels and thins what is left again: a junction that loses its spurs is no curve yet (the
            # thinning kept its voxels FOR those end points), and only the thinning's own rules keep the topology while it becomes one
            pruned += len(spurs)
            host = skel.download() if host is None else host
            host.reshape(-1)[[p for s in spurs for p in s["_points"]]] = 0
            skel.upload(host)
            eng.skeleton_dev(skel, out=skel)
            host = skel.download()
            index, code, d2_points, _ = eng.skeleton_points_dev(skel, d2)
        lab_points = np.zeros(index.size, np.int64) if lab_dev is None else lab_dev.download().ravel()[index]
    return tree_from_points(shape, index, code, d2_points, lab_points, seed, sp, spur_factor, pruned, start)


def airway_tree(mask, seed, spacing=None, labels=None, spur_factor=1.5, engine=None) -> dict:
    """The airway tree of a mask -> a JSON-serialisable dict: spacing_mm, spur_factor, root, segments, generations, totals.

    `skeletonize(mask)`; the radius at the skeleton points from `lm_edt_dev` on the complement (as the vessel tree's); the graph of
    `skeleton.graph_from_points`.  On the graph, on the host:
    - Root: the segment that holds the skeleton voxel nearest to `seed` ((z, y, x), or a list whose first entry counts).
    - Pruning: repeatedly, the free-ended segments other than the root with length_mm < spur_factor * their largest radius, at a
      junction cluster that joins three segment ends or more, are removed (surface spurs: the thinning keeps every end point).
      Their voxels leave the skeleton and what is left is thinned again (`lm_skeleton_dev`), so the voxels a junction held for
      those end points go as well and the two segments left at a junction of degree two become one.
    - Generation: the root is 0; a segment's generation is the number of junction clusters between it and the root.  A cycle is
      reported, not broken: `closed` segments and totals["cycles"].
    - segments: id, generation, parent, children, voxels, length_mm, diameter_mm (2 x the mean radius), label (of the first voxel, as
      the vessel tree does), closed, first_index.  generations: segments, length_mm, mean_diameter_mm.  totals: segments,
      end_points, deepest_generation, pruned_spurs, cycles, skeleton_voxels, unreached_segments (parts of the mask that do not hang
      on the root's tree; generation None).
    The diameter is twice a distance between voxel centres: for thin airways it overestimates the lumen by up to a voxel."""
    arr = _skeleton._mask_volume(mask)
    seeds = _seed_list(seed)
    lab = None
    if labels is not None:
        lab = _skeleton._mask_volume(labels)
        if lab.shape != arr.shape:
            raise ValueError(f"labels {lab.shape} and mask {arr.shape} must have the same shape")
    sp = None if spacing is None else [float(s) for s in spacing]
    if sp is not None and (len(sp) != 3 or not all(v > 0 and math.isfinite(v) for v in sp)):
        raise ValueError(f"spacing needs three positive values in the array's axis order, got {spacing!r}")
    if arr.size == 0 or not arr.any():
        return tree_from_points(arr.shape, [], [], [], [], seeds, sp, spur_factor)
    with _native.engine_scope(engine) as eng, eng.scope() as dev:
        return tree_dev(eng, dev.upload((arr != 0).astype(np.uint8)), None if lab is None else dev.upload(lab), seeds, sp, spur_factor)


# ---- the segmentation -----------------------------------------------------------------------------------------------------------------
class AirwayResult:
    """What `segment_airways` and `LMInferer.apply_with_airways` return: `mask` uint8 [n][h][w] (1 = airway), `cost` int16 [n][h][w]
    (`minimax_cost`), `threshold` (HU, or None when nothing was segmented), `seed` (the (z, y, x) the flood started from, a list),
    `curve` (int64, the flood's histogram), `analysis` (a JSON-serialisable dict) and `tree` (`airway_tree`'s dict)."""

    def __init__(self, mask, cost, threshold, seed, curve, analysis, tree):
        self.mask, self.cost, self.threshold, self.seed, self.curve, self.analysis, self.tree = mask, cost, threshold, seed, curve, analysis, tree

    def meta(self) -> dict:
        """analysis and tree as one JSON-serialisable dict."""
        return {"analysis": self.analysis, "tree": self.tree}


def check_arguments(cap_hu=DEFAULT_CAP_HU, threshold=None, seed=None, spur_factor=1.5, **rule_kw):
    """The host checks of `segment_airways`, before anything runs -> (cap, threshold, seeds or None, rule keywords)."""
    cap = _check_cap(cap_hu)
    if threshold is not None and (np.ndim(threshold) != 0 or int(threshold) != threshold or not -1024 <= threshold <= cap):
        raise ValueError(f"threshold: None or an integer in -1024 .. cap_hu ({cap}), got {threshold!r}")
    unknown = sorted(set(rule_kw) - set(RULE_DEFAULTS) - {"seed_hu", "min_length_mm", "max_area_mm2"})
    if unknown:
        raise TypeError(f"segment_airways: unknown keyword(s) {unknown}")
    rule = dict(RULE_DEFAULTS, **{k: v for k, v in rule_kw.items() if k in RULE_DEFAULTS})
    choose_threshold(np.zeros(cap + 1025, np.int64), 1.0, **dict(rule, start_hu=min(rule["start_hu"], cap)))  # (its own checks)
    if rule["start_hu"] > cap:
        raise ValueError(f"start_hu ({rule['start_hu']}) must not exceed cap_hu ({cap})")
    trachea = {k: rule_kw[k] for k in ("seed_hu", "min_length_mm", "max_area_mm2") if k in rule_kw}
    _check_trachea_arguments(trachea.get("seed_hu", -950), trachea.get("min_length_mm", 20.0), trachea.get("max_area_mm2", 600.0))
    _check_spur_factor(spur_factor)
    return cap, None if threshold is None else int(threshold), None if seed is None else _seed_list(seed), rule, trachea


def empty_result(shape, error, params, trachea=None, spacing=None) -> AirwayResult:
    """Nothing was segmented: zeros, an unreached cost and the reason in analysis["error"]."""
    sp = None if spacing is None else [float(s) for s in spacing]
    analysis = {"parameters": params, "spacing_mm": sp, "trachea": trachea, "seed": None, "threshold": None, "first_leaking": None,
                "rounds": 0, "reached": 0, "voxels": 0, "volume_ml": 0.0 if sp is not None else None, "by_label": {}, "error": str(error)}
    return AirwayResult(np.zeros(shape, np.uint8), np.full(shape, UNREACHED, np.int16), None, None, np.zeros(0, np.int64), analysis,
                        tree_from_points(shape, [], [], [], [], [(0, 0, 0)], sp, params.get("spur_factor", 1.5)))


def airways_dev(eng, vol_dev, lab_dev, seed=None, cap_hu=DEFAULT_CAP_HU, threshold=None, spacing=None, names=None, spur_factor=1.5,
                **rule_kw) -> AirwayResult:
    """`segment_airways` on device-resident image and labels (u8; None: no labels); the volumes are brought to the host once."""
    cap, threshold, seeds, rule, trachea_kw = check_arguments(cap_hu, threshold, seed, spur_factor, **rule_kw)
    shape = tuple(vol_dev.shape)
    sp = None if spacing is None else [float(s) for s in spacing]
    voxel_ml = 1e-3 if sp is None else float(np.prod(sp)) / 1000.0  # (without a spacing a voxel is 1 mm^3)
    params = dict(rule, cap_hu=cap, spur_factor=float(spur_factor), explicit_threshold=threshold, explicit_seed=seeds is not None, **trachea_kw)
    trachea = None
    if seeds is None:
        try:
            trachea = trachea_dev(eng, vol_dev, lab_dev, spacing=sp, **trachea_kw)
        except NoTrachea as exc:
            return empty_result(shape, exc, params, None, sp)
        seeds = [tuple(trachea["index"])]
        trachea = {k: trachea[k] for k in ("index", "component", "rejected", "components")} | {"candidates": trachea["candidates"][:8]}
        trachea["index"] = list(trachea["index"])
    with eng.scope() as dev:
        cost, curve, info = eng.seed_cost_dev(vol_dev, seeds, cap)
        dev.add(cost)
        chosen = choose_threshold(curve, voxel_ml, **rule)
        t = threshold if threshold is not None else chosen["threshold"]
        if t is None:
            why = "the seed is not air below cap_hu" if info["seeds_passable"] == 0 else \
                f"the region leaks at the first tested threshold ({chosen['first_leaking']} HU): is the trachea open to outside air?"
            r = empty_result(shape, f"segment_airways: no threshold: {why}", params, trachea, sp)
            r.cost, r.curve, r.seed = cost.download(), curve, [list(s) for s in seeds]
            r.analysis.update(seed=r.seed, first_leaking=chosen["first_leaking"], rounds=info["rounds"], reached=info["reached"])
            return r
        mask, counts = eng.airway_mask_dev(cost, t, lab=lab_dev)
        dev.add(mask)
        tree = tree_dev(eng, mask, lab_dev, seeds, sp, spur_factor)
        names = dict(names or {})
        by_label = {str(k): {"name": "outside the labels" if k == 0 else names.get(k, f"label {k}"), "voxels": int(counts[k]),
                             "volume_ml": int(counts[k]) * voxel_ml if sp is not None else None}
                    for k in range(256) if counts[k] or (k and k in names)}
        voxels = int(counts.sum())
        analysis = {"parameters": params, "spacing_mm": sp, "trachea": trachea, "seed": [list(s) for s in seeds], "threshold": int(t),
                    "first_leaking": chosen["first_leaking"], "rule_threshold": chosen["threshold"], "rounds": info["rounds"],
                    "reached": info["reached"], "voxels": voxels, "volume_ml": voxels * voxel_ml if sp is not None else None,
                    "by_label": by_label, "curve": chosen["curve"], "error": None}
        return AirwayResult(mask.download(), cost.download(), int(t), [list(s) for s in seeds], curve, analysis, tree)


def segment_airways(image, labels=None, seed=None, cap_hu=DEFAULT_CAP_HU, threshold=None, spacing=None, names=None, engine=None,
                    spur_factor=1.5, **rule_kw) -> AirwayResult:
    """The airways of a chest CT -> AirwayResult (mask, cost, threshold, seed, curve, analysis, tree).

    `seed`: (z, y, x) or a list of them; None: `find_trachea(image, labels)`.  The flood (`minimax_cost`) runs once up to `cap_hu`;
    `threshold` (HU) skips the rule, otherwise `choose_threshold` picks it from the curve (`rule_kw`: its start_hu, step_hu,
    leak_ratio, leak_ml, max_ml, and find_trachea's seed_hu, min_length_mm, max_area_mm2).  mask = cost <= threshold.  `analysis`:
    parameters, trachea (the winning candidate and up to eight candidates), seed, threshold, first_leaking, rule_threshold, rounds
    and reached (of the flood), voxels, volume_ml, by_label ("0": outside the lung labels, i.e. trachea and main bronchi; the
    others by `names`), the sampled curve, and error (None).  A volume in which no trachea is found raises NoTrachea here
    (`LMInferer.apply_with_airways` returns an empty result instead); no usable threshold gives an empty mask with the reason in
    analysis["error"].  Without a spacing a voxel counts as 1 mm^3 for the rule and volume_ml is None.  One global threshold, no
    leak repair; the defaults are conventional and not validated on patient data (see the module's head)."""
    r = segment_or_empty(image, labels, seed, cap_hu, threshold, spacing, names, engine, spur_factor, **rule_kw)
    if seed is None and r.analysis["trachea"] is None:
        raise NoTrachea(r.analysis["error"])
    return r


def segment_or_empty(image, labels=None, seed=None, cap_hu=DEFAULT_CAP_HU, threshold=None, spacing=None, names=None, engine=None,
                     spur_factor=1.5, **rule_kw) -> AirwayResult:
    """`segment_airways` that returns the empty result with the reason in analysis["error"] where that raises NoTrachea."""
    check_arguments(cap_hu, threshold, seed, spur_factor, **rule_kw)
    arr, lab, sp = _filters._inputs(image, labels, spacing)
    if arr.size == 0:
        return empty_result(arr.shape, "segment_airways: the volume is empty", dict(cap_hu=cap_hu, spur_factor=spur_factor), None, sp)
    with _native.engine_scope(engine) as eng, eng.scope() as dev:
        return airways_dev(eng, dev.upload(arr), None if lab is None else dev.upload(lab), seed, cap_hu, threshold, sp, names, spur_factor, **rule_kw)
