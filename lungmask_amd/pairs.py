"""Paired-CT analysis on the GPU: two CTs of one patient compared voxel by voxel through a transform of
`lungmask_amd.registration` / `lungmask_amd.deformable` -- the parametric response map of an inspiration / expiration pair, the
mass-corrected density change of a baseline / follow-up pair and the mean Jacobian (ventilation, volume change) per label.

One device call (lm_pair_map_dev, include/lungmask_hip.h) streams the fixed grid once: per voxel of a kept label the fixed HU f, the
moving HU m sampled trilinearly through the transform, and J, the Jacobian determinant of the whole transform (the field's, times
the absolute determinant of the affine's matrix), give

  the class     1 + (f < fixed_threshold) + 2 * (m < moving_threshold) where both f and m lie in `hu_range` (0 elsewhere);
  the change    J (m - air) + air - f: the moving density carried onto the fixed voxel with its mass kept -- lung that is more
                inflated is less dense without being more diseased (the "sponge model"; HU - air is proportional to density);
  the Jacobian  J: above 1 the voxel's neighbourhood is larger in the moving image

and an integer table per label from which every figure of the analysis follows exactly.  `roles` names the images: for
("inspiration", "expiration") the thresholds are -950 / -856 HU and the classes 1 .. 4 are normal, uncategorised, fsad (functional
small-airways disease: not emphysema on inspiration, air trapping on expiration) and emphysema; the swapped pair swaps thresholds and
the two middle names; `roles=None` is a longitudinal pair with -950 HU for both and the classes neither, fixed_only, moving_only, both.

Two things this module does NOT do.  PRM is customarily computed after a 3 x 3 x 3 median filter: `filters.median` does that, and
the caller applies it to both images first.  The class thresholds and the -1000 .. -500 HU window are the conventional ones; nothing
here validates them clinically."""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import numpy as np

from . import _native
from . import resample as rs

MAP_NAMES = ("classes", "change", "jacobian")
ROLE_CLASSES = {
    ("inspiration", "expiration"): ((-950.0, -856.0), ("normal", "uncategorised", "fsad", "emphysema")),
    ("expiration", "inspiration"): ((-856.0, -950.0), ("normal", "fsad", "uncategorised", "emphysema")),
    None: ((-950.0, -950.0), ("neither", "fixed_only", "moving_only", "both")),
}


class PairAnalysis:
    """What `pair_analysis` returns.  `classes` (uint8: 0 not classified, 1 .. 4 `class_names`), `change` (float32, HU) and `jacobian`
    (float32) on the fixed grid in the caller's orientation, each None when it was not asked for; `analysis`: the JSON-serialisable
    dict (parameters, `labels` {"k": row}, `lung`: the labels >= 1 together); `table`: the device's integer table
    [n_labels][_native.LM_PAIR_COLS]."""

    def __init__(self, analysis: dict, table: np.ndarray, class_names, classes=None, change=None, jacobian=None):
        self.analysis, self.table, self.class_names = analysis, table, tuple(class_names)
        self.classes, self.change, self.jacobian = classes, change, jacobian


def check_arguments(roles=("inspiration", "expiration"), fixed_threshold=None, moving_threshold=None, hu_range=(-1000, -500), air_hu=-1000.0,
                    keep=None, n_labels=None, maps=MAP_NAMES) -> dict:
    """The analysis arguments checked (ValueError) and resolved -> the keyword arguments of `Engine.pair_map_dev` plus "roles",
    "class_names" and "maps"."""
    key = None if roles is None else tuple(roles) if isinstance(roles, (tuple, list)) else roles
    if key not in ROLE_CLASSES:
        raise ValueError(f"roles: ('inspiration', 'expiration'), ('expiration', 'inspiration') or None, got {roles!r}")
    (fthr, mthr), names = ROLE_CLASSES[key]
    fthr = fthr if fixed_threshold is None else float(fixed_threshold)
    mthr = mthr if moving_threshold is None else float(moving_threshold)
    try:
        lo, hi = (float(v) for v in hu_range)
    except (TypeError, ValueError):
        raise ValueError(f"hu_range: (lo, hi), got {hu_range!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise ValueError(f"hu_range: finite lo <= hi, got {hu_range!r}")
    for name, t in (("fixed_threshold", fthr), ("moving_threshold", mthr)):
        if not lo <= t <= hi:  # (also a NaN)
            raise ValueError(f"{name} {t!r} lies outside hu_range {(lo, hi)}: one class could never occur")
    if not math.isfinite(float(air_hu)):
        raise ValueError(f"air_hu: a finite HU value, got {air_hu!r}")
    if n_labels is not None and (int(n_labels) != n_labels or not 1 <= int(n_labels) <= 16):
        raise ValueError(f"n_labels must lie in 1..16, got {n_labels!r}")
    unknown = set(maps) - set(MAP_NAMES)
    if unknown:
        raise ValueError(f"maps: any of {MAP_NAMES}, got {sorted(unknown)}")
    if keep is not None:
        keep = sorted({int(k) for k in keep})
        if any(not 0 <= k <= 255 for k in keep):
            raise ValueError(f"keep: label values in 0..255, got {keep!r}")
    return {"roles": None if key is None else list(key), "class_names": names, "fixed_thr": fthr, "moving_thr": mthr, "lo": lo, "hi": hi,
            "air": float(air_hu), "keep": keep, "n_labels": None if n_labels is None else int(n_labels), "maps": tuple(maps)}


def split_transform(transform):
    """None, an `Affine`, a `Registration`, a `DisplacementField` or a `DeformableRegistration` -> (Affine or None,
    DisplacementField or None): what `warp_image` / `resample_image` would sample through."""
    from . import deformable as lmdef
    from . import registration as lmreg

    if transform is None or isinstance(transform, rs.Affine):
        return transform, None
    if isinstance(transform, lmreg.Registration):
        return transform.transform, None
    if isinstance(transform, lmdef.DeformableRegistration):
        transform = transform.field
    if isinstance(transform, lmdef.DisplacementField):
        return transform.affine, transform
    raise TypeError(f"transform: None, an Affine, a Registration, a DisplacementField or a DeformableRegistration, got {type(transform).__name__}")


def jac_scale(affine: Optional[rs.Affine]) -> float:
    """The volume change of the affine under the field: the absolute determinant of its matrix (1.0 without one)."""
    if affine is None:
        return 1.0
    det = abs(float(np.linalg.det(np.asarray(affine.matrix, np.float64))))
    if not (math.isfinite(det) and det > 0.0):
        raise ValueError("the affine's matrix is singular or not finite")
    return det


def label_count(lab: np.ndarray, n_labels, names) -> int:
    """`n_labels` as given; else max(names) + 1; else the largest label present + 1 -- ValueError when that label is above 15."""
    if n_labels is not None:
        return int(n_labels)
    if names:
        return max(1, min(max(int(k) for k in names) + 1, 16))
    top = int(lab.max()) if lab.size else 0
    if top > 15:
        raise ValueError(f"the labels reach {top}: the table has 16 rows, pass n_labels (labels at or above it are left out) or names")
    return top + 1


def _ratio(num, den):
    return None if not den else num / den


def row_entry(cols: Sequence[int], name, class_names, voxel_ml=None) -> dict:
    """One row of the analysis from the thirteen integer columns of a label (or of a sum of labels).  Derived figures are float64
    from the integers; each is None where its denominator is 0, the volumes also without a spacing."""
    c = [int(v) for v in cols]
    analysed, classified = c[1], sum(c[9:13])
    mean_j = _ratio(c[5] / _native.PAIR_J_Q, analysed)
    ms = _ratio(c[7] / _native.PAIR_C_Q, analysed)
    ml = lambda n: None if voxel_ml is None else n * voxel_ml  # noqa: E731
    return {"name": name, "voxels": c[0], "analysed": analysed, "outside": c[2], "nonfinite": c[3], "folded": c[4], "excluded": c[8],
            "classified": classified,
            "classes": {cn: {"voxels": c[9 + k], "fraction": _ratio(c[9 + k], classified), "ml": ml(c[9 + k])} for k, cn in enumerate(class_names)},
            "mean_jacobian": mean_j, "mean_change_hu": _ratio(c[6] / _native.PAIR_C_Q, analysed),
            "rms_change_hu": None if ms is None else math.sqrt(ms),
            "volume_fixed_ml": ml(c[0]), "volume_moving_ml": None if mean_j is None or voxel_ml is None else mean_j * analysed * voxel_ml}


def analysis_from_table(table, cfg: dict, names: Optional[Dict[int, str]] = None, spacing=None, jacobian_scale: float = 1.0,
                        transform_kind: Optional[str] = None) -> dict:
    """The JSON-serialisable analysis from the device's integer table [n_labels][LM_PAIR_COLS]: the parameters, `labels` {"k": row}
    for every row, and `lung`, the exact column sum of the rows of the labels >= 1 (every column is a per-voxel sum, so the sum of
    rows IS the row of the union).  `spacing`: the fixed grid's in millimetres (None: no volumes).  A row: see `row_entry`;
    volume_fixed_ml is the label's selected voxels, volume_moving_ml = mean_jacobian x the volume of the analysed ones."""
    rows = [[int(v) for v in row] for row in np.asarray(table).reshape(-1, _native.LM_PAIR_COLS)]
    names = dict(names or {})
    cn = list(cfg["class_names"])
    sp = None if spacing is None else [float(v) for v in spacing]
    voxel_ml = None if sp is None else float(np.prod(sp)) / 1000.0
    labels = {str(k): row_entry(row, "background" if k == 0 else names.get(k, f"label {k}"), cn, voxel_ml) for k, row in enumerate(rows)}
    lung = row_entry([sum(row[c] for row in rows[1:]) for c in range(_native.LM_PAIR_COLS)], "lung", cn, voxel_ml)
    return {"roles": cfg["roles"], "class_names": cn, "fixed_threshold": cfg["fixed_thr"], "moving_threshold": cfg["moving_thr"],
            "hu_range": [cfg["lo"], cfg["hi"]], "air_hu": cfg["air"], "jac_scale": float(jacobian_scale), "transform": transform_kind,
            "keep": cfg["keep"], "n_labels": len(rows), "spacing_mm": sp, "voxel_volume_ml": voxel_ml, "labels": labels, "lung": lung}


def _kind(affine, field) -> Optional[str]:
    return "deformable" if field is not None else ("affine" if affine is not None else None)


def pair_dev(eng, fixed_dev, lab_dev, moving_dev, field_dev, fixed_grid: rs.Grid, moving_grid: rs.Grid, affine: Optional[rs.Affine], scope,
             cfg: dict, n_labels: int):
    """The device call on device-resident pieces -> (table DeviceArray, {map name: DeviceArray}, jac_scale), all owned by `scope`
    and enqueued on the engine's stream.  `field_dev`: float32 [3, *fixed shape] in millimetres along the fixed grid's array axes,
    or None; `affine`: the transform under it, from the fixed to the moving space."""
    from . import deformable as lmdef

    A, b = rs.index_map(moving_grid, fixed_grid, affine)
    scale = jac_scale(affine)
    table = scope.empty((int(n_labels), _native.LM_PAIR_COLS), np.int64)
    out = {name: scope.empty(fixed_dev.shape, np.uint8 if name == "classes" else np.float32) for name in cfg["maps"]}
    eng.pair_map_dev(fixed_dev, lab_dev, moving_dev, field_dev, A, b, table, n_labels, spacing=lmdef.spacing_zyx(fixed_grid), jac_scale=scale,
                     air=cfg["air"], fixed_thr=cfg["fixed_thr"], moving_thr=cfg["moving_thr"], lo=cfg["lo"], hi=cfg["hi"], keep=cfg["keep"],
                     classes=out.get("classes"), change=out.get("change"), jacobian=out.get("jacobian"))
    return table, out, scale


def collect(table_dev, out_dev: dict, cfg: dict, names, spacing, scale: float, kind) -> PairAnalysis:
    """Downloads what `pair_dev` enqueued (the caller has synchronised) -> PairAnalysis."""
    table = table_dev.download()
    maps = {name: arr.download() for name, arr in out_dev.items()}
    return PairAnalysis(analysis_from_table(table, cfg, names, spacing, scale, kind), table, cfg["class_names"], maps.get("classes"),
                        maps.get("change"), maps.get("jacobian"))


def pair_analysis(fixed, moving, labels, transform=None, roles=("inspiration", "expiration"), fixed_threshold=None, moving_threshold=None,
                  hu_range=(-1000, -500), air_hu=-1000.0, keep=None, n_labels=None, names=None, maps=MAP_NAMES, spacing=None,
                  moving_spacing=None, engine=None) -> PairAnalysis:
    """The paired analysis of `fixed` and `moving` (numpy [n, h, w], `volume_io.Volume`s or SimpleITK images) inside `labels` (u8-valued,
    on `fixed`'s grid: a mask from `apply`), on the GPU -> `PairAnalysis`; the module docstring has the definitions.

    `transform`: None, an `Affine`, a `registration.Registration`, a `deformable.DisplacementField` or a
    `deformable.DeformableRegistration`, from the fixed to the moving space, used exactly as `warp_image` / `resample_image` use it
    (a field's grid is the fixed grid).  The Jacobian is the field's determinant times the absolute determinant of the affine's
    matrix.  `roles`: ("inspiration", "expiration") (thresholds -950 / -856 HU; classes normal, uncategorised, fsad, emphysema),
    the swapped pair (thresholds swapped; normal, fsad, uncategorised, emphysema) or None, a longitudinal pair (-950 for both;
    neither, fixed_only, moving_only, both).  `fixed_threshold`, `moving_threshold`: override the role's; "low" is value <
    threshold.  `hu_range`: a voxel is classified when both values lie inside it.  `air_hu`: the HU of zero density of the mass
    correction.  `keep`: the label values analysed (None: every label >= 1); `n_labels` (1..16): rows of the table, labels at or
    above it are left out (default: max(names) + 1, else the largest label + 1; ValueError above 15).  `names`: {k: name}.
    `maps`: which of "classes", "change", "jacobian" are computed and returned.  `spacing`, `moving_spacing`: numpy inputs only,
    in the array's axis order (None: unit voxels, volumes are None).

    `.analysis` holds the parameters, per label and for `lung` (the labels >= 1 together, the exact sum of their rows): voxels,
    analysed, outside (the transform leaves the moving image), nonfinite, folded (J <= 0), excluded (analysed, outside hu_range),
    classified, classes {name: {voxels, fraction of classified, ml}}, mean_jacobian, mean_change_hu, rms_change_hu,
    volume_fixed_ml and volume_moving_ml = mean_jacobian x the volume of the analysed voxels; None where a denominator is 0.

    PRM is customarily computed after a 3 x 3 x 3 median filter (`filters.median`): apply it to both images first.  The thresholds
    and the -1000 .. -500 HU window are conventional; nothing here validates them clinically."""
    from . import deformable as lmdef

    cfg = check_arguments(roles, fixed_threshold, moving_threshold, hu_range, air_hu, keep, n_labels, maps)
    affine, field = split_transform(transform)
    fv, mv, lab = rs._image_array(fixed), rs._image_array(moving), rs._label_u8(labels)
    if lab.shape != fv.shape:
        raise ValueError(f"labels {lab.shape} must have the fixed volume's shape {fv.shape}")
    fixed_grid = rs.Grid.of(fixed if not isinstance(fixed, np.ndarray) else fv, spacing)
    if field is not None:
        if tuple(field.grid.shape) != tuple(fv.shape):
            raise ValueError(f"the field's grid {tuple(field.grid.shape)} must have the fixed volume's shape {fv.shape}")
        fixed_grid = field.grid
    moving_grid = rs.Grid.of(moving if not isinstance(moving, np.ndarray) else mv, moving_spacing)
    rows = label_count(lab, cfg["n_labels"], names)
    has_mm = field is not None or rs._has_geometry(fixed, spacing)
    with _native.engine_scope(engine) as eng:
        with eng.scope() as dev:
            table, out, scale = pair_dev(eng, dev.upload(fv), dev.upload(lab), dev.upload(mv), dev.upload(field.array) if field is not None else None,
                                         fixed_grid, moving_grid, affine, dev, cfg, rows)
            eng.sync()
            return collect(table, out, cfg, names, lmdef.spacing_zyx(fixed_grid) if has_mm else None, scale, _kind(affine, field))
