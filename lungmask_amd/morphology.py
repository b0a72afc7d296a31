"""Label morphology on the GPU: dilation, erosion, opening and closing of a label selection by a ball of a radius in millimetres,
the nearest-label transform underneath them, and label propagation (not in the reference: what callers run `scipy.ndimage` on the
finished mask for -- closing a lung mask over juxta-pleural nodules, a "core" region free of pleura, growing a lobe, giving every
unlabelled voxel of a region the label of the nearest lobe).

The device passes (`lm_nearest_label_dev`, `lm_morph_dev`, lungmask_amd/csrc/morph_kernels.hip) follow the definitions in
include/lungmask_hip.h.  With S the voxels whose label is in `keep`, d(v, X) the exact float32 squared Euclidean distance (mm^2 with a
spacing, voxels^2 without) of voxel v to the set X, and r2 = float32(radius_mm^2):

- D(X) = {v : d(v, X) <= r2};  E(X) = {v in X : d(v, volume minus X) > r2}.  Outside the volume there are no voxels: the volume's
  border does not erode.  Closing is extensive and idempotent, opening anti-extensive and idempotent, exactly.
- nearest_label: per voxel the label of the nearest voxel of S.  Equal distances take the smaller label, pass by pass (x, then y,
  then z), as the header's recursion has it.
- dilate: a voxel of D(S) outside S whose label is in `into` takes its nearest label; erode: a voxel of S outside E(S) becomes 0;
  open: a voxel of S outside D(E(S)) becomes 0; close: a voxel of E(D(S)) outside S whose label is in `into` takes the nearest label
  of S.  The selection is closed / opened AS A WHOLE; new voxels go to the nearest lung or lobe.  radius_mm == 0 is the identity.
- propagate: the dilation with an infinite radius (`max_mm`: a finite one) -- every `into` voxel takes the nearest kept label.

Everything is in the caller's array orientation (no LPS re-orientation), as the statistics are.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

from . import _native


def check_arguments(op, radius_mm, sp, keep, into):
    """The argument errors of the operators, raised before anything runs on the device."""
    if op not in _native.MORPH_OPS:
        raise ValueError(f"op: one of {sorted(_native.MORPH_OPS)}, got {op!r}")
    r = float(radius_mm)
    if not r >= 0 or (math.isinf(r) and op != "dilate"):
        raise ValueError(f"radius_mm must be >= 0 and finite, got {radius_mm!r}")
    if sp is not None and (len(sp) != 3 or not all(v > 0 and math.isfinite(v) for v in sp)):
        raise ValueError(f"spacing needs three positive values in the array's axis order, got {sp!r}")
    _native.Engine._keep_table(keep)
    _native.Engine._into_table(into)


def label_input(labels, spacing=None):
    """(labels u8 C-contiguous [n][h][w], spacing in array axis order or None) of a numpy integer array, a volume_io.Volume or a
    SimpleITK image.  `spacing` may only be given for a numpy array: the images carry their own."""
    from . import stats as st

    arr, sp, _ = st.geometry(labels, spacing)
    arr = np.asarray(arr)
    if arr.ndim != 3:
        raise ValueError(f"labels must be a 3-D volume (got shape {arr.shape})")
    if arr.dtype.kind not in "iub":
        raise ValueError(f"labels must be an integer label volume (got {arr.dtype})")
    if arr.dtype != np.uint8 and arr.size and (arr.min() < 0 or arr.max() > 255):
        raise ValueError("labels must lie in 0..255")
    if sp is not None and (len(sp) != 3 or not all(v > 0 and math.isfinite(v) for v in sp)):
        raise ValueError(f"spacing needs three positive values in the array's axis order, got {sp!r}")
    return np.ascontiguousarray(arr.astype(np.uint8, copy=False)), sp


def nearest_label(labels, spacing=None, keep=None, return_distance: bool = False, engine=None):
    """uint8 [n][h][w]: per voxel the label of the nearest voxel of `labels` (numpy integer array, `volume_io.Volume` or SimpleITK
    image) whose value is in `keep` (label values 1..255; None: every label >= 1) -- 0 everywhere when there is none.  With
    `return_distance` -> (nearest, distance): the float32 Euclidean distance to it as well (mm with a spacing, voxels without; the
    root of lm_edt_dev's squared distance).  `spacing`: numpy input only, in the array's axis order.  `engine`: a _native.Engine
    (default: a new one on device 0)."""
    lab, sp = label_input(labels, spacing)
    _native.Engine._keep_table(keep)
    if lab.shape[0] == 0:
        return (lab.copy(), np.empty(lab.shape, np.float32)) if return_distance else lab.copy()
    with _native.engine_scope(engine) as eng:
        res = eng.nearest_label(lab, sp, keep, return_distance)
    return (res[0], np.sqrt(res[1])) if return_distance else res


def _operator(op, labels, radius_mm, spacing, keep, into, engine):
    lab, sp = label_input(labels, spacing)
    check_arguments(op, radius_mm, sp, keep, into)
    with _native.engine_scope(engine) as eng:
        return eng.morph(lab, op, radius_mm, spacing=sp, keep=keep, into=into)[0]


def dilate(labels, radius_mm, spacing=None, keep=None, into=(0,), engine=None) -> np.ndarray:
    """The labels with the selection (`keep`: label values, None = every label >= 1) dilated by a ball of `radius_mm` (voxels
    without a spacing): every voxel within that distance of the selection whose label is in `into` takes the label of its nearest
    selected voxel.  ValueError when nothing is selected."""
    return _operator("dilate", labels, radius_mm, spacing, keep, into, engine)


def erode(labels, radius_mm, spacing=None, keep=None, into=(0,), engine=None) -> np.ndarray:
    """The labels with the selection eroded by a ball of `radius_mm`: every selected voxel within that distance of a voxel outside
    the selection (inside the volume) becomes 0.  `into` is accepted for symmetry and not used."""
    return _operator("erode", labels, radius_mm, spacing, keep, into, engine)


def open_(labels, radius_mm, spacing=None, keep=None, into=(0,), engine=None) -> np.ndarray:
    """The labels with the selection opened (eroded, then dilated) by a ball of `radius_mm`: selected voxels that no ball inside the
    selection covers become 0.  `into` is accepted for symmetry and not used."""
    return _operator("open", labels, radius_mm, spacing, keep, into, engine)


def close(labels, radius_mm, spacing=None, keep=None, into=(0,), engine=None) -> np.ndarray:
    """The labels with the selection closed (dilated, then eroded) by a ball of `radius_mm`: holes and clefts narrower than the ball
    are filled, each new voxel (its label in `into`) with the label of its nearest selected voxel."""
    return _operator("close", labels, radius_mm, spacing, keep, into, engine)


def propagate(labels, keep=None, into=(0,), max_mm: Optional[float] = None, spacing=None, engine=None) -> np.ndarray:
    """Every voxel whose label is in `into` takes the label of the nearest voxel whose label is in `keep` (None: every label >= 1),
    however far (`max_mm`: only within that distance)."""
    if max_mm is not None and not float(max_mm) >= 0:
        raise ValueError(f"max_mm must be >= 0 or None, got {max_mm!r}")
    return _operator("dilate", labels, math.inf if max_mm is None else max_mm, spacing, keep, into, engine)
