"""Resampling of images and label volumes onto any grid on the GPU (not in the reference: what callers leave the device for
`SimpleITK.Resample` or `scipy.ndimage.affine_transform` for) -- a mask from another reconstruction of the scan, a ground truth at
another spacing, a follow-up placed onto the baseline by a known transform, a volume brought to isotropic voxels.

Geometry lives on the host and becomes one affine map of indices (`index_map`): source index = A @ output index + b, array axis
order, float64.  The device pass (`lm_resample_dev`, lungmask_amd/csrc/resample_kernels.hip) follows the definition in
include/lungmask_hip.h:

- Domain: an output voxel whose source coordinate c has floor(c_i + 0.5) inside 0 .. e_i - 1 on every axis -- ITK's buffer test,
  [-0.5, e_i - 0.5) -- is inside; every other voxel takes `fill`.  The interpolating modes then clamp c to [0, e_i - 1].
- order 0: nearest neighbour, the raw source value.  order 1: trilinear in float64 (the ROI's lerp).  order 3: cubic B-spline with
  mirror boundaries -- the IBSI / pyradiomics convention for images: a recursive prefilter per axis (x, y, z), then 4 x 4 x 4 taps.
  The spline overshoots at edges and is not clamped.
- labels: "nearest", or "linear" -- the per-label trilinear indicator followed by an argmax (the smaller label on a tie), which
  does not staircase; it equals nearest under a shift by whole voxels.
- dtype float32, float16 (== the float32 result's astype(float16)) or int16 (rint, saturated; integer volumes only).

No anti-alias filter is applied when downsampling: call `filters.gaussian` first.  Nothing in this module is a registration:
transforms are given, `align_centroids` only offers a starting translation; `lungmask_amd.registration` finds one.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

from . import _native


class Grid:
    """A voxel grid in LPS physical space: `shape` in array axis order (z, y, x); `spacing` and `origin` in (x, y, z) order and
    `direction` 3 x 3 as SimpleITK and `volume_io.Volume` keep them.  The physical point of array index (k, j, i) is
    origin + direction @ (spacing * (i, j, k))."""

    def __init__(self, shape, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), direction=None):
        self.shape = tuple(int(v) for v in shape)
        self.spacing = tuple(float(v) for v in spacing)
        self.origin = tuple(float(v) for v in origin)
        self.direction = np.eye(3) if direction is None else np.asarray(direction, np.float64).reshape(3, 3).copy()
        if len(self.shape) != 3 or min(self.shape) < 1:
            raise ValueError(f"Grid: three extents >= 1 are needed, got {shape!r}")
        if len(self.spacing) != 3 or not all(v > 0 and math.isfinite(v) for v in self.spacing):
            raise ValueError(f"Grid: three positive spacings are needed, got {spacing!r}")
        if len(self.origin) != 3 or not np.all(np.isfinite(self.direction)) or not all(math.isfinite(v) for v in self.origin):
            raise ValueError("Grid: origin (3 values) and direction (3 x 3) must be finite")

    @classmethod
    def of(cls, image, spacing=None) -> "Grid":
        """The grid of a `volume_io.Volume`, a SimpleITK image, a `Grid`, or a numpy array with `spacing=` in the array's axis
        order (origin 0, identity direction; no spacing: unit voxels)."""
        from . import volume_io

        if isinstance(image, Grid):
            return image
        if isinstance(image, np.ndarray):
            if image.ndim != 3:
                raise ValueError(f"a 3-D volume is needed, got shape {image.shape}")
            sp = (1.0, 1.0, 1.0) if spacing is None else tuple(float(v) for v in spacing)
            if len(sp) != 3:
                raise ValueError(f"spacing needs one value per array axis (3), got {spacing!r}")
            return cls(image.shape, sp[::-1])
        if spacing is not None:
            raise ValueError("spacing is taken from the image (Volume / SimpleITK image): do not pass it as well")
        if isinstance(image, volume_io.Volume):
            return cls(image.array.shape, image.spacing, image.origin, image.direction)
        return cls(tuple(image.GetSize())[::-1], image.GetSpacing(), image.GetOrigin(), np.asarray(image.GetDirection(), np.float64).reshape(3, 3))

    @classmethod
    def isotropic(cls, image, spacing_mm, spacing=None) -> "Grid":
        """The physical box and direction of `image` with new spacing `spacing_mm` (one value, or three in array axis order):
        N_i = floor((e_i - 1) * s_i / t_i) + 1, the ROI's rule -- the first voxel stays where it is."""
        g = cls.of(image, spacing)
        t = [float(spacing_mm)] * 3 if np.ndim(spacing_mm) == 0 else [float(v) for v in spacing_mm]
        if len(t) != 3 or not all(v > 0 and math.isfinite(v) for v in t):
            raise ValueError(f"spacing_mm: one positive value or three in the array's axis order, got {spacing_mm!r}")
        s = g.spacing[::-1]
        shape = [int(math.floor((g.shape[i] - 1) / (t[i] / s[i]))) + 1 for i in range(3)]
        return cls(shape, t[::-1], g.origin, g.direction)

    def like(self, array: np.ndarray):
        """`array` (of the grid's shape) as a `volume_io.Volume` on this grid."""
        from . import volume_io

        if tuple(array.shape) != self.shape:
            raise ValueError(f"Grid.like: the array has shape {tuple(array.shape)}, the grid {self.shape}")
        return volume_io.Volume(array, self.spacing, self.origin, self.direction)

    def index_to_physical(self, idx_zyx) -> np.ndarray:
        return np.asarray(self.origin) + self.direction @ (np.asarray(idx_zyx, np.float64)[::-1] * np.asarray(self.spacing))

    def same_as(self, other: "Grid", rtol: float = 1e-5) -> bool:
        """Equal shape, and spacing, direction and origin equal within `rtol` (the origin: within rtol of a voxel)."""
        return (self.shape == other.shape and np.allclose(self.spacing, other.spacing, rtol=rtol, atol=0.0)
                and np.allclose(self.direction, other.direction, rtol=rtol, atol=rtol)
                and np.allclose(self.origin, other.origin, rtol=0.0, atol=rtol * min(self.spacing)))

    def meta(self) -> dict:
        return {"shape": list(self.shape), "spacing_mm": list(self.spacing[::-1]), "origin": list(self.origin),
                "direction": [float(v) for v in self.direction.reshape(-1)]}

    def __repr__(self):
        return f"Grid(shape={self.shape}, spacing={self.spacing}, origin={self.origin}, direction={self.direction.tolist()})"


class Affine:
    """An affine transform p -> matrix @ p + translation of LPS millimetres.  As a resampling transform it maps a physical point of
    the OUTPUT grid to the physical point of the SOURCE that is sampled there -- ITK's resampling convention (`ResampleImageFilter`:
    the transform goes from the output space to the input space).  Moving the content by +d therefore takes `Affine.translation(-d)`."""

    def __init__(self, matrix=None, translation=None):
        self.matrix = np.eye(3) if matrix is None else np.asarray(matrix, np.float64).reshape(3, 3).copy()
        self.translation_vector = np.zeros(3) if translation is None else np.asarray(translation, np.float64).reshape(3).copy()

    @classmethod
    def identity(cls) -> "Affine":
        return cls()

    @classmethod
    def translation(cls, offset) -> "Affine":
        return cls(None, offset)

    @classmethod
    def rotation(cls, axis, degrees: float, centre=(0.0, 0.0, 0.0)) -> "Affine":
        """The rotation by `degrees` about the direction `axis` (right-handed) through the point `centre`."""
        u = np.asarray(axis, np.float64).reshape(3)
        norm = float(np.linalg.norm(u))
        if not norm > 0:
            raise ValueError("rotation: the axis must not be the zero vector")
        u = u / norm
        a = math.radians(float(degrees))
        K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
        R = np.eye(3) + math.sin(a) * K + (1.0 - math.cos(a)) * (K @ K)
        c = np.asarray(centre, np.float64).reshape(3)
        return cls(R, c - R @ c)

    @classmethod
    def scale(cls, factors, centre=(0.0, 0.0, 0.0)) -> "Affine":
        """The scaling by `factors` (one value or three, along L, P, S) about `centre`."""
        f = np.full(3, float(factors)) if np.ndim(factors) == 0 else np.asarray(factors, np.float64).reshape(3)
        c = np.asarray(centre, np.float64).reshape(3)
        M = np.diag(f)
        return cls(M, c - M @ c)

    PARAMETERS = {"translation": 3, "rigid": 6, "similarity": 7, "affine": 12}

    @classmethod
    def from_parameters(cls, kind: str, parameters, centre=(0.0, 0.0, 0.0)) -> "Affine":
        """The transform p -> t + c + R @ H @ S @ (p - c) of the registration's parameter vector (lungmask_amd.registration), the one
        place that holds the parameterisation.  `kind`: "translation" (t: 3 values in mm along L, P, S), "rigid" (three angles in
        degrees about the L, P and S axes through `centre` c, R = R_S @ R_P @ R_L, then t), "similarity" (rigid, then one log-scale
        in per cent: S = exp(s / 100) * I) or "affine" (rigid, then three log-scales in per cent along L, P, S and three shears in per
        cent: H = [[1, h0, h1], [0, 1, h2], [0, 0, 1]]).  One unit is one degree, one millimetre or 1 %.  All zeros: the identity."""
        if kind not in cls.PARAMETERS:
            raise ValueError(f"transform: one of {sorted(cls.PARAMETERS)}, got {kind!r}")
        p = np.asarray(parameters, np.float64).reshape(-1)
        if p.size != cls.PARAMETERS[kind]:
            raise ValueError(f"transform {kind!r} takes {cls.PARAMETERS[kind]} parameters, got {p.size}")
        if kind == "translation":
            return cls.translation(p)
        out = cls()
        if kind == "similarity":
            out = cls.scale(math.exp(p[6] / 100.0), centre)
        elif kind == "affine":
            shear = cls(np.array([[1.0, p[9] / 100.0, p[10] / 100.0], [0.0, 1.0, p[11] / 100.0], [0.0, 0.0, 1.0]]))
            c = np.asarray(centre, np.float64).reshape(3)
            shear.translation_vector = c - shear.matrix @ c
            out = shear.compose(cls.scale(np.exp(p[6:9] / 100.0), centre))
        for axis, degrees in zip(np.eye(3), p[:3]):
            out = cls.rotation(axis, degrees, centre).compose(out)
        return cls.translation(p[3:6]).compose(out)

    def compose(self, other: "Affine") -> "Affine":
        """p -> self(other(p)): `other` is applied first."""
        return Affine(self.matrix @ other.matrix, self.matrix @ other.translation_vector + self.translation_vector)

    def inverse(self) -> "Affine":
        inv = np.linalg.inv(self.matrix)
        return Affine(inv, -(inv @ self.translation_vector))

    def apply(self, points) -> np.ndarray:
        """The images of `points` ([..., 3])."""
        return np.asarray(points, np.float64) @ self.matrix.T + self.translation_vector

    def __repr__(self):
        return f"Affine(matrix={self.matrix.tolist()}, translation={self.translation_vector.tolist()})"


def index_map(source_grid: Grid, out_grid: Grid, transform: Optional[Affine] = None):
    """(A [3][3], b [3]) in float64 and array axis order: the source index sampled by output index o is A @ o + b =
    S_src^-1 D_src^T (T(D_out S_out o + O_out) - O_src).  The single place where geometry becomes the device's map."""
    T = transform if transform is not None else Affine()
    flip = np.eye(3)[::-1]  # (z, y, x) <-> (x, y, z)
    to_phys = out_grid.direction @ np.diag(out_grid.spacing) @ flip
    to_index = flip @ np.diag(1.0 / np.asarray(source_grid.spacing)) @ source_grid.direction.T
    with np.errstate(invalid="ignore", over="ignore"):  # (a transform that is not finite is refused below)
        A = to_index @ (T.matrix @ to_phys)
        b = to_index @ (T.matrix @ np.asarray(out_grid.origin) + T.translation_vector - np.asarray(source_grid.origin))
    if not (np.all(np.isfinite(A)) and np.all(np.isfinite(b))):
        raise ValueError("index_map: the geometry or the transform is not finite")
    return np.ascontiguousarray(A, np.float64), np.ascontiguousarray(b, np.float64)


_ORDERS = {0: "nearest", 1: "linear", 3: "cubic"}
_LABEL_MODES = {"nearest": "nearest", "linear": "label_linear"}


def _has_geometry(image, spacing) -> bool:
    return not isinstance(image, np.ndarray) or spacing is not None


def _image_array(image) -> np.ndarray:
    from . import stats as st
    from .mask import LMInferer

    arr = np.asarray(st._label_array(image))
    if arr.ndim != 3 or arr.shape[0] < 1:
        raise ValueError(f"a 3-D volume with at least one slice is needed, got shape {arr.shape}")
    return np.ascontiguousarray(LMInferer._engine_dtype(arr))


def _label_u8(labels) -> np.ndarray:
    from . import metrics
    from . import stats as st

    return metrics._u8(st._label_array(labels), "labels")


def image_dtype(order: int, source_dtype, dtype):
    """The result dtype of `resample_image`: the source's for order 0, else `dtype` (default float32), checked."""
    if order not in _ORDERS:
        raise ValueError(f"order: 0 (nearest), 1 (linear) or 3 (cubic B-spline), got {order!r}")
    if order == 0:
        if dtype is not None and np.dtype(dtype) != np.dtype(source_dtype):
            raise ValueError(f"order 0 returns the source's raw values: dtype must be {np.dtype(source_dtype)} or None")
        return np.dtype(source_dtype)
    dt = np.dtype(np.float32 if dtype is None else dtype)
    if dt not in _native.LM_ROI_DTYPES:
        raise TypeError(f"resample dtype float32, float16 or int16, not {dt}")
    if dt == np.int16 and np.dtype(source_dtype).kind == "f":
        raise ValueError("resample dtype int16 needs an integer volume")
    return dt


def resample_image(image, like, transform: Optional[Affine] = None, order: int = 1, fill=-1024, dtype=None, spacing=None, engine=None):
    """`image` (numpy [n, h, w], a `volume_io.Volume` or a SimpleITK image) resampled onto the grid `like` (a `Grid`, a Volume or
    an image) on the GPU -> a `volume_io.Volume` on that grid, or the bare array when `image` is a numpy array without `spacing`
    (its grid then has unit voxels at the origin).

    `transform`: an `Affine` from the output's physical space to the source's (default: the identity -- both grids describe the
    same space).  `order`: 0, 1 or 3.  `fill`: the value outside the source.  `dtype`: float32 (default), float16 or int16 for
    orders 1 and 3; order 0 keeps the source's.  `spacing`: numpy input only, in the array's axis order.  `engine`: a
    _native.Engine (default: a new one on device 0)."""
    src_grid, out_grid = Grid.of(image, spacing), Grid.of(like)
    vol = _image_array(image)
    dt = image_dtype(order, vol.dtype, dtype)
    A, b = index_map(src_grid, out_grid, transform)
    with _native.engine_scope(engine) as eng:
        out = eng.resample(vol, A, b, out_grid.shape, _ORDERS[order], fill, dt)
    return out_grid.like(out) if _has_geometry(image, spacing) else out


def resample_labels(labels, like, transform: Optional[Affine] = None, mode: str = "nearest", fill=0, spacing=None, engine=None):
    """`labels` (u8-valued: numpy, Volume or SimpleITK image) resampled onto the grid `like` on the GPU -> a Volume of uint8 on
    that grid, or the bare array for a numpy array without `spacing`.  `mode`: "nearest", or "linear" (the per-label trilinear
    indicator and an argmax; the smaller label on a tie).  The other arguments are `resample_image`'s."""
    if mode not in _LABEL_MODES:
        raise ValueError(f"mode: 'nearest' or 'linear', got {mode!r}")
    src_grid, out_grid = Grid.of(labels if not isinstance(labels, np.ndarray) else np.asarray(labels), spacing), Grid.of(like)
    lab = _label_u8(labels)
    if lab.shape[0] < 1:
        raise ValueError("resample_labels: the labels have no slice")
    A, b = index_map(src_grid, out_grid, transform)
    with _native.engine_scope(engine) as eng:
        out = eng.resample(lab, A, b, out_grid.shape, _LABEL_MODES[mode], fill, np.uint8)
    return out_grid.like(out) if _has_geometry(labels, spacing) else out


def align_centroids(fixed_labels, moving_labels, spacing=None, moving_spacing=None, engine=None) -> Affine:
    """The translation `Affine` that places the centroid of every label >= 1 of `moving_labels` onto that of `fixed_labels`, for
    resampling the moving volume onto the fixed grid: it maps the fixed centroid to the moving one.  The centroids come from
    `stats.label_statistics` (centroid_mm; for bare arrays the index centroid times `spacing` / `moving_spacing`, unit voxels without).
    A starting transform, not a registration (`registration.register(..., initial="centroids")` starts from it)."""
    from . import stats as st

    def centroid(labels, sp):
        lab = (_label_u8(labels) > 0).astype(np.uint8)
        grid = Grid.of(labels if not isinstance(labels, np.ndarray) else lab, sp)
        res = st.label_statistics(lab.astype(np.int16), lab, n_labels=2, engine=engine)
        idx = res["labels"]["1"]["centroid_index"]
        if idx is None:
            raise ValueError("align_centroids: a label volume holds no voxel with a label >= 1")
        return grid.index_to_physical(idx)

    return Affine.translation(centroid(moving_labels, moving_spacing) - centroid(fixed_labels, spacing))


class Resampled:
    """What `LMInferer.apply_resampled` returns beside the labels: `image` (the resampled array), `labels` (uint8, the labels on
    the same grid) and `grid` (the `Grid` both lie on)."""

    def __init__(self, image: np.ndarray, labels: np.ndarray, grid: Grid, order: int, label_mode: str, has_geometry: bool):
        self.image = image
        self.labels = labels
        self.grid = grid
        self.order = int(order)
        self.label_mode = label_mode
        self._has_geometry = has_geometry

    def _volume(self, arr):
        if not self._has_geometry:
            raise ValueError("the resampling of a bare numpy array has no geometry (pass spacing=, a Volume or a SimpleITK image)")
        return self.grid.like(arr)

    def as_volume(self):
        """`image` as a `volume_io.Volume` on the grid."""
        return self._volume(self.image)

    def labels_volume(self):
        """`labels` as a `volume_io.Volume` on the grid."""
        return self._volume(self.labels)

    def meta(self) -> dict:
        """The non-array fields, JSON-serialisable."""
        out = self.grid.meta()
        out.update({"dtype": str(self.image.dtype), "order": self.order, "label_mode": self.label_mode})
        return out


def resample_pair_dev(eng, vol_dev, lab_dev, src_grid: Grid, out_grid: Grid, order: int, label_mode: str, fill, dtype, scope):
    """The device-resident volume and labels resampled onto `out_grid` -> (image, labels) as numpy arrays.  `scope`: `add` takes
    the two device results (a _native.DeviceScope or LMInferer's label scope)."""
    A, b = index_map(src_grid, out_grid, None)
    img = scope.add(eng.resample_dev(vol_dev, A, b, out_grid.shape, _ORDERS[order], fill, dtype))
    lab = scope.add(eng.resample_dev(lab_dev, A, b, out_grid.shape, _LABEL_MODES[label_mode], 0, np.uint8))
    eng.sync()
    return img.download(), lab.download()
