"""Deformable registration on the GPU (not in the reference: what callers leave the device for elastix or ANTs for): a dense
displacement field between two scans of the same patient, images and labels warped through it, and its Jacobian determinant -- the
local volume change.  `lungmask_amd.registration` ends at an affine; lungs do not move rigidly.

A `DisplacementField` lives on the FIXED grid: float32 [3][n][h][w], component i the displacement along the grid's array axis i
(z, y, x) in millimetres.  The fixed voxel o samples the moving image at  affine(position(o) + u(o)):  the field is applied first,
in the fixed space, and the affine (from a rigid / affine registration, or the identity) under it.  The device follows the
definitions in include/lungmask_hip.h (lm_warp_dev, lm_demons_step_dev, lm_jacobian_dev; lungmask_amd/csrc/deform_kernels.hip):
float64 arithmetic in a fixed order and integer sums, so results are the same bit for bit on every run.

`register_deformable` is Thirion's additive demons with the force from the fixed image's gradient, on a pyramid:

- Per level, both volumes are smoothed (the Gaussian of `filters.gaussian` as the anti-alias filter, sigma = 0.5 * sqrt((t / s)^2 - 1)
  source voxels for a level spacing t over a native spacing s) and resampled linearly, each onto its own grid (`level_grid`): the
  volume's box with about the level's spacing, never finer than the native one, the first and the last sample of every axis kept.
  The LAST level's spacing is `levels_mm[-1]`, not the native one: the returned field is that level's field upsampled once,
  linearly, onto the fixed grid.
- The field starts from zeros, or from the previous level's field upsampled linearly per component (the field is in millimetres, so
  nothing is rescaled, and every level covers the same box, so nothing is extrapolated).
- An iteration is one `demons_step_dev` (u -> v), one Gaussian pass per component (v -> u, `lm_filter_dev`, sigma `sigma_mm`) and
  one read-back of five integers.  The step of a voxel is d * g / (|g|^2 + d^2 / k^2), d the intensity difference and g the fixed
  gradient per millimetre: its length never exceeds k / 2 = `max_step_mm`.
- The loop of a level ends at its iteration count, or when the mean squared difference -- the exact integer ratio counts[4] /
  (16 * counts[1]) reported BEFORE each step -- has not fallen below its lowest value so far for `patience` iterations in a row
  (compared by cross-multiplication of Python integers), or when no voxel contributes.

Metrics.  `metric="ssd"` (the default) is the squared intensity difference: both images must share an intensity scale (the same
scanner protocol, a follow-up).  Between inspiration and expiration the lung's density changes; for such a pair `metric="lcc"` is
the local correlation metric (lm_local_moments_dev, lm_lcc_step_dev; lungmask_amd/csrc/lcc_kernels.hip): within a window of
`window_mm` the two images are taken to be related by an affine intensity map, the difference d is the residual of that fit and
the force is the gradient of the WARPED MOVING image scaled by the fit's gain.  An "lcc" iteration is one `warp_dev` of the level's
moving volume through the field (linear, NaN outside), the six window sums, one `lcc_step_dev` (u -> v), the three smoothings and
one read-back of six integers; the stop rule runs on the mean squared residual, and the mean squared local correlation is reported
beside it.  Everything else -- the pyramid, the smoothing, the step limit -- is shared.

Scope.  There is no diffeomorphic or fluid variant, no mass-preserving metric.  The defaults are conventional choices
(DESIGN.md has how they were chosen); nothing here validates them clinically.

Fields as operands (lm_field_combine_dev; lungmask_amd/csrc/field_kernels.hip): `invert` (the inverse transform, on the moving grid:
labels of the fixed scan carried onto the moving one, `DeformableRegistration.inverse` / `.resample_to_moving`), `compose` (two
registrations chained into one field) and `inverse_consistency` (how far forward-then-inverse is from the identity).  All three are
one device operation -- a field sampled through another field, rotated, scaled and added -- with the geometry decided here.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np

from . import _native
from . import resample as rs
from .filters import gaussian_taps

# defaults of register_deformable ("Deformable registration" has the experiment behind them)
SIGMA_LEVEL_VOXELS = 1.0     # sigma_mm=None: the field is smoothed by this many voxels of the level
MAX_STEP_LEVEL_VOXELS = 0.5  # max_step_mm=None: the longest step of one iteration, in voxels of the level
DEN_MIN = 1e-9
PATIENCE = 5
METRICS = ("ssd", "lcc")
# defaults of metric="lcc" (picked on a synthetic pair)
WINDOW_LEVEL_VOXELS = 4      # window_mm=None: the window reaches this many voxels of the level to either side
VAR_EPS = 25.0               # added to the window's variance of the moving image per voxel, HU^2
A_MAX = 4.0                  # the largest gain of the window's intensity fit


# ------------------------------------------------------------------------------------------------ the field
def spacing_zyx(grid: rs.Grid):
    """The grid's spacing in array axis order: the unit of the field's components."""
    return tuple(grid.spacing[::-1])


def field_scales(spacing=None):
    """(field_scale, grad_scale) of include/lungmask_hip.h for a spacing in array axis order (None: voxels), float64: 1 / spacing_i
    and half of that."""
    fs = [float(v) for v in _native.Engine.field_scale(spacing)]
    return fs, [v / 2.0 for v in fs]


class DisplacementField:
    """A dense displacement field on the fixed grid.  `array`: float32 [3][n][h][w], millimetres along the array axes z, y, x of
    `grid` (a `resample.Grid`); `affine`: the `resample.Affine` under the field (fixed space -> moving space; None: the identity)."""

    def __init__(self, array, grid, affine: Optional[rs.Affine] = None):
        self.grid = rs.Grid.of(grid)
        arr = np.asarray(array)
        if arr.ndim != 4 or arr.shape[0] != 3 or tuple(arr.shape[1:]) != self.grid.shape:
            raise ValueError(f"DisplacementField: the array must have shape {(3,) + self.grid.shape}, got {arr.shape}")
        if affine is not None and not isinstance(affine, rs.Affine):
            raise TypeError(f"DisplacementField: affine must be a resample.Affine or None, got {type(affine).__name__}")
        self.array = np.ascontiguousarray(arr, dtype=np.float32)
        self.affine = affine if affine is not None else rs.Affine()

    @classmethod
    def zeros(cls, grid, affine: Optional[rs.Affine] = None) -> "DisplacementField":
        g = rs.Grid.of(grid)
        return cls(np.zeros((3,) + g.shape, np.float32), g, affine)

    def lps(self) -> np.ndarray:
        """The vectors in LPS millimetres, float64 [n][h][w][3]: direction @ (u_x, u_y, u_z)."""
        xyz = np.stack([self.array[2], self.array[1], self.array[0]], axis=-1).astype(np.float64)
        return xyz @ self.grid.direction.T

    def meta(self) -> dict:
        """The non-array fields, JSON-serialisable."""
        out = self.grid.meta()
        out.update({"units": "mm", "components": "array axes z, y, x", "matrix": [float(v) for v in self.affine.matrix.reshape(-1)],
                    "translation": [float(v) for v in self.affine.translation_vector]})
        return out

    def save(self, path: str) -> None:
        """`.npz`: the array with the grid and the affine in float64, an exact round trip.  `.nii` / `.nii.gz`: a 4-D float32
        NIfTI-1 with the component as the 4th axis (z, y, x displacement in that order) and the grid's geometry as NIfTI keeps it
        (float32); the affine is not stored."""
        kind = _field_kind(path)
        if kind == "npz":
            with open(path, "wb") as f:  # (np.savez would append ".npz" to a name without it)
                np.savez(f, array=self.array, shape=np.asarray(self.grid.shape, np.int64), spacing=np.asarray(self.grid.spacing, np.float64),
                         origin=np.asarray(self.grid.origin, np.float64), direction=self.grid.direction,
                         matrix=self.affine.matrix, translation=self.affine.translation_vector)
        else:
            from . import volume_io

            volume_io.write_nifti_channels(path, self.grid.like(self.array[0]), self.array)

    @classmethod
    def load(cls, path: str) -> "DisplacementField":
        kind = _field_kind(path)
        if kind == "npz":
            with np.load(path) as z:
                grid = rs.Grid(tuple(int(v) for v in z["shape"]), z["spacing"], z["origin"], z["direction"])
                return cls(z["array"], grid, rs.Affine(z["matrix"], z["translation"]))
        from . import volume_io

        vol, stack = volume_io.read_nifti_channels(path)
        if stack.shape[0] != 3 or stack.dtype != np.float32:
            raise ValueError(f"{path}: a displacement field needs three float32 components, got {stack.shape[0]} of {stack.dtype}")
        return cls(stack, rs.Grid.of(vol))


def _field_kind(path: str) -> str:
    low = str(path).lower()
    if low.endswith(".npz"):
        return "npz"
    if low.endswith(".nii") or low.endswith(".nii.gz"):
        return "nii"
    raise ValueError(f"{path}: a displacement field is saved as .npz, .nii or .nii.gz")


def load(path: str) -> DisplacementField:
    """`DisplacementField.load`."""
    return DisplacementField.load(path)


# ------------------------------------------------------------------------------------------------ warping
def warp_dev(eng, src_dev, field_dev, src_grid: rs.Grid, field_grid: rs.Grid, affine: Optional[rs.Affine], mode: str, fill, dtype, scope,
             out=None):
    """The device-resident `src_dev` on `field_grid` through the field -> DeviceArray.  `mode`: a key of _native.RESAMPLE_MODES;
    "cubic" prefilters `src_dev` here (one float64 volume of the source's size, handed to `scope`)."""
    A, b = rs.index_map(src_grid, field_grid, affine)
    if mode == "cubic":
        src_dev = scope.add(eng.spline_prefilter_dev(src_dev))
    return eng.warp_dev(src_dev, field_dev, A, b, field_grid.shape, mode, fill, dtype, spacing_zyx(field_grid), out=out)


def warp_image(image, field: DisplacementField, order: int = 1, fill=-1024, dtype=None, engine=None, spacing=None):
    """`image` (numpy [n, h, w], a `volume_io.Volume` or a SimpleITK image) on the field's grid, sampled at
    affine(position + displacement), on the GPU -> a `volume_io.Volume` on that grid, or the bare array when `image` is a numpy
    array without `spacing`.  `order` 0, 1 or 3, `fill`, `dtype`: `resample.resample_image`'s.  With a field of zeros the result is
    `resample.resample_image(image, field.grid, field.affine, ...)` bit for bit."""
    if not isinstance(field, DisplacementField):
        raise TypeError(f"warp_image: field must be a DisplacementField, got {type(field).__name__}")
    src_grid = rs.Grid.of(image, spacing)
    vol = rs._image_array(image)
    dt = rs.image_dtype(order, vol.dtype, dtype)
    with _native.engine_scope(engine) as eng:
        with eng.scope() as dev:
            res = dev.add(warp_dev(eng, dev.upload(vol), dev.upload(field.array), src_grid, field.grid, field.affine, rs._ORDERS[order], fill,
                                   dt, dev))
            eng.sync()
            out = res.download()
    return field.grid.like(out) if rs._has_geometry(image, spacing) else out


def warp_labels(labels, field: DisplacementField, mode: str = "nearest", fill=0, engine=None, spacing=None):
    """`labels` (u8-valued) on the field's grid through the field -> a Volume of uint8, or the bare array for a numpy array without
    `spacing`.  `mode`: "nearest", or "linear" (the per-label trilinear indicator and an argmax), as `resample.resample_labels`."""
    if mode not in rs._LABEL_MODES:
        raise ValueError(f"mode: 'nearest' or 'linear', got {mode!r}")
    if not isinstance(field, DisplacementField):
        raise TypeError(f"warp_labels: field must be a DisplacementField, got {type(field).__name__}")
    src_grid = rs.Grid.of(labels if not isinstance(labels, np.ndarray) else np.asarray(labels), spacing)
    lab = rs._label_u8(labels)
    if lab.shape[0] < 1:
        raise ValueError("warp_labels: the labels have no slice")
    with _native.engine_scope(engine) as eng:
        with eng.scope() as dev:
            res = dev.add(warp_dev(eng, dev.upload(lab), dev.upload(field.array), src_grid, field.grid, field.affine, rs._LABEL_MODES[mode],
                                   fill, np.uint8, dev))
            eng.sync()
            out = res.download()
    return field.grid.like(out) if rs._has_geometry(labels, spacing) else out


# ------------------------------------------------------------------------------------------------ Jacobian
def jacobian_determinant(field: DisplacementField, total: bool = False, engine=None):
    """The Jacobian determinant of position -> position + displacement, the local volume change under the field alone (1: none;
    above 1: the voxel's neighbourhood is larger in the moving image) -> (det float32 [n][h][w], {"folded": voxels with det <= 0,
    "nonfinite": voxels with a NaN det, "min": .., "max": ..}, min and max over the finite values).  Central differences inside,
    one-sided at the border (lm_jacobian_dev).  `total`: the map is multiplied on the host by the determinant of the affine's matrix,
    the volume change of the whole transform; the two counts stay those of the field."""
    if not isinstance(field, DisplacementField):
        raise TypeError(f"jacobian_determinant: field must be a DisplacementField, got {type(field).__name__}")
    with _native.engine_scope(engine) as eng:
        det, folded, nan = eng.jacobian(field.array, spacing_zyx(field.grid))
    if total:
        det = (det.astype(np.float64) * float(np.linalg.det(field.affine.matrix))).astype(np.float32)
    finite = det[np.isfinite(det)]
    info = {"folded": int(folded), "nonfinite": int(nan), "min": float(finite.min()) if finite.size else None,
            "max": float(finite.max()) if finite.size else None}
    return det, info


# ------------------------------------------------------------------------------------------------ fields as operands
# One device operation (lm_field_combine_dev, include/lungmask_hip.h) under all of it: a field sampled through another field, rotated,
# scaled and added.  The geometry is decided here, once per function; DESIGN.md 8q has the derivations.
FIELD_RESOLUTION_MM = 2.0 ** -11  # the device reports squared lengths in units of 2^-22 mm^2
MIN_TOLERANCE_MM = 0.001


def _flip():
    return np.eye(3)[::-1]  # (z, y, x) <-> (x, y, z)


def _q_mm(q: int) -> float:
    """The length in millimetres of a squared length in the device's units of 2^-22 mm^2."""
    return math.sqrt(int(q) / float(_native.FIELD_Q))


def _field_figures(counts, voxels: int) -> dict:
    """max_mm, rms_mm (over the voxels that are not `nonfinite`), outside and nonfinite of lm_field_combine_dev's four counts."""
    outside, nan, total, peak = (int(v) for v in counts[:4])
    n = voxels - nan
    return {"max_mm": _q_mm(peak), "rms_mm": math.sqrt(total / float(_native.FIELD_Q) / n) if n > 0 else None, "outside": outside,
            "nonfinite": nan}


def compose_rotation(first_grid: rs.Grid, first_affine: rs.Affine, second_grid: rs.Grid) -> np.ndarray:
    """R of `compose`: the second field's vector (array axes of the second grid) as a vector of the first grid's array axes, pulled
    back through the first affine: flip @ D_1^T @ M_1^-1 @ D_2 @ flip."""
    try:
        inv = np.linalg.inv(first_affine.matrix)
    except np.linalg.LinAlgError:
        raise ValueError("compose: the first field's affine is singular") from None
    R = _flip() @ first_grid.direction.T @ inv @ second_grid.direction @ _flip()
    if not np.all(np.isfinite(R)):
        raise ValueError("compose: the first field's affine is not invertible in float64")
    return R


def compose_dev(eng, first_dev, first_grid: rs.Grid, first_affine: rs.Affine, second_dev, second_grid: rs.Grid, scope, counts=None):
    """The array of `compose` on device-resident fields -> DeviceArray float32 [3, *first_grid.shape] (owned by `scope`).
    `first_dev` None: a field of zeros (the transport of `second_dev` onto `first_grid`)."""
    A, b = rs.index_map(second_grid, first_grid, first_affine)
    R = compose_rotation(first_grid, first_affine, second_grid)
    if first_dev is None:
        first_dev = scope.add(eng.to_device(np.zeros((3,) + first_grid.shape, np.float32)))
    return scope.add(eng.field_combine_dev(second_dev, first_grid.shape, A, b, R, add=first_dev, coord=first_dev, alpha=1.0, beta=1.0,
                                           spacing=spacing_zyx(first_grid), counts=counts))


def _check_fields(who: str, *fields):
    for f in fields:
        if not isinstance(f, DisplacementField):
            raise TypeError(f"{who}: a DisplacementField is needed, got {type(f).__name__}")


def compose(first: DisplacementField, second: DisplacementField, engine=None) -> DisplacementField:
    """The transform "`first`, then `second`":  x -> second(first(x)),  each T_k(x) = affine_k(x + u_k(x)), as ONE field on
    `first.grid` with the affine `second.affine.compose(first.affine)`.  Its array is  u_1 + R u_2(c):  c the index in the second
    grid of first(x) (the second field sampled trilinearly and extended by its edge values) and R = `compose_rotation`.  One device
    call.  `first`'s affine must be invertible."""
    _check_fields("compose", first, second)
    with _native.engine_scope(engine) as eng:
        with eng.scope() as dev:
            fd = dev.upload(first.array)
            sd = fd if second.array is first.array else dev.upload(second.array)
            out = compose_dev(eng, fd, first.grid, first.affine, sd, second.grid, dev)
            eng.sync()
            return DisplacementField(out.download(), first.grid, second.affine.compose(first.affine))


def inverse_consistency(forward: DisplacementField, inverse: DisplacementField, engine=None) -> dict:
    """How far `compose(forward, inverse)` is from the identity: {"max_mm", "rms_mm" (over the voxels that are not `nonfinite`),
    "outside" (voxels of `forward.grid` whose image lies outside `inverse.grid`: the inverse is extended by its edge values there),
    "nonfinite"}, from the device's integer counts -- resolution 2^-11 mm, lengths above 16 mm count as 16.  Only the field of the
    composition is measured: for a `forward` with an affine, `inverse` must carry the inverse affine (as `invert` returns it)."""
    _check_fields("inverse_consistency", forward, inverse)
    with _native.engine_scope(engine) as eng:
        with eng.scope() as dev:
            counts = dev.empty((4,), np.int64)
            fd = dev.upload(forward.array)
            sd = fd if inverse.array is forward.array else dev.upload(inverse.array)
            compose_dev(eng, fd, forward.grid, forward.affine, sd, inverse.grid, dev, counts=counts)
            eng.sync()
            return _field_figures(counts.download(), int(np.prod(forward.grid.shape)))


def check_inversion(iterations, tolerance_mm, affine: Optional[rs.Affine] = None, onto=None):
    """(iterations, the threshold on counts[3]) of `invert`; the ValueErrors of its arguments."""
    identity = affine is None or bool(np.array_equal(affine.matrix, np.eye(3)) and not affine.translation_vector.any())
    if onto is None and not identity:
        raise ValueError("invert: the field has an affine under it, so its inverse lives on the moving grid: pass the moving grid as onto=")
    if int(iterations) != iterations or int(iterations) < 1:
        raise ValueError(f"iterations: a number of iterations >= 1, got {iterations!r}")
    tol = float(tolerance_mm)
    if not (math.isfinite(tol) and tol >= MIN_TOLERANCE_MM):
        raise ValueError(f"tolerance_mm: at least {MIN_TOLERANCE_MM} mm -- the device measures a step with a resolution of 2^-11 = "
                         f"{FIELD_RESOLUTION_MM:.6f} mm -- got {tolerance_mm!r}")
    return int(iterations), int(math.floor(tol * tol * float(_native.FIELD_Q) + 0.5))


def invert_dev(eng, field_dev, grid: rs.Grid, affine: rs.Affine, scope, iterations: int = 30, tolerance_mm: float = 0.01,
               onto: Optional[rs.Grid] = None):
    """`invert` on a device-resident field -> (DeviceArray of the inverse's array, owned by `scope`; its grid; its affine; info)."""
    iterations, threshold = check_inversion(iterations, tolerance_mm, affine, onto)
    sp = spacing_zyx(grid)
    w = scope.add(eng.to_device(np.zeros((3,) + grid.shape, np.float32)))
    nxt = scope.add(eng.empty((3,) + grid.shape, np.float32))
    counts = scope.add(eng.empty((4,), np.int64))
    I, zero = np.eye(3), np.zeros(3)
    residuals, converged, c = [], False, None
    for _ in range(iterations):
        eng.field_combine_dev(field_dev, grid.shape, I, zero, None, coord=w, ref=w, beta=-1.0, spacing=sp, out=nxt, counts=counts)
        eng.sync()
        c = [int(v) for v in counts.download()[:4]]
        w, nxt = nxt, w
        residuals.append(_q_mm(c[3]))
        if c[3] <= threshold:
            converged = True
            break
    fig = _field_figures(c, int(np.prod(grid.shape)))
    info = {"iterations": len(residuals), "converged": converged, "residual_max_mm": fig["max_mm"],
            "residual_rms_mm": fig["rms_mm"], "residuals": residuals, "outside": fig["outside"], "nonfinite": fig["nonfinite"]}
    if onto is None:
        return w, grid, rs.Affine(), info
    inv_affine = affine.inverse()
    return compose_dev(eng, None, onto, inv_affine, w, grid, scope), onto, inv_affine, info


def invert(field: DisplacementField, iterations: int = 30, tolerance_mm: float = 0.01, onto=None, engine=None):
    """The inverse of the transform T(x) = affine(x + u(x)) of `field` -> (DisplacementField, info).

    Step one finds w with (Id + u) o (Id + w) = Id on `field.grid` by the fixed point  w_0 = 0,  w_{k+1} = -u o (Id + w_k),  one
    device call per iteration (u sampled trilinearly, extended by its edge values).  It stops when the longest step of an iteration,
    |w_{k+1} - w_k|, is at most `tolerance_mm` (an integer comparison on the device's count; at least 0.001 mm, the count's
    resolution being 2^-11 mm), or after `iterations`.  Step two, when `onto` (the MOVING grid, anything `Grid.of` takes) is given
    or the field has an affine under it: T^-1 = (Id + w) o affine^-1 as one field on `onto` with the affine `field.affine.inverse()`,
    by `compose`.  A field with an affine and no `onto` is a ValueError: its inverse lives on the moving grid.

    The iteration is a contraction exactly when the largest singular value of the field's gradient (millimetres per millimetre) is
    below 1, and that value is its rate: the steps then shrink by at least that factor per iteration.  A folded field (Jacobian
    determinant <= 0 somewhere) has no inverse and cannot converge: the call then returns `converged: False` and raises nothing.

    `info` (JSON-serialisable): `iterations` run, `converged`, `residual_max_mm` and `residual_rms_mm` (the last
    iteration's step, the RMS over the voxels that are not `nonfinite`), `residuals` (the longest step of every iteration, mm),
    `outside` (voxels whose x + w(x) left the grid in the last iteration) and `nonfinite`."""
    _check_fields("invert", field)
    onto = rs.Grid.of(onto) if onto is not None else None
    check_inversion(iterations, tolerance_mm, field.affine, onto)
    with _native.engine_scope(engine) as eng:
        with eng.scope() as dev:
            out, grid, affine, info = invert_dev(eng, dev.upload(field.array), field.grid, field.affine, dev, iterations, tolerance_mm, onto)
            eng.sync()
            return DisplacementField(out.download(), grid, affine), info


# ------------------------------------------------------------------------------------------------ the stopping rule
class StopRule:
    """The stopping rule of a level on the integer metric (ssd16, contributed) = (counts[4], counts[1]) of each iteration: `update`
    returns None to go on, or the reason to stop after this iteration -- "no overlap" (nothing contributed) or "patience" (the ratio
    has not fallen below its lowest value so far for `patience` iterations in a row).  Ratios are compared by cross-multiplication
    of Python integers: exact."""

    def __init__(self, patience: int):
        if int(patience) != patience or int(patience) < 1:
            raise ValueError(f"patience: a number of iterations >= 1, got {patience!r}")
        self.patience = int(patience)
        self.best = None
        self.stale = 0

    def update(self, metric) -> Optional[str]:
        ssd, n = int(metric[0]), int(metric[1])
        if n <= 0:
            return "no overlap"
        if self.best is None or ssd * self.best[1] < self.best[0] * n:
            self.best, self.stale = (ssd, n), 0
            return None
        self.stale += 1
        return "patience" if self.stale >= self.patience else None


def run_stop_rule(metrics, patience: int, iterations: Optional[int] = None):
    """(iterations run, reason) of a level whose iterations would report `metrics` (a list of (ssd16, contributed))."""
    rule = StopRule(patience)
    limit = len(metrics) if iterations is None else min(int(iterations), len(metrics))
    for k in range(limit):
        why = rule.update(metrics[k])
        if why is not None:
            return k + 1, why
    return limit, "iterations"


# ------------------------------------------------------------------------------------------------ the pyramid
def level_grid(grid: rs.Grid, level_mm: float) -> rs.Grid:
    """The grid of a pyramid level: `grid`'s box, first and last sample of every axis where the grid has them, with
    N_i = min(e_i, round((e_i - 1) * s_i / level_mm) + 1) samples (at least 2 on an axis that has 2) -- a spacing of about `level_mm`,
    never finer than the native one.  Every level so covers exactly the same box: resampling between levels never leaves it."""
    if not (float(level_mm) > 0 and math.isfinite(float(level_mm))):
        raise ValueError(f"levels_mm: spacings > 0, got {level_mm!r}")
    shape, spacing = [], []
    for e, s in zip(grid.shape, spacing_zyx(grid)):
        n = min(e, max(2, int(math.floor((e - 1) * s / float(level_mm) + 0.5)) + 1)) if e > 1 else 1
        shape.append(n)
        spacing.append((e - 1) * s / (n - 1) if n > 1 else s)
    return rs.Grid(shape, spacing[::-1], grid.origin, grid.direction)


def antialias_taps(grid: rs.Grid, level: rs.Grid):
    """The three tap arrays of the anti-alias Gaussian before `grid` is resampled onto `level`: sigma_i = 0.5 * sqrt((t_i / s_i)^2 - 1)
    source voxels (0 where the level is not coarser), taps reaching 4 sigma, 32 voxels at the most."""
    taps = []
    for s, t in zip(spacing_zyx(grid), spacing_zyx(level)):
        ratio = t / s
        sigma = 0.5 * math.sqrt(max(ratio * ratio - 1.0, 0.0))
        truncate = 4.0 if 4.0 * sigma + 0.5 < _native.FILTER_MAX_RADIUS + 1 else _native.FILTER_MAX_RADIUS / sigma
        taps.append(gaussian_taps(sigma, 0, truncate))
    return taps


def field_taps(level: rs.Grid, sigma_mm):
    """The three tap arrays of the field's Gaussian on `level`: `sigma_mm` millimetres (one value or three in array axis order), or
    SIGMA_LEVEL_VOXELS voxels of the level for None."""
    sp = spacing_zyx(level)
    if sigma_mm is None:
        sig = [SIGMA_LEVEL_VOXELS] * 3
    else:
        mm = [float(sigma_mm)] * 3 if np.ndim(sigma_mm) == 0 else [float(v) for v in sigma_mm]
        if len(mm) != 3 or not all(v >= 0 and math.isfinite(v) for v in mm):
            raise ValueError(f"sigma_mm: one value >= 0 or three in the array's axis order, got {sigma_mm!r}")
        sig = [mm[i] / sp[i] for i in range(3)]
    return [gaussian_taps(s, 0, 4.0) for s in sig]


def level_inv_k2(level: rs.Grid, max_step_mm) -> float:
    """inv_k2 of lm_demons_step_dev for a longest step of `max_step_mm` (None: MAX_STEP_LEVEL_VOXELS voxels of the level, the
    smallest spacing): a step is at most k / 2 long, so k = 2 * max_step and inv_k2 = 1 / k^2."""
    step = MAX_STEP_LEVEL_VOXELS * min(level.spacing) if max_step_mm is None else float(max_step_mm)
    if not (step > 0 and math.isfinite(step)):
        raise ValueError(f"max_step_mm: a length > 0, got {max_step_mm!r}")
    return 1.0 / (4.0 * step * step)


def _to_level(eng, vol_dev, grid: rs.Grid, level: rs.Grid, scope):
    """The device-resident volume smoothed and resampled linearly onto `level` -> float32 DeviceArray (owned by the scope)."""
    smooth = eng.filter_dev(vol_dev, kind="separable", taps=antialias_taps(grid, level))
    try:
        A, b = rs.index_map(grid, level, None)
        return scope.add(eng.resample_dev(smooth, A, b, level.shape, "linear", 0.0, np.float32))
    finally:
        eng.sync()
        smooth.free()


def _components(field_dev):
    n = field_dev.nbytes // 3
    return [field_dev.view(i * n, field_dev.shape[1:]) for i in range(3)]


def _upsample_field(eng, field_dev, grid: rs.Grid, onto: rs.Grid, scope):
    """The field on `grid` resampled linearly, per component, onto `onto` -> DeviceArray float32 [3, *onto.shape]."""
    out = scope.add(eng.empty((3,) + onto.shape, np.float32))
    A, b = rs.index_map(grid, onto, None)
    for src, dst in zip(_components(field_dev), _components(out)):
        eng.resample_dev(src, A, b, onto.shape, "linear", 0.0, np.float32, out=dst)
    return out


def _counts(eng, counts_dev):
    eng.sync()
    return [int(v) for v in counts_dev.download()[:5]]


# ------------------------------------------------------------------------------------------------ the local correlation metric
def check_metric(metric, window_mm, var_eps, a_max):
    """The ValueErrors of `register_deformable`'s metric arguments."""
    if metric not in METRICS:
        raise ValueError(f"metric: one of {METRICS}, got {metric!r}")
    if window_mm is not None:
        mm = [window_mm] * 3 if np.ndim(window_mm) == 0 else list(window_mm)
        if len(mm) != 3 or not all(float(v) > 0 and math.isfinite(float(v)) for v in mm):
            raise ValueError(f"window_mm: one length > 0 or three in the array's axis order, got {window_mm!r}")
    if not (float(var_eps) >= 0 and math.isfinite(float(var_eps))):
        raise ValueError(f"var_eps: a number >= 0, got {var_eps!r}")
    if not (float(a_max) > 0 and math.isfinite(float(a_max))):
        raise ValueError(f"a_max: a number > 0, got {a_max!r}")


def level_window(level: rs.Grid, window_mm=None):
    """The window radius of a level in voxels per array axis: WINDOW_LEVEL_VOXELS for None, otherwise max(1, round(window_mm /
    spacing_i)) (one length or three in array axis order); 0 along an axis of extent 1.  A radius above the device's limit of
    _native.LCC_MAX_RADIUS voxels is a ValueError."""
    sp = spacing_zyx(level)
    if window_mm is None:
        r = [WINDOW_LEVEL_VOXELS] * 3
    else:
        mm = [float(window_mm)] * 3 if np.ndim(window_mm) == 0 else [float(v) for v in window_mm]
        r = [max(1, int(math.floor(mm[i] / sp[i] + 0.5))) for i in range(3)]
    r = [0 if e == 1 else v for e, v in zip(level.shape, r)]
    if max(r) > _native.LCC_MAX_RADIUS:
        raise ValueError(f"window_mm: {window_mm!r} is a window radius of {r} voxels at the level of spacing {tuple(round(v, 4) for v in sp)} mm; "
                         f"the limit is {_native.LCC_MAX_RADIUS} voxels per axis")
    return r


class LccLevel:
    """The buffers and parameters of metric="lcc" on one level: `step(u, v)` is one warp, the window sums and one step (u -> v), the
    counts in `counts_dev`."""

    def __init__(self, eng, fixed_l, moving_l, labels_l, keep, counts_dev, A, b, level: rs.Grid, radius, inv_k2, den_min, var_eps, a_max, scope):
        self.eng, self.fixed_l, self.moving_l, self.labels_l, self.keep, self.counts_dev = eng, fixed_l, moving_l, labels_l, keep, counts_dev
        self.A, self.b, self.shape, self.sp, self.radius = A, b, level.shape, spacing_zyx(level), radius
        self.inv_k2, self.den_min, self.var_eps, self.a_max = inv_k2, den_min, var_eps, a_max
        self.warped = scope.add(eng.empty(level.shape, np.float32))
        self.sums = scope.add(eng.empty((6,) + tuple(level.shape), np.float64))

    def step(self, u, v):
        eng = self.eng
        eng.warp_dev(self.moving_l, u, self.A, self.b, self.shape, "linear", float("nan"), np.float32, self.sp, out=self.warped)
        eng.local_moments_dev(self.fixed_l, self.warped, self.radius, out=self.sums)
        eng.lcc_step_dev(self.fixed_l, self.warped, self.sums, u, v, self.counts_dev, self.A, self.b, self.moving_l.shape, self.sp, self.inv_k2,
                         self.den_min, self.var_eps, self.a_max, self.labels_l, self.keep)

    def counts(self):
        self.eng.sync()
        return [int(c) for c in self.counts_dev.download()[:6]]

    def free(self):
        self.warped.free()
        self.sums.free()


def run_level_lcc(lcc: LccLevel, u, v, iterations: int, taps, patience: int):
    """`run_level` for metric="lcc" -> (iterations run, metrics [(residual16, contributed, rho2q), ...], reason)."""
    rule, metrics, why = StopRule(patience), [], "iterations"
    uc, vc = _components(u), _components(v)
    for _ in range(int(iterations)):
        lcc.step(u, v)
        for src, dst in zip(vc, uc):
            lcc.eng.filter_dev(src, kind="separable", taps=taps, out=dst)
        c = lcc.counts()
        metrics.append([c[4], c[1], c[5]])
        stop = rule.update((c[4], c[1]))
        if stop is not None:
            why = stop
            break
    return len(metrics), metrics, why


def run_level(eng, fixed_l, moving_l, labels_l, keep, u, v, counts_dev, A, b, level: rs.Grid, iterations: int, taps, inv_k2: float,
              den_min: float, patience: int):
    """The iterations of one level on device-resident volumes of that level; the field is `u` before and after (v is the step's
    output and the smoothing's input) -> (iterations run, metrics [(ssd16, contributed), ...], reason)."""
    rule, metrics, why = StopRule(patience), [], "iterations"
    sp = spacing_zyx(level)
    uc, vc = _components(u), _components(v)
    for _ in range(int(iterations)):
        eng.demons_step_dev(fixed_l, moving_l, u, v, counts_dev, A, b, sp, inv_k2, den_min, labels_l, keep)
        for src, dst in zip(vc, uc):
            eng.filter_dev(src, kind="separable", taps=taps, out=dst)
        c = _counts(eng, counts_dev)
        metrics.append([c[4], c[1]])
        stop = rule.update((c[4], c[1]))
        if stop is not None:
            why = stop
            break
    return len(metrics), metrics, why


class DeformableRegistration:
    """What `register_deformable` returns.  `field`: the `DisplacementField` on the fixed grid (its `.affine` is `affine`, the
    transform under it).  `levels`: per level the grid shape, the spacing, the iterations run, the integer metric of every iteration
    -- [16 x the sum of squared differences, contributing voxels] BEFORE that iteration's step -- and why the level stopped.
    `initial_metric`, `final_metric`: the same pair on the last level's volumes with a field of zeros and with the level's final
    field.  With `metric` "lcc" every such entry is a triple -- [16 x the sum of squared residuals of the window's intensity fit,
    contributing voxels, 2^20 x the sum of squared local correlation coefficients] -- and a level also records `window_voxels`.
    `folding`: the folded and NaN voxels of the returned field's Jacobian.  `image`, `affine_registration` (the affine stage's
    `registration.Registration`): set by `LMInferer.apply_deformable`."""

    def __init__(self, field: DisplacementField, levels, initial_metric, final_metric, folding, metric: str = "ssd"):
        self.field = field
        self.metric = metric
        self.affine = field.affine
        self.levels = levels
        self.initial_metric = initial_metric
        self.final_metric = final_metric
        self.folding = folding
        self.fixed_grid = field.grid
        self.moving_grid = None  # (set by register_deformable: where the inverse lives)
        self.image = None
        self.affine_registration = None
        self.field_dev = None
        self.inverse_field = None
        self.inverse_info = None
        self.labels_on_moving = None
        self._inverse_key = None

    def inverse(self, iterations: int = 30, tolerance_mm: float = 0.01, engine=None):
        """`invert(self.field, iterations, tolerance_mm, onto=the moving grid)` -> (DisplacementField on the moving grid, info),
        kept: a second call with the same arguments returns the same objects.  Also `inverse_field` and `inverse_info`."""
        if self.moving_grid is None:
            raise ValueError("DeformableRegistration.inverse: the moving grid is not known (set .moving_grid)")
        key = (int(iterations), float(tolerance_mm))
        if self.inverse_field is None or self._inverse_key != key:
            self.inverse_field, self.inverse_info = invert(self.field, iterations, tolerance_mm, onto=self.moving_grid, engine=engine)
            self._inverse_key = key
        return self.inverse_field, self.inverse_info

    def resample_to_moving(self, data, kind: str = "labels", mode: str = "linear", order: int = 1, fill=None, dtype=None, spacing=None,
                           engine=None, iterations: int = 30, tolerance_mm: float = 0.01):
        """Labels (`kind="labels"`: `warp_labels(data, inverse, mode, ...)`) or an image (`kind="image"`: `warp_image(data, inverse,
        order, ...)`) of the FIXED volume carried onto the moving grid through `self.inverse(iterations, tolerance_mm)`.  `fill`:
        None is 0 for labels and -1024 for an image; `spacing`: a numpy input's, in its axis order."""
        if kind not in ("labels", "image"):
            raise ValueError(f"kind: 'labels' or 'image', got {kind!r}")
        inv, _ = self.inverse(iterations, tolerance_mm, engine=engine)
        if kind == "labels":
            return warp_labels(data, inv, mode, 0 if fill is None else fill, engine=engine, spacing=spacing)
        return warp_image(data, inv, order, -1024 if fill is None else fill, dtype, engine=engine, spacing=spacing)

    def jacobian(self, total: bool = False, engine=None):
        """`jacobian_determinant(self.field, total)`."""
        return jacobian_determinant(self.field, total, engine=engine)

    def resample(self, moving, order: int = 3, fill=-1024, dtype=None, moving_spacing=None, engine=None):
        """`moving` on the fixed grid through the affine and the field: `warp_image(moving, field, order, ...)`."""
        return warp_image(moving, self.field, order, fill, dtype, engine=engine, spacing=moving_spacing)

    def resample_labels(self, labels, mode: str = "linear", fill=0, moving_spacing=None, engine=None):
        """Labels of the moving volume on the fixed grid: `warp_labels(labels, field, mode, ...)`."""
        return warp_labels(labels, self.field, mode, fill, engine=engine, spacing=moving_spacing)

    @staticmethod
    def mean_squared(metric):
        """The mean squared difference of a metric pair, or None when nothing contributed."""
        return metric[0] / (16.0 * metric[1]) if metric and metric[1] else None

    @staticmethod
    def local_correlation(metric):
        """The mean squared local correlation coefficient of an "lcc" metric triple, or None when nothing contributed."""
        return metric[2] / (float(_native.LCC_Q) * metric[1]) if metric and len(metric) > 2 and metric[1] else None

    def meta(self) -> dict:
        """The non-array fields, JSON-serialisable."""
        out = {"kind": "deformable", "metric": self.metric, "levels": self.levels, "initial_metric": self.initial_metric,
               "final_metric": self.final_metric, "initial_mean_squared": self.mean_squared(self.initial_metric),
               "final_mean_squared": self.mean_squared(self.final_metric), "folding": self.folding, "field": self.field.meta(),
               "affine": self.affine_registration.meta() if self.affine_registration is not None else None}
        if self.metric == "lcc":
            out.update({"window_voxels": [lv["window_voxels"] for lv in self.levels],
                        "initial_local_correlation": self.local_correlation(self.initial_metric),
                        "final_local_correlation": self.local_correlation(self.final_metric)})
        if self.inverse_info is not None:  # (only once an inverse has been computed)
            out["inverse"] = self.inverse_info
        return out


def check_schedule(levels_mm, iterations, patience, den_min):
    levels = [float(v) for v in levels_mm]
    its = [int(v) for v in iterations]
    if not levels:
        raise ValueError("levels_mm: at least one level is needed")
    if len(levels) != len(its):
        raise ValueError(f"levels_mm and iterations must have the same length (got {len(levels)} and {len(its)})")
    if any(v < 0 for v in its) or any(float(a) != int(a) for a in iterations):
        raise ValueError(f"iterations: whole numbers >= 0, got {iterations!r}")
    if not (float(den_min) >= 0 and math.isfinite(float(den_min))):
        raise ValueError(f"den_min: a number >= 0, got {den_min!r}")
    StopRule(patience)
    return levels, its


def register_deformable_dev(eng, fixed_dev, moving_dev, fixed_grid: rs.Grid, moving_grid: rs.Grid, scope, affine: Optional[rs.Affine] = None,
                            labels_dev=None, keep=None, levels_mm: Sequence[float] = (8.0, 4.0, 2.0), iterations: Sequence[int] = (60, 40, 20),
                            sigma_mm=None, max_step_mm=None, den_min: float = DEN_MIN, patience: int = PATIENCE, metric: str = "ssd",
                            window_mm=None, var_eps: float = VAR_EPS, a_max: float = A_MAX) -> DeformableRegistration:
    """`register_deformable` on device-resident volumes (and labels of the fixed volume): what `register_deformable` and
    `LMInferer.apply_deformable` share.  `scope`: `add` takes the buffers (a _native.DeviceScope or LMInferer's label scope)."""
    levels_mm, iterations = check_schedule(levels_mm, iterations, patience, den_min)
    check_metric(metric, window_mm, var_eps, a_max)
    if metric == "lcc":
        return _register_lcc_dev(eng, fixed_dev, moving_dev, fixed_grid, moving_grid, scope, affine, labels_dev, keep, levels_mm, iterations,
                                 sigma_mm, max_step_mm, den_min, patience, window_mm, float(var_eps), float(a_max))
    affine = affine if affine is not None else rs.Affine()
    counts_dev = scope.add(eng.empty((5,), np.int64))
    u, prev, records = None, None, []
    initial = final = None
    for k, (mm, its) in enumerate(zip(levels_mm, iterations)):
        fl_grid, ml_grid = level_grid(fixed_grid, mm), level_grid(moving_grid, mm)
        fixed_l = _to_level(eng, fixed_dev, fixed_grid, fl_grid, scope)
        moving_l = _to_level(eng, moving_dev, moving_grid, ml_grid, scope)
        labels_l = None
        if labels_dev is not None:
            A0, b0 = rs.index_map(fixed_grid, fl_grid, None)
            labels_l = scope.add(eng.resample_dev(labels_dev, A0, b0, fl_grid.shape, "nearest", 0, np.uint8))
        if u is None:
            u = scope.add(eng.to_device(np.zeros((3,) + fl_grid.shape, np.float32)))
        else:
            up = _upsample_field(eng, u, prev, fl_grid, scope)
            eng.sync()
            u.free()
            u = up
        v = scope.add(eng.empty((3,) + fl_grid.shape, np.float32))
        A, b = rs.index_map(ml_grid, fl_grid, affine)
        taps, inv_k2 = field_taps(fl_grid, sigma_mm), level_inv_k2(fl_grid, max_step_mm)
        last = k == len(levels_mm) - 1
        if last:  # the metric of the affine alone on this level's volumes: one step from zeros whose field is not used
            zero = eng.to_device(np.zeros((3,) + fl_grid.shape, np.float32))
            try:
                eng.demons_step_dev(fixed_l, moving_l, zero, v, counts_dev, A, b, spacing_zyx(fl_grid), inv_k2, den_min, labels_l, keep)
                c = _counts(eng, counts_dev)
                initial = [c[4], c[1]]
            finally:
                zero.free()
        ran, metrics, why = run_level(eng, fixed_l, moving_l, labels_l, keep, u, v, counts_dev, A, b, fl_grid, its, taps, inv_k2, den_min, patience)
        if last:
            eng.demons_step_dev(fixed_l, moving_l, u, v, counts_dev, A, b, spacing_zyx(fl_grid), inv_k2, den_min, labels_l, keep)
            c = _counts(eng, counts_dev)
            final = [c[4], c[1]]
        records.append({"level_mm": mm, "shape": list(fl_grid.shape), "spacing_mm": list(spacing_zyx(fl_grid)), "iterations": ran, "metric": metrics,
                        "stopped": why})
        eng.sync()
        for d in (fixed_l, moving_l, labels_l, v):
            if d is not None:
                d.free()
        prev = fl_grid
    full = _upsample_field(eng, u, prev, fixed_grid, scope) if prev.shape != fixed_grid.shape or not prev.same_as(fixed_grid) else u
    fold = scope.add(eng.empty((2,), np.int64))
    det = eng.jacobian_dev(full, spacing_zyx(fixed_grid), counts=fold)
    eng.sync()
    det.free()
    f = fold.download()
    field = DisplacementField(full.download(), fixed_grid, affine)
    reg = DeformableRegistration(field, records, initial, final, {"folded": int(f[0]), "nonfinite": int(f[1])})
    reg.moving_grid = moving_grid
    reg.field_dev = full  # (the device copy, alive as long as `scope`: apply_deformable warps through it)
    return reg


def _register_lcc_dev(eng, fixed_dev, moving_dev, fixed_grid, moving_grid, scope, affine, labels_dev, keep, levels_mm, iterations, sigma_mm,
                      max_step_mm, den_min, patience, window_mm, var_eps, a_max) -> DeformableRegistration:
    """`register_deformable_dev` with metric="lcc": the same pyramid, the iterations of `run_level_lcc`."""
    affine = affine if affine is not None else rs.Affine()
    grids = [(level_grid(fixed_grid, mm), level_grid(moving_grid, mm)) for mm in levels_mm]
    windows = [level_window(fl, window_mm) for fl, _ in grids]  # (a window that is too wide is refused before anything runs)
    counts_dev = scope.add(eng.empty((6,), np.int64))
    u, prev, records = None, None, []
    initial = final = None
    for k, (mm, its) in enumerate(zip(levels_mm, iterations)):
        fl_grid, ml_grid = grids[k]
        fixed_l = _to_level(eng, fixed_dev, fixed_grid, fl_grid, scope)
        moving_l = _to_level(eng, moving_dev, moving_grid, ml_grid, scope)
        labels_l = None
        if labels_dev is not None:
            A0, b0 = rs.index_map(fixed_grid, fl_grid, None)
            labels_l = scope.add(eng.resample_dev(labels_dev, A0, b0, fl_grid.shape, "nearest", 0, np.uint8))
        if u is None:
            u = scope.add(eng.to_device(np.zeros((3,) + fl_grid.shape, np.float32)))
        else:
            up = _upsample_field(eng, u, prev, fl_grid, scope)
            eng.sync()
            u.free()
            u = up
        v = scope.add(eng.empty((3,) + fl_grid.shape, np.float32))
        A, b = rs.index_map(ml_grid, fl_grid, affine)
        taps, inv_k2 = field_taps(fl_grid, sigma_mm), level_inv_k2(fl_grid, max_step_mm)
        lcc = LccLevel(eng, fixed_l, moving_l, labels_l, keep, counts_dev, A, b, fl_grid, windows[k], inv_k2, den_min, var_eps, a_max, scope)
        last = k == len(levels_mm) - 1
        if last:  # the metric of the affine alone on this level's volumes: one step from zeros whose field is not used
            zero = eng.to_device(np.zeros((3,) + fl_grid.shape, np.float32))
            try:
                lcc.step(zero, v)
                c = lcc.counts()
                initial = [c[4], c[1], c[5]]
            finally:
                zero.free()
        ran, metrics, why = run_level_lcc(lcc, u, v, its, taps, patience)
        if last:
            lcc.step(u, v)
            c = lcc.counts()
            final = [c[4], c[1], c[5]]
        records.append({"level_mm": mm, "shape": list(fl_grid.shape), "spacing_mm": list(spacing_zyx(fl_grid)), "window_voxels": list(windows[k]),
                        "iterations": ran, "metric": metrics, "stopped": why})
        eng.sync()
        lcc.free()
        for d in (fixed_l, moving_l, labels_l, v):
            if d is not None:
                d.free()
        prev = fl_grid
    full = _upsample_field(eng, u, prev, fixed_grid, scope) if prev.shape != fixed_grid.shape or not prev.same_as(fixed_grid) else u
    fold = scope.add(eng.empty((2,), np.int64))
    det = eng.jacobian_dev(full, spacing_zyx(fixed_grid), counts=fold)
    eng.sync()
    det.free()
    f = fold.download()
    field = DisplacementField(full.download(), fixed_grid, affine)
    reg = DeformableRegistration(field, records, initial, final, {"folded": int(f[0]), "nonfinite": int(f[1])}, metric="lcc")
    reg.moving_grid = moving_grid
    reg.field_dev = full
    return reg


def _initial_affine(initial) -> Optional[rs.Affine]:
    from . import registration as lmreg

    if initial is None or isinstance(initial, rs.Affine):
        return initial
    if isinstance(initial, lmreg.Registration):
        return initial.transform
    raise TypeError(f"initial: None, an Affine or a Registration, got {type(initial).__name__}")


def register_deformable(fixed, moving, initial=None, labels=None, keep=None, levels_mm: Sequence[float] = (8.0, 4.0, 2.0),
                        iterations: Sequence[int] = (60, 40, 20), sigma_mm=None, max_step_mm=None, den_min: float = DEN_MIN,
                        patience: int = PATIENCE, spacing=None, moving_spacing=None, engine=None, metric: str = "ssd", window_mm=None,
                        var_eps: float = VAR_EPS, a_max: float = A_MAX) -> DeformableRegistration:
    """Registers `moving` onto `fixed` (numpy [n, h, w], `volume_io.Volume`s or SimpleITK images) by additive demons on the GPU -> a
    `DeformableRegistration`; the module docstring has the method.  `initial`: None, an `Affine` or a `registration.Registration`
    (its transform) from the fixed to the moving space -- the field is found on top of it.  `labels`, `keep`: labels of the FIXED
    volume; only voxels whose label is in `keep` (None: every label >= 1) take a step, the others are moved by the smoothing alone.
    `levels_mm`, `iterations`: the pyramid's spacings and the iteration count of each level; the last level's spacing is
    `levels_mm[-1]`, not the native one, and its field is upsampled once to the fixed grid.  `sigma_mm`: the field's Gaussian in
    millimetres (None: one voxel of each level).  `max_step_mm`: the longest step of an iteration (None: half a voxel of each
    level).  `den_min`: denominators below it give no step.  `patience`: see the module docstring.  `spacing`, `moving_spacing`:
    numpy inputs only, in the array's axis order (None: unit voxels, and every "mm" above is a voxel).  `metric`: "ssd", or "lcc" for
    a pair whose intensities differ locally (inspiration / expiration; the module docstring), with `window_mm` (the window reaches
    this far to either side: None is 4 voxels of each level, otherwise max(1, round(window_mm / spacing)) voxels per axis, at most 8:
    a wider one is a ValueError), `var_eps` (HU^2 added per voxel to the window's variance of the moving image: a nearly flat window
    gets a small gain) and `a_max` (the largest gain).  With "ssd" the three are checked and not used."""
    from . import registration as lmreg

    check_schedule(levels_mm, iterations, patience, den_min)
    check_metric(metric, window_mm, var_eps, a_max)
    affine = _initial_affine(initial)
    fixed_grid, moving_grid = lmreg._grid_of(fixed, spacing), lmreg._grid_of(moving, moving_spacing)
    fv, mv = rs._image_array(fixed), rs._image_array(moving)
    lab = None
    if labels is not None:
        lab = rs._label_u8(labels)
        if lab.shape != fv.shape:
            raise ValueError(f"labels {lab.shape} must have the fixed volume's shape {fv.shape}")
    with _native.engine_scope(engine) as eng:
        with eng.scope() as dev:
            reg = register_deformable_dev(eng, dev.upload(fv), dev.upload(mv), fixed_grid, moving_grid, dev, affine,
                                          dev.upload(lab) if lab is not None else None, keep, levels_mm, iterations, sigma_mm, max_step_mm,
                                          den_min, patience, metric, window_mm, var_eps, a_max)
            reg.field_dev = None  # (freed with the scope)
            return reg
