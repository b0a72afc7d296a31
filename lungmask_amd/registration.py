"""Rigid and affine registration of two volumes by mutual information on the GPU (not in the reference: what callers leave the
device for SimpleITK or elastix for) -- the transform that `resample.resample_image(moving, fixed, transform=...)` needs to place a
follow-up onto its baseline.

The cost is read off the joint intensity histogram of the fixed and the moving volume under an affine map of indices
(`lm_joint_hist_dev`, lungmask_amd/csrc/register_kernels.hip; the definition is in include/lungmask_hip.h).  Both volumes and the
optional labels cross to the device once; an evaluation is one device call and one read-back of bins^2 + 4 integers, and no
resampled volume is ever written.  The histogram is made of integers -- a sample adds 65536, split between the two nearest moving
bins -- so it does not depend on the schedule, and the optimiser around it is deterministic float64 numpy: a registration gives the
same transform wherever it runs.

- metric: "nmi", (H(F) + H(M)) / H(F, M) (Studholme), or "mi", H(F) + H(M) - H(F, M); natural logarithms.
- transform: "translation", "rigid", "similarity" or "affine" (`resample.Affine.from_parameters`: degrees about the L, P, S axes
  through the centre, millimetres, per cent of scale and shear).  The centre is the physical centre of the fixed grid, or the
  centroid of the sampled labels.
- levels: each entry of `levels_mm` is a sampling distance -- every step_i = max(1, round(level / spacing_i))-th fixed voxel is
  sampled -- coarse to fine, each level starting at the optimum of the one before.  No smoothing is applied: call
  `filters.gaussian` first where the coarse levels should see less noise.
- optimiser: Powell's direction set with a bracketing and Brent line search.  The last level stops on a parameter tolerance of 0.01
  units (coarser levels on the same tolerance times their step ratio, at most 4 times), or at `max_evaluations`.  An evaluation in
  which fewer than `min_overlap` of the sampled voxels fall inside the moving volume is worse than any valid one.

The result maps the fixed (output) space to the moving (source) space, `resample`'s convention.  Quality on real CT pairs is not
validated by anything here.
"""
from __future__ import annotations

import math
from typing import Callable, Optional, Sequence

import numpy as np

from . import _native
from . import resample as rs

TRANSFORMS = rs.Affine.PARAMETERS
METRICS = ("nmi", "mi")
TOLERANCE = 0.01  # parameter units: degrees, millimetres, per cent
# The optimiser's inner thresholds as shares of its tolerance: a line is minimised to _LINE of it, and a sweep of all directions has
# to move every parameter by less than _SWEEP of it before the search stops.  With the tolerance itself in both places the search
# stopped up to 0.08 units short of the minimum of a quadratic of condition 100 in 12 variables (a sweep creeps along the flat
# directions); with these it ends within 0.006 (tests/test_register_host.py).
_LINE, _SWEEP = 0.05, 0.25
# the first level's search steps per parameter: degrees, millimetres, per cent of scale, per cent of shear
_FIRST_STEPS = {"rotation": 2.0, "translation": 4.0, "scale": 2.0, "shear": 2.0}


# ------------------------------------------------------------------------------------------------ the metric
def mutual_information(hist, normalized: bool = True) -> Optional[float]:
    """The (normalised) mutual information of a joint histogram, in float64: P = hist / hist.sum(), entropies with the natural
    logarithm over the non-zero bins.  `normalized`: (H(F) + H(M)) / H(F, M), between 1 (independent) and 2 (one determines the
    other); otherwise H(F) + H(M) - H(F, M).  None for an empty histogram or a joint entropy of 0."""
    h = np.asarray(hist, np.float64)
    total = float(h.sum())
    if not total > 0.0:
        return None
    p = h / total

    def entropy(q):
        q = q[q > 0.0]
        return -float(np.sum(q * np.log(q)))

    hf, hm, hj = entropy(p.sum(axis=1)), entropy(p.sum(axis=0)), entropy(p.reshape(-1))
    if not hj > 0.0:
        return None
    return (hf + hm) / hj if normalized else hf + hm - hj


def evaluation_cost(hist, counts: dict, metric: str = "nmi", min_overlap: float = 0.5) -> float:
    """What the optimiser minimises: minus the metric, or -- when fewer than `min_overlap` of the sampled voxels contributed, or the
    metric does not exist -- 1 + the share that did not contribute: above every valid value (a valid one is <= 0), and falling
    towards more overlap, so that the volumes cannot slide apart."""
    sampled, inside = counts["sampled"], counts["contributed"]
    value = mutual_information(hist, metric == "nmi") if sampled and inside >= min_overlap * sampled else None
    if value is None:
        return 1.0 + (1.0 - inside / sampled if sampled else 1.0)
    return -value


# ------------------------------------------------------------------------------------------------ the optimiser
class _OutOfEvaluations(Exception):
    pass


class _Counted:
    """`cost` with a budget and the best point seen."""

    def __init__(self, cost: Callable, budget: int):
        self.cost, self.budget, self.evaluations = cost, int(budget), 0
        self.best_x, self.best_f = None, math.inf

    def __call__(self, x):
        if self.evaluations >= self.budget:
            raise _OutOfEvaluations()
        self.evaluations += 1
        f = float(self.cost(x))
        if f < self.best_f:
            self.best_x, self.best_f = np.array(x, np.float64), f
        return f


_GOLD = 1.618033988749895
_CGOLD = 0.3819660112501051


def _bracket(g, fa: float):
    """A bracket a < b < c (or a > b > c) of a minimum of g with g(b) <= g(a), g(c), from a = 0 and a first step of 1, by golden
    expansion (at most 30 steps) -> (a, b, c, g(b))."""
    a, b = 0.0, 1.0
    fb = g(b)
    if fb > fa:
        a, b, fa, fb = b, a, fb, fa
    c = b + _GOLD * (b - a)
    fc = g(c)
    for _ in range(30):
        if fc >= fb:
            break
        a, b, fa, fb = b, c, fb, fc
        c = b + _GOLD * (b - a)
        fc = g(c)
    return a, b, c, fb


def _brent(g, a: float, b: float, c: float, fb: float, tol: float):
    """Brent's minimisation inside the bracket (a, b, c) to the absolute tolerance `tol` -> (t, g(t))."""
    lo, hi = min(a, c), max(a, c)
    x = w = v = b
    fx = fw = fv = fb
    d = e = 0.0
    for _ in range(40):
        xm = 0.5 * (lo + hi)
        if abs(x - xm) <= 2.0 * tol - 0.5 * (hi - lo):
            break
        parabolic = False
        if abs(e) > tol:
            r = (x - w) * (fx - fv)
            q = (x - v) * (fx - fw)
            p = (x - v) * q - (x - w) * r
            q = 2.0 * (q - r)
            if q > 0.0:
                p = -p
            q = abs(q)
            if abs(p) < abs(0.5 * q * e) and p > q * (lo - x) and p < q * (hi - x):
                e, d = d, p / q
                u = x + d
                if u - lo < 2.0 * tol or hi - u < 2.0 * tol:
                    d = tol if xm >= x else -tol
                parabolic = True
        if not parabolic:
            e = (lo if x >= xm else hi) - x
            d = _CGOLD * e
        u = x + d if abs(d) >= tol else x + (tol if d > 0.0 else -tol)
        fu = g(u)
        if fu <= fx:
            if u >= x:
                lo = x
            else:
                hi = x
            v, w, x = w, x, u
            fv, fw, fx = fw, fx, fu
        else:
            if u < x:
                lo = u
            else:
                hi = u
            if fu <= fw or w == x:
                v, w, fv, fw = w, u, fw, fu
            elif fu <= fv or v == x or v == w:
                v, fv = u, fu
    return x, fx


def minimize(cost: Callable, x0, steps, tolerance: float = TOLERANCE, max_evaluations: int = 4000, max_iterations: int = 30):
    """Powell's direction-set minimisation of `cost` from `x0`, deterministic and derivative-free -> (x, cost(x), evaluations).
    `steps`: the first search step per parameter; the directions start as the axes scaled by them.  Every line is bracketed from
    its direction's length and minimised with Brent's method to `tolerance` / 20 in the parameter that moves most.  Stops when no
    parameter moved by `tolerance` / 4 during a whole sweep of the directions -- so that the minimum is reached within `tolerance`
    on anisotropic cost functions too --, or with the best point seen after `max_evaluations`."""
    x = np.array(x0, np.float64).reshape(-1)
    n = x.size
    steps = np.asarray(steps, np.float64).reshape(-1)
    if steps.size != n or not np.all(steps > 0):
        raise ValueError("minimize: one positive step per parameter is needed")
    f = _Counted(cost, max_evaluations)
    dirs = [np.eye(n)[i] * steps[i] for i in range(n)]

    def line(x, fx, d):
        tol = _LINE * tolerance / float(np.max(np.abs(d)))
        a, b, c, fb = _bracket(lambda t: f(x + t * d), fx)
        t, ft = _brent(lambda t: f(x + t * d), a, b, c, fb, tol)
        return (x + t * d, ft, t * d) if ft < fx else (x, fx, 0.0 * d)

    try:
        fx = f(x)
        for _ in range(max_iterations):
            x_start, f_start = x.copy(), fx
            biggest, which = 0.0, 0
            for i in range(n):
                f_before = fx
                x, fx, move = line(x, fx, dirs[i])
                if np.any(move != 0.0):  # the next bracket along this direction starts from what it took this time
                    dirs[i] = move if np.max(np.abs(move)) >= 4.0 * tolerance else move * (4.0 * tolerance / np.max(np.abs(move)))
                if f_before - fx > biggest:
                    biggest, which = f_before - fx, i
            total = x - x_start
            if np.max(np.abs(total)) < _SWEEP * tolerance:
                break
            f_ext = f(x + total)  # Powell's test: is the sweep's overall move worth a direction of its own?
            if f_ext < f_start and 2.0 * (f_start - 2.0 * fx + f_ext) * (f_start - fx - biggest) ** 2 < biggest * (f_start - f_ext) ** 2:
                x, fx, _ = line(x, fx, total)
                dirs[which] = dirs[-1]
                dirs[-1] = total
    except _OutOfEvaluations:
        pass
    if f.best_x is not None and f.best_f <= fx:
        x, fx = f.best_x, f.best_f
    return x, fx, f.evaluations


def first_steps(kind: str) -> np.ndarray:
    """The first level's search step of every parameter of `kind`."""
    s = _FIRST_STEPS
    full = [s["rotation"]] * 3 + [s["translation"]] * 3 + [s["scale"]] * 3 + [s["shear"]] * 3
    return np.array({"translation": full[3:6], "rigid": full[:6], "similarity": full[:7], "affine": full}[kind])


# ------------------------------------------------------------------------------------------------ inputs
def _bins_of(hu_range, bins: int):
    lo, hi = int(hu_range[0]), int(hu_range[1])
    if int(bins) != bins or not 2 <= int(bins) <= 64:
        raise ValueError(f"bins: 2 .. 64, got {bins!r}")
    if hi < lo:
        raise ValueError(f"hu_range: (lowest, highest) HU, got {hu_range!r}")
    return lo, -(-(hi - lo + 1) // int(bins))


def _level_step(level_mm: float, spacing_zyx) -> tuple:
    if not level_mm > 0:
        raise ValueError(f"levels_mm: sampling distances > 0, got {level_mm!r}")
    return tuple(max(1, int(math.floor(level_mm / s + 0.5))) for s in spacing_zyx)


def _volume_array(image) -> np.ndarray:
    """The array of an image input in a dtype of the engine; uint8 (a label volume, for mode "nearest") stays uint8."""
    from . import stats as st

    arr = np.asarray(st._label_array(image))
    if arr.dtype == np.uint8 and arr.ndim == 3 and arr.shape[0] >= 1:
        return np.ascontiguousarray(arr)
    return rs._image_array(image)


def _grid_of(image, spacing) -> rs.Grid:
    return rs.Grid.of(image if not isinstance(image, np.ndarray) else np.asarray(image), spacing)


def label_centroid_index(labels: np.ndarray, keep=None):
    """The centroid (array axis order) of the voxels of `labels` whose value is in `keep` (None: every label >= 1), from integer
    sums -> three floats, or None without such a voxel."""
    sel = labels > 0 if keep is None else np.isin(labels, list(keep))
    voxels = int(np.count_nonzero(sel))
    if not voxels:
        return None
    sums = [int(np.dot(sel.sum(axis=tuple(a for a in range(3) if a != i), dtype=np.int64), np.arange(labels.shape[i], dtype=np.int64)))
            for i in range(3)]
    return [s / voxels for s in sums]


# ------------------------------------------------------------------------------------------------ results
class Registration:
    """What `register` returns.  `transform`: the `resample.Affine` from the fixed (output) space to the moving (source) space --
    `resample.resample_image(moving, fixed, transform=reg.transform)` applies it.  `parameters`: the parameter vector of `kind`
    about `centre` (applied before `initial`).  `metric`, `value` (the metric at the optimum, None when no evaluation was valid),
    `evaluations`, `levels` (per level: step, evaluations, metric value, parameters) and `counts` (those of the last evaluation:
    sampled, contributed, outside, nan).  `image`: set by `LMInferer.apply_registered` only."""

    def __init__(self, transform, parameters, kind, centre, metric, value, evaluations, levels, counts, fixed_grid):
        self.transform = transform
        self.parameters = [float(v) for v in parameters]
        self.kind = kind
        self.centre = [float(v) for v in centre]
        self.metric = metric
        self.value = value
        self.evaluations = int(evaluations)
        self.levels = levels
        self.counts = counts
        self.fixed_grid = fixed_grid
        self.image = None

    def meta(self) -> dict:
        """The non-array fields, JSON-serialisable."""
        return {"kind": self.kind, "metric": self.metric, "value": self.value, "parameters": self.parameters, "centre": self.centre,
                "matrix": [float(v) for v in self.transform.matrix.reshape(-1)],
                "translation": [float(v) for v in self.transform.translation_vector], "evaluations": self.evaluations,
                "levels": self.levels, "counts": self.counts, "fixed_grid": self.fixed_grid.meta()}

    def resample(self, moving, order: int = 3, fill=-1024, dtype=None, moving_spacing=None, engine=None):
        """`moving` on the fixed grid: `resample.resample_image(moving, fixed grid, transform, order, ...)` -- a Volume, or the
        bare array for a numpy `moving` without `moving_spacing`."""
        return rs.resample_image(moving, self.fixed_grid, self.transform, order, fill, dtype, spacing=moving_spacing, engine=engine)

    def resample_labels(self, labels, mode: str = "linear", fill=0, moving_spacing=None, engine=None):
        """Labels of the moving volume on the fixed grid: `resample.resample_labels(labels, fixed grid, transform, mode, ...)`."""
        return rs.resample_labels(labels, self.fixed_grid, self.transform, mode, fill, spacing=moving_spacing, engine=engine)


# ------------------------------------------------------------------------------------------------ device forms
class _Evaluator:
    """The joint histogram of two device-resident volumes as a function of the transform: one device call and one read-back of
    bins^2 + 4 integers per evaluation."""

    def __init__(self, eng, fixed_dev, moving_dev, fixed_grid, moving_grid, bins, fixed_bins, moving_bins, mode, labels_dev, keep, scope):
        self.eng, self.fixed, self.moving, self.labels, self.keep = eng, fixed_dev, moving_dev, labels_dev, keep
        self.fixed_grid, self.moving_grid = fixed_grid, moving_grid
        self.bins, self.fixed_bins, self.moving_bins, self.mode = int(bins), fixed_bins, moving_bins, mode
        self.out = scope.add(eng.empty((self.bins ** 2 + 4,), np.int64))

    def __call__(self, transform, step=(1, 1, 1), start=(0, 0, 0)):
        A, b = rs.index_map(self.moving_grid, self.fixed_grid, transform)
        self.eng.joint_hist_dev(self.fixed, self.moving, A, b, self.bins, self.fixed_bins, self.moving_bins, start, step, self.mode,
                                self.labels, self.keep, out=self.out)
        self.eng.sync()
        return self.eng.split_joint_hist(self.out.download(), self.bins)


def register_dev(eng, fixed_dev, moving_dev, fixed_grid: rs.Grid, moving_grid: rs.Grid, scope, transform: str = "rigid", labels_dev=None,
                 keep=None, centre=None, initial: Optional[rs.Affine] = None, metric: str = "nmi", bins: int = 32, hu_range=(-1024, 1023),
                 moving_hu_range=None, levels_mm: Sequence[float] = (8.0, 4.0, 2.0), min_overlap: float = 0.5, max_evaluations: int = 4000,
                 mode: str = "linear") -> Registration:
    """`register` on device-resident volumes (and labels): what `register` and `LMInferer.apply_registered` share.  `centre`: the
    rotation centre in LPS millimetres (None: the physical centre of the fixed grid).  `scope`: `add` takes the result buffer."""
    if transform not in TRANSFORMS:
        raise ValueError(f"transform: one of {sorted(TRANSFORMS)}, got {transform!r}")
    if metric not in METRICS:
        raise ValueError(f"metric: 'nmi' or 'mi', got {metric!r}")
    if mode not in _native.JOINT_HIST_MODES:
        raise ValueError(f"mode: 'linear' or 'nearest', got {mode!r}")
    if not 0.0 <= float(min_overlap) <= 1.0:
        raise ValueError(f"min_overlap: a share in 0 .. 1, got {min_overlap!r}")
    if int(max_evaluations) < 1:
        raise ValueError(f"max_evaluations: at least 1, got {max_evaluations!r}")
    levels_mm = [float(v) for v in levels_mm]
    if not levels_mm:
        raise ValueError("levels_mm: at least one sampling distance is needed")
    fixed_bins = _bins_of(hu_range, bins)
    moving_bins = _bins_of(hu_range if moving_hu_range is None else moving_hu_range, bins)
    spacing_zyx = fixed_grid.spacing[::-1]
    level_steps = [_level_step(v, spacing_zyx) for v in levels_mm]
    if centre is None:
        centre = fixed_grid.index_to_physical([(e - 1) / 2.0 for e in fixed_grid.shape])
    centre = np.asarray(centre, np.float64).reshape(3)
    first = initial if initial is not None else rs.Affine()
    evaluate = _Evaluator(eng, fixed_dev, moving_dev, fixed_grid, moving_grid, bins, fixed_bins, moving_bins, mode, labels_dev, keep, scope)

    def transform_of(x):
        return first.compose(rs.Affine.from_parameters(transform, x, centre))

    x = np.zeros(TRANSFORMS[transform])
    levels, used, last = [], 0, {}
    for k, step in enumerate(level_steps):
        def cost(p, step=step):
            hist, counts = evaluate(transform_of(p), step)
            last["hist"], last["counts"] = hist, counts
            return evaluation_cost(hist, counts, metric, min_overlap)

        if max_evaluations - used < 1:
            break
        coarse = min(4.0, float(max(a / b for a, b in zip(step, level_steps[-1]))))
        x, fx, n_eval = minimize(cost, x, np.maximum(first_steps(transform) / 2.0 ** k, 4.0 * TOLERANCE), TOLERANCE * max(1.0, coarse),
                                 max_evaluations - used)
        used += n_eval
        levels.append({"level_mm": levels_mm[k], "step": [int(v) for v in step], "evaluations": int(n_eval), "metric": -fx if fx <= 0.0 else None,
                       "parameters": [float(v) for v in x]})
    final = transform_of(x)
    hist, counts = evaluate(final, level_steps[len(levels) - 1] if levels else level_steps[-1])  # the counts of the result
    used += 1
    value = evaluation_cost(hist, counts, metric, min_overlap)
    return Registration(final, x, transform, centre, metric, -value if value <= 0.0 else None, used, levels, counts, fixed_grid)


# ------------------------------------------------------------------------------------------------ host forms
def joint_histogram(fixed, moving, transform: Optional[rs.Affine] = None, bins: int = 32, hu_range=(-1024, 1023), moving_hu_range=None,
                    step=1, labels=None, keep=None, mode: str = "linear", spacing=None, moving_spacing=None, engine=None):
    """The joint histogram of `fixed` and `moving` (numpy [n, h, w], `volume_io.Volume`s or SimpleITK images) under `transform` (an
    `Affine` from the fixed space to the moving space; None: the identity) on the GPU -> (hist int64 [bins][bins], counts).
    hist[i][k]: 65536 per sample whose fixed value falls into bin i and whose moving value into bin k, split between the two
    nearest moving bins with `mode` "linear" (the trilinear value) and whole with "nearest" (the raw nearest voxel: the mode for
    two label volumes).  Bins: `bins` of width ceil((hi - lo + 1) / bins) from lo, values outside clamped; `moving_hu_range`
    defaults to `hu_range`.  `step`: every step-th fixed voxel (one value or three, array axis order).  `labels`, `keep`: only the
    fixed voxels whose label is in `keep` (None: every label >= 1) are sampled.  counts: sampled, contributed, outside (the moving
    volume), nan.  `spacing`, `moving_spacing`: numpy inputs only, in the array's axis order."""
    fixed_grid, moving_grid = _grid_of(fixed, spacing), _grid_of(moving, moving_spacing)
    fv, mv = _volume_array(fixed), _volume_array(moving)
    fixed_bins = _bins_of(hu_range, bins)
    moving_bins = _bins_of(hu_range if moving_hu_range is None else moving_hu_range, bins)
    st = [int(step)] * 3 if np.ndim(step) == 0 else [int(v) for v in step]
    if len(st) != 3 or min(st) < 1:
        raise ValueError(f"step: one value or three >= 1, got {step!r}")
    lab = None
    if labels is not None:
        lab = rs._label_u8(labels)
        if lab.shape != fv.shape:
            raise ValueError(f"labels {lab.shape} must have the fixed volume's shape {fv.shape}")
    with _native.engine_scope(engine) as eng:
        with eng.scope() as dev:
            ev = _Evaluator(eng, dev.upload(fv), dev.upload(mv), fixed_grid, moving_grid, bins, fixed_bins, moving_bins, mode,
                            dev.upload(lab) if lab is not None else None, keep, dev)
            return ev(transform, st)


def register(fixed, moving, transform: str = "rigid", labels=None, keep=None, initial=None, metric: str = "nmi", bins: int = 32,
             hu_range=(-1024, 1023), levels_mm: Sequence[float] = (8.0, 4.0, 2.0), min_overlap: float = 0.5, max_evaluations: int = 4000,
             spacing=None, moving_spacing=None, engine=None, moving_labels=None, moving_hu_range=None, mode: str = "linear") -> Registration:
    """Registers `moving` onto `fixed` (numpy [n, h, w], `volume_io.Volume`s or SimpleITK images) by mutual information on the GPU
    -> a `Registration`; the module docstring has the method.  `transform`: "translation", "rigid", "similarity" or "affine".
    `labels`, `keep`: labels of the FIXED volume; only voxels whose label is in `keep` (None: every label >= 1) are sampled, and
    their centroid is the rotation centre.  `initial`: an `Affine` to start from, or "centroids" (`resample.align_centroids` of
    `labels` and `moving_labels`).  `mode` "nearest" with two uint8 label volumes (hu_range=(0, bins - 1)) is the label-driven form.
    `spacing`, `moving_spacing`: numpy inputs only, in the array's axis order (None: unit voxels)."""
    fixed_grid, moving_grid = _grid_of(fixed, spacing), _grid_of(moving, moving_spacing)
    fv, mv = _volume_array(fixed), _volume_array(moving)
    lab, centre = None, None
    if labels is not None:
        lab = rs._label_u8(labels)
        if lab.shape != fv.shape:
            raise ValueError(f"labels {lab.shape} must have the fixed volume's shape {fv.shape}")
        idx = label_centroid_index(lab, keep)
        if idx is None:
            raise ValueError("register: the labels hold no voxel of the kept label values")
        centre = fixed_grid.index_to_physical(idx)
    if isinstance(initial, str):
        if initial != "centroids":
            raise ValueError(f"initial: an Affine or 'centroids', got {initial!r}")
        if labels is None or moving_labels is None:
            raise ValueError("initial='centroids' needs labels= and moving_labels=")
        initial = rs.align_centroids(labels, moving_labels, spacing, moving_spacing, engine=engine)
    elif initial is not None and not isinstance(initial, rs.Affine):
        raise TypeError(f"initial: an Affine or 'centroids', got {type(initial).__name__}")
    with _native.engine_scope(engine) as eng:
        with eng.scope() as dev:
            return register_dev(eng, dev.upload(fv), dev.upload(mv), fixed_grid, moving_grid, dev, transform,
                                dev.upload(lab) if lab is not None else None, keep, centre, initial, metric, bins, hu_range, moving_hu_range,
                                levels_mm, min_overlap, max_evaluations, mode)
