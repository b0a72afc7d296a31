"""lm_local_moments_dev and lm_lcc_step_dev on the emulation library, bit for bit against numpy restatements of the definitions in
include/lungmask_hip.h (`moments_oracle`, `lcc_step_oracle`; test_gpu_lcc.py runs the same cases on the device), their properties, a
five-iteration loop against the same loop written with the restatements, and the quality of `register_deformable(metric="lcc")` on
two synthetic inspiration / expiration pairs beside `metric="ssd"`.

Shapes: (5, 7, 9) with three different radii; (1, 6, 8), where an axis of extent 1 has no window and no gradient; (3, 4, 70) with
radius 8 on every axis, where the window is wider than two of the axes; a radius of 0 on one axis, whose pass is skipped.

Quality pairs (28 x 44 x 44, the blobs-and-sinusoid construction of test_deform_emu.py, field peak 2 voxels, levels of 2 and 1
voxels, 40 + 20 iterations): fixed = air + (content(o + u) - air) / (s * J), J the Jacobian determinant of the true field, N(0, 20)
noise on both images.  End-point errors in voxels over the voxels at least 3 from the border, measured on the emulator (the device
gives the same bits, test_gpu_lcc.py):

    s = 1.6 (a global deflation as well):  zero field 1.226,  ssd 3.905 (15 folded voxels),  lcc 1.124 (no folded voxel, Jacobian
        0.467 .. 1.938), lcc / ssd 0.288 (bar: 0.5), mean squared local correlation 0.6031 -> 0.7348, 25 + 20 iterations
    s = 1.0 (the Jacobian's density change only):  zero field 1.226,  ssd 1.365,  lcc 1.149 (Jacobian 0.396 .. 2.012), lcc / ssd
        0.842 (measured, not barred), mean squared local correlation 0.6744 -> 0.8257, 29 + 20 iterations

The bars hold, but the margin over the zero field is 8 % and 6 %: the true field of this pair has a Jacobian of 0.47 .. 1.94, so
the density of the fixed image changes by a factor of four across the volume, and at the true field the metric (mean squared
residual 493.5 at s = 1.6) is no better than at the field found (428.7) -- the residual there is at the level of the noise.  On the
plain pair of test_deform_emu.py (no density change) the same run reaches 0.617 where ssd reaches 0.529 of 1.226.
"""
import warnings

import numpy as np
import pytest

from lungmask_amd import _native as nat
from lungmask_amd import deformable as dfm
from lungmask_amd import resample as rs
from tests.test_deform_emu import RECOVERY_KW, RECOVERY_SHAPE, content, coordinate, domain, make_field, same_bits, scales, warp_oracle
from tests.test_filters_emu import oracle_separable


# ------------------------------------------------------------------------------------------------ the restatements
def _window_sum(a, r, axis):
    """acc = 0.0; for k = -r .. r ascending, in range: acc = acc + in[i + k] along `axis` (a zero stands for a term that is out of
    range: it changes no bit of a sum that starts at +0.0)."""
    e = a.shape[axis]
    acc = np.zeros(a.shape, np.float64)
    for k in range(-r, r + 1):
        term = np.zeros(a.shape, np.float64)
        lo, hi = max(0, -k), min(e, e - k)  # the outputs i with 0 <= i + k < e
        if lo < hi:
            dst, src = [slice(None)] * 3, [slice(None)] * 3
            dst[axis], src[axis] = slice(lo, hi), slice(lo + k, hi + k)
            term[tuple(dst)] = a[tuple(src)]
        acc = acc + term
    return acc


def moments_oracle(f, m, radius):
    """lm_local_moments_dev's definition -> float64 [6][n][h][w]."""
    r = [int(radius)] * 3 if np.ndim(radius) == 0 else [int(v) for v in radius]
    valid = np.isfinite(f) & np.isfinite(m)
    fd, md = np.where(valid, f.astype(np.float64), 0.0), np.where(valid, m.astype(np.float64), 0.0)
    out = []
    for term in (valid.astype(np.float64), fd, md, fd * fd, md * md, fd * md):
        s = _window_sum(term, r[2], 2)
        for axis in (1, 0):
            if r[axis] > 0:
                s = _window_sum(s, r[axis], axis)
        out.append(s)
    return np.stack(out)


def lcc_step_oracle(f, m, S, u, A, b, moving_shape, spacing=None, inv_k2=1.0, den_min=1e-9, var_eps=25.0, a_max=4.0, labels=None, keep=None):
    """lm_lcc_step_dev's definition -> (out float32 [3][n][h][w], counts: six Python integers)."""
    fs, gs = scales(spacing)
    shape = f.shape
    sel = np.ones(shape, bool)
    if labels is not None:
        table = np.zeros(256, bool)
        table[list(range(1, 256)) if keep is None else list(keep)] = True
        sel = table[labels]
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        inside, _ = domain(coordinate(A, b, shape, u, fs), moving_shape)
        F, M = f.astype(np.float64), m.astype(np.float64)
        n1, sf, sm, sff, smm, sfm = S
        usable = np.isfinite(f) & np.isfinite(m) & (n1 >= 2.0)
        mu_f, mu_m = sf / n1, sm / n1
        c_fm = sfm - (sf * sm) / n1
        c_mm = smm - (sm * sm) / n1
        c_ff = sff - (sf * sf) / n1
        a = c_fm / (c_mm + var_eps * n1)
        a = np.where(a < 0.0, 0.0, np.where(a > a_max, a_max, a))
        d = (F - mu_f) - a * (M - mu_m)
        g = []
        for j in range(3):
            if shape[j] == 1:
                g.append(np.zeros(shape))
                continue
            idx = np.arange(shape[j])
            hi, lo = np.take(M, np.minimum(idx + 1, shape[j] - 1), axis=j), np.take(M, np.maximum(idx - 1, 0), axis=j)
            g.append(a * ((hi - lo) * gs[j]))
        dd = d * d
        den = ((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]) + dd * inv_k2
        still = den < den_min
        steps = [np.where(still, 0.0, (d * g[j]) / den) for j in range(3)]
        nan = np.isnan(a) | np.isnan(den) | np.isnan(steps[0]) | np.isnan(steps[1]) | np.isnan(steps[2])
        c_out = sel & ~inside
        c_nan = sel & inside & (~usable | nan)
        c_in = sel & inside & usable & ~nan
        out = np.empty((3,) + shape, np.float32)
        for j in range(3):
            out[j] = np.where(c_in, (u[j].astype(np.float64) + steps[j]).astype(np.float32), u[j])
        capped = np.where(dd < 16777216.0, dd, 16777216.0)
        res = np.floor(capped * 16.0 + 0.5)[c_in]
        vv = c_mm * c_ff
        rho2 = np.where(vv > 0.0, np.minimum(np.maximum((c_fm * c_fm) / vv, 0.0), 1.0), 0.0)
        rho = np.floor(rho2 * 1048576.0 + 0.5)[c_in]
    total = lambda t: sum(int(v) for v in t.astype(np.int64).reshape(-1))  # noqa: E731  (Python integers: no overflow)
    return out, [int(sel.sum()), int(c_in.sum()), int(c_out.sum()), int(c_nan.sum()), total(res), total(rho)]


# ------------------------------------------------------------------------------------------------ the cases
def pair(shape, seed, correlated=True):
    """(f, m) float32: m an affine map of f plus noise (HU-like), or independent of it."""
    rng = np.random.default_rng(seed)
    f = rng.normal(-600.0, 250.0, shape).astype(np.float32)
    m = (0.7 * f + 120.0 + rng.normal(0.0, 40.0, shape)).astype(np.float32) if correlated else rng.normal(-500.0, 200.0, shape).astype(np.float32)
    return f, m


def check_moments(eng, f, m, radius):
    got, want = eng.local_moments(f, m, radius), moments_oracle(f, m, radius)
    assert same_bits(got, want), (f.shape, radius)
    return got


def check_step(eng, f, m, radius, u, A=None, b=None, moving_shape=None, **kw):
    """The device's step on the device's sums against the restatement on the restated sums -> (out, counts, sums)."""
    A, b = np.eye(3) if A is None else A, np.zeros(3) if b is None else b
    moving_shape = f.shape if moving_shape is None else moving_shape
    S = check_moments(eng, f, m, radius)
    got = eng.lcc_step(f, m, S, u, A, b, moving_shape, **kw)
    want = lcc_step_oracle(f, m, S, u, A, b, moving_shape, **kw)
    assert same_bits(got[0], want[0]) and got[1] == want[1], (f.shape, radius, got[1], want[1])
    c = got[1]
    assert c[0] == c[1] + c[2] + c[3]  # the count invariant
    # the step-length bound 1 / (2 sqrt(inv_k2)), in the field's unit; each component of out is rounded to float32 once
    limit = 1.0 / (2.0 * np.sqrt(kw.get("inv_k2", 1.0)))
    step = (got[0].astype(np.float64) - u.astype(np.float64))
    length = np.sqrt(sum(step[j] ** 2 for j in range(3)))
    ok = np.isfinite(length)
    slack = 2.0 * float(np.spacing(np.float32(np.abs(u[np.isfinite(u)]).max() + limit)))
    assert np.all(length[ok] <= limit * (1.0 + 1e-12) + slack), (length[ok].max(), limit)
    return got[0], c, S


SHAPE_CASES = [((5, 7, 9), (1, 2, 3)), ((1, 6, 8), (0, 2, 3)), ((1, 6, 8), (3, 2, 3)), ((3, 4, 70), (8, 8, 8)), ((5, 7, 9), (2, 0, 1)),
               ((5, 7, 9), (0, 3, 0)), ((4, 5, 6), (0, 0, 0))]
SPACING = (2.5, 0.7, 0.8)


def run_shape_case(eng, shape, radius, seed=0):
    f, m = pair(shape, 50 + seed)
    u = make_field("random", shape, 51 + seed, SPACING)
    _, c, _ = check_step(eng, f, m, radius, u, spacing=SPACING, inv_k2=0.25)
    assert c[1] > 0 or max(radius) == 0  # (a window of one voxel has N = 1: nothing contributes)
    if max(radius) == 0:
        assert c[1] == 0 and c[3] == c[0] - c[2]


def run_nan_and_labels(eng):
    shape = (5, 7, 9)
    f, m = pair(shape, 60)
    f, m = f.copy(), m.copy()
    f[1, 2, 3], f[4, 6, 8], m[2, 3, 4], m[0, 0, 0], m[3, 3, 3] = np.nan, np.inf, np.nan, -np.inf, np.nan
    u = make_field("random", shape, 61)
    S = check_moments(eng, f, m, (1, 2, 3))
    assert S[0].max() < 3 * 5 * 7 and S[0].min() >= 1 and np.all(np.isfinite(S))
    _, c, _ = check_step(eng, f, m, (1, 2, 3), u)
    assert c[3] >= 5  # the five voxels themselves, and the neighbours whose gradient meets a NaN
    labels = np.random.default_rng(62).integers(0, 4, shape).astype(np.uint8)
    out, c, _ = check_step(eng, f, m, (1, 2, 3), u, labels=labels, keep=(1, 3))
    assert c[0] == int(np.isin(labels, (1, 3)).sum()) and same_bits(out[:, ~np.isin(labels, (1, 3))], u[:, ~np.isin(labels, (1, 3))])
    check_step(eng, f, m, (1, 2, 3), u, labels=labels)  # keep=None: every label >= 1
    # nothing valid at all: every sum is zero, nothing contributes
    S = check_moments(eng, np.full(shape, np.nan, np.float32), m, 2)
    assert not S.any()


def run_outside(eng):
    """A field that sends a corner outside the moving volume."""
    shape = (5, 7, 9)
    f, m = pair(shape, 63)
    u = np.zeros((3,) + shape, np.float32)
    u[:, 0, 0, 0] = -3.0
    u[2, 4, 6, 8] = 2.0
    out, c, _ = check_step(eng, f, m, 2, u)
    assert c[2] == 2 and same_bits(out[:, 0, 0, 0], u[:, 0, 0, 0])
    # a smaller moving volume under a shift: a whole face is outside
    _, c, _ = check_step(eng, f, m, 2, np.zeros_like(u), b=np.array([0.0, 0.0, -2.0]), moving_shape=(5, 7, 6))
    assert c[2] > 5 * 7


def run_special_windows(eng):
    shape = (5, 7, 9)
    f, _ = pair(shape, 64)
    f = np.rint(f).astype(np.float32)
    u = np.random.default_rng(65).uniform(-0.4, 0.4, (3,) + shape).astype(np.float32)  # (below half a voxel: no voxel is outside)
    # a constant m: the gain may be a rounding residue, the gradient is exactly zero -- no voxel moves
    out, c, _ = check_step(eng, f, np.full(shape, -700.0, np.float32), 2, u)
    assert c[1] == c[0] and same_bits(out, u)
    # m = 2 f + 100 exactly: a = 1 / 2 up to var_eps, the residual vanishes and the correlation is 1 in every window
    m = (2.0 * f + 100.0).astype(np.float32)
    assert np.array_equal(m.astype(np.float64), 2.0 * f.astype(np.float64) + 100.0)
    _, c, _ = check_step(eng, f, m, 2, u, var_eps=1e-9)
    assert c[1] == c[0] and c[4] <= c[1] and abs(c[5] - (c[1] << 20)) <= c[1]  # (within one unit of the rounding per voxel)
    # an anti-correlated window: the gain is clamped to 0, so there is no force, while the correlation is still 1
    out, c, _ = check_step(eng, f, (-2.0 * f + 100.0).astype(np.float32), 2, u, var_eps=1e-9)
    assert c[1] == c[0] and same_bits(out, u) and abs(c[5] - (c[1] << 20)) <= c[1]
    # the gain's upper clamp: m = f / 16 would need a = 16
    _, c, _ = check_step(eng, f, (f / 16.0).astype(np.float32), 2, u, var_eps=0.0, a_max=4.0)
    assert c[1] == c[0] and c[4] > 16 * c[1]
    # var_eps = 0 on a constant window: 0 / 0, counted as NaN
    _, c, _ = check_step(eng, f, np.zeros(shape, np.float32), 2, u, var_eps=0.0)
    assert c[3] == c[0] and c[1] == 0


# ------------------------------------------------------------------------------------------------ a loop of five iterations
def oracle_level_lcc(fixed_l, moving_l, labels_l, keep, u, A, b, spacing, radius, iterations, taps, inv_k2, den_min, var_eps, a_max, patience):
    """`deformable.run_level_lcc` written with the restatements -> (field, metrics, reason)."""
    rule, metrics, why = dfm.StopRule(patience), [], "iterations"
    for _ in range(iterations):
        m = warp_oracle(moving_l, u, A, b, fixed_l.shape, "linear", np.nan, np.float32, spacing)
        S = moments_oracle(fixed_l, m, radius)
        v, c = lcc_step_oracle(fixed_l, m, S, u, A, b, moving_l.shape, spacing, inv_k2, den_min, var_eps, a_max, labels_l, keep)
        u = np.stack([oracle_separable(v[i], None, taps) for i in range(3)])
        metrics.append([c[4], c[1], c[5]])
        stop = rule.update((c[4], c[1]))
        if stop is not None:
            why = stop
            break
    return u, metrics, why


def device_level_lcc(eng, fixed_l, moving_l, labels_l, keep, u, A, b, grid, radius, iterations, taps, inv_k2, den_min, var_eps, a_max, patience):
    with eng.scope() as dev:
        ud, vd, counts = dev.upload(u), dev.empty(u.shape, np.float32), dev.empty((6,), np.int64)
        lcc = dfm.LccLevel(eng, dev.upload(fixed_l), dev.upload(moving_l), dev.upload(labels_l) if labels_l is not None else None, keep, counts,
                           A, b, grid, radius, inv_k2, den_min, var_eps, a_max, dev)
        ran, metrics, why = dfm.run_level_lcc(lcc, ud, vd, iterations, taps, patience)
        eng.sync()
        return ud.download(), metrics, why


def run_five_iterations(eng):
    fixed, moving, _ = quality_pair(1.6)
    fixed, moving = fixed[4:20, 8:32, 8:36].astype(np.float32), moving[2:20, 8:34, 6:36].astype(np.float32)  # (two different extents)
    grid = rs.Grid(fixed.shape, (0.8, 0.7, 2.5))
    labels = np.zeros(fixed.shape, np.uint8)
    labels[2:-2, 3:-3, 3:-3] = 1
    taps, inv_k2 = dfm.field_taps(grid, None), dfm.level_inv_k2(grid, None)
    u0 = np.zeros((3,) + fixed.shape, np.float32)
    A, b = np.eye(3), np.array([2.0, 0.0, 2.0])
    for lab in (None, labels):
        got = device_level_lcc(eng, fixed, moving, lab, None, u0, A, b, grid, (2, 3, 3), 5, taps, inv_k2, 1e-9, 25.0, 4.0, 5)
        want = oracle_level_lcc(fixed, moving, lab, None, u0, A, b, (2.5, 0.7, 0.8), (2, 3, 3), 5, taps, inv_k2, 1e-9, 25.0, 4.0, 5)
        assert same_bits(got[0], want[0]) and got[1] == want[1] and got[2] == want[2] == "iterations"
        assert len(got[1]) == 5 and got[1][-1][2] * got[1][0][1] > got[1][0][2] * got[1][-1][1]  # the local correlation rose


# ------------------------------------------------------------------------------------------------ the quality pairs
AIR = -1000.0
_PAIRS, _RUNS = {}, {}


def true_field():
    n, h, w = RECOVERY_SHAPE
    z, y, x = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    sz, sy, sx = np.sin(2 * np.pi * z / (n - 1)), np.sin(2 * np.pi * y / (h - 1)), np.sin(2 * np.pi * x / (w - 1))
    env = np.sin(np.pi * z / (n - 1)) * np.sin(np.pi * y / (h - 1)) * np.sin(np.pi * x / (w - 1))  # zero at the border
    u = np.stack([2.0 * env * sy, 2.0 * env * sx, 2.0 * env * sz])
    u *= 2.0 / np.abs(u).max()
    return (z, y, x), u


def determinant(u):
    """det(I + grad u) by numpy's central differences (one-sided at the border), u in voxels."""
    a = [[(1.0 if i == j else 0.0) + np.gradient(u[i], axis=j) for j in range(3)] for i in range(3)]
    return (a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0])) + \
        a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0])


def quality_pair(s):
    """(fixed int16, moving int16, the true field in voxels) of an inspiration / expiration pair: moving(o) = content(o),
    fixed(o) = air + (content(o + u(o)) - air) / (s * J(o)), each with its own N(0, 20) noise."""
    if s not in _PAIRS:
        (z, y, x), u = true_field()
        rng = np.random.default_rng(11)
        fixed = AIR + (content(z + u[0], y + u[1], x + u[2]) - AIR) / (s * determinant(u))
        fixed = np.rint(fixed + rng.normal(0.0, 20.0, z.shape)).astype(np.int16)
        moving = np.rint(content(z, y, x) + rng.normal(0.0, 20.0, z.shape)).astype(np.int16)
        for a in (fixed, moving, u):
            a.setflags(write=False)
        _PAIRS[s] = (fixed, moving, u)
    return _PAIRS[s]


def end_point_error(field, truth):
    """The mean length of field - truth in voxels over the voxels at least 3 from the border."""
    inner = (slice(None),) + (slice(3, -3),) * 3
    return float(np.sqrt(((np.asarray(field, np.float64) - truth)[inner] ** 2).sum(axis=0)).mean())


def quality_run(eng, s, metric, key):
    """`register_deformable` of the pair `s` with `metric`, once per engine kind (`key`)."""
    if (key, s, metric) not in _RUNS:
        fixed, moving, _ = quality_pair(s)
        _RUNS[(key, s, metric)] = dfm.register_deformable(fixed, moving, engine=eng, metric=metric, **RECOVERY_KW)
    return _RUNS[(key, s, metric)]


def check_quality(eng, s, key):
    truth = quality_pair(s)[2]
    lcc, ssd = quality_run(eng, s, "lcc", key), quality_run(eng, s, "ssd", key)
    zero, e_lcc, e_ssd = end_point_error(np.zeros_like(truth), truth), end_point_error(lcc.field.array, truth), end_point_error(ssd.field.array, truth)
    _, info = lcc.jacobian(engine=eng)
    meta = lcc.meta()
    rho0, rho1 = meta["initial_local_correlation"], meta["final_local_correlation"]
    print(f"s = {s}: end-point error zero field {zero:.3f}, ssd {e_ssd:.3f} ({ssd.folding['folded']} folded), lcc {e_lcc:.3f} "
          f"({lcc.folding['folded']} folded), lcc / ssd {e_lcc / e_ssd:.3f}; Jacobian {info['min']:.3f} .. {info['max']:.3f}; local "
          f"correlation {rho0:.4f} -> {rho1:.4f}; iterations {[lv['iterations'] for lv in lcc.levels]} ({[lv['stopped'] for lv in lcc.levels]})")
    assert e_lcc < zero                       # conditions 1 and 4
    if s == 1.6:
        assert e_lcc <= 0.5 * e_ssd           # condition 2
        assert lcc.folding == {"folded": 0, "nonfinite": 0} and info["folded"] == 0  # condition 3
    assert rho1 > rho0                        # condition 5
    assert meta["metric"] == "lcc" and meta["window_voxels"] == [[4, 4, 4], [4, 4, 4]] and ssd.meta()["metric"] == "ssd"
    assert "window_voxels" not in ssd.meta() and all(len(it) == 3 for lv in lcc.levels for it in lv["metric"])
    for lv in lcc.levels:
        assert dfm.run_stop_rule(lv["metric"], dfm.PATIENCE) == (lv["iterations"], lv["stopped"])
    return lcc


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("shape,radius", SHAPE_CASES, ids=lambda v: "x".join(map(str, v)))
def test_moments_and_step(emu_engine, shape, radius):
    run_shape_case(emu_engine, shape, radius)


def test_nan_voxels_and_labels(emu_engine):
    run_nan_and_labels(emu_engine)


def test_outside(emu_engine):
    run_outside(emu_engine)


def test_special_windows(emu_engine):
    run_special_windows(emu_engine)


def test_five_iterations_equal_the_restated_loop(emu_engine):
    run_five_iterations(emu_engine)


@pytest.mark.parametrize("s", [1.6, 1.0])
def test_quality(emu_engine, s):
    check_quality(emu_engine, s, "emu")


def test_apply_deformable_and_apply_pair_reach_the_metric(emu_engine, monkeypatch):
    """`metric="lcc"` through LMInferer equals the stand-alone function, in the one-GPU branch and in the detour of the multi-GPU
    forms, and `apply_pair` hands `deformable_kw` on."""
    from lungmask_amd import morphology, registration as reg
    from tests.test_mask_wrappers_emu import Harness
    from tests.test_register_emu import REG_SPACING, RIGID_CASES, lung_classes, registration_case

    fixed, moving, _ = registration_case("rigid", RIGID_CASES["a"])
    labels = (lung_classes(fixed.array) == 1).astype(np.uint8)
    h = Harness(emu_engine, labels)
    try:
        rkw = dict(levels_mm=(8.0,), max_evaluations=20)
        dkw = dict(levels_mm=(8.0, 6.0), iterations=(4, 3), metric="lcc", window_mm=14.0, var_eps=16.0)
        rim = morphology.dilate(fixed.like(labels), 6.0, engine=emu_engine)
        first = reg.register(fixed, moving, "rigid", labels=rim, moving_spacing=REG_SPACING, engine=emu_engine, **rkw)
        want = dfm.register_deformable(fixed, moving, initial=first, labels=rim, moving_spacing=REG_SPACING, engine=emu_engine, **dkw)
        assert want.meta()["metric"] == "lcc" and all(len(it) == 3 for lv in want.levels for it in lv["metric"])
        for host in (False, True):
            if host:
                monkeypatch.setattr(h.inf, "_shard", object())
            out, r = h.inf.apply_deformable(fixed, moving, margin_mm=6.0, moving_spacing=REG_SPACING, register_kw=rkw, **dkw)
            assert np.array_equal(out, labels) and r.levels == want.levels and same_bits(r.field.array, want.field.array)
            assert r.meta()["window_voxels"] == want.meta()["window_voxels"] and r.metric == "lcc"
            assert (r.initial_metric, r.final_metric, r.folding) == (want.initial_metric, want.final_metric, want.folding)
            _, rp, pair = h.inf.apply_pair(fixed, moving, margin_mm=6.0, moving_spacing=REG_SPACING, register_kw=rkw, deformable_kw=dkw,
                                           maps=())
            assert same_bits(rp.field.array, want.field.array) and rp.metric == "lcc" and pair.analysis["lung"]["analysed"] > 0
        with pytest.raises(ValueError, match="metric: one of"):
            h.inf.apply_deformable(fixed, moving, moving_spacing=REG_SPACING, metric="ncc")
        with pytest.raises(TypeError, match="unexpected"):
            h.inf.apply_deformable(fixed, moving, moving_spacing=REG_SPACING, window=3)
    finally:
        monkeypatch.undo()
        h.inf.close()


def test_window_of_a_level():
    grid = rs.Grid((20, 30, 40), (0.7, 0.8, 2.5))  # (spacing x, y, z)
    assert dfm.level_window(grid, None) == [4, 4, 4]
    assert dfm.level_window(grid, 5.0) == [2, 6, 7] and dfm.level_window(grid, 0.1) == [1, 1, 1]
    assert dfm.level_window(grid, (20.0, 1.0, 1.0)) == [8, 1, 1]
    assert dfm.level_window(rs.Grid((1, 30, 40), (1.0, 1.0, 1.0)), None) == [0, 4, 4]
    with pytest.raises(ValueError, match="limit is 8"):
        dfm.level_window(grid, 7.0)
    assert nat.LCC_MAX_RADIUS == 8 and nat.LCC_Q == 1 << 20
