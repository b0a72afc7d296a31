"""lm_field_combine_dev on the emulation library, bit for bit -- the field and all four counts -- against a numpy restatement of the
definition in include/lungmask_hip.h (`combine_oracle`; test_gpu_field.py runs the same `run_*` cases on the device), its exact
properties and refusals, and what lungmask_amd.deformable builds from it: `invert` against the same loop written with the oracle,
`compose`, `inverse_consistency`, and a round trip through a second grid evaluated in numpy.

Shapes: the smallest at which each part can go wrong -- (1, 1, 1), where every tap degenerates; an output of (2, 3, 5) sampling a
field of (4, 2, 7), where the extents differ on every axis; (3, 37, 130), where lines cross the workgroups' shares and the last
workgroup is partial; and a constant pair whose squared difference passes the cap of 256."""
import json
import warnings

import numpy as np
import pytest

from lungmask_amd import _native as nat
from lungmask_amd import deformable as dfm
from lungmask_amd import resample as rs
from tests.test_deform_emu import SHAPES, SPACING, coordinate, domain, make_field, rot_scale, same_bits, scales, trilinear

Q = 4194304  # 2^22: the counts' units per squared unit of the field


# ------------------------------------------------------------------------------------------------ the oracle
def combine_oracle(src, out_shape, A, b, R=None, add=None, coord=None, ref=None, alpha=1.0, beta=1.0, spacing=None):
    """lm_field_combine_dev's definition -> (out float32 [3][N_0][N_1][N_2], counts: four Python integers)."""
    fs, _ = scales(spacing)
    R = np.eye(3) if R is None else np.asarray(R, np.float64).reshape(3, 3)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        c = coordinate(A, b, out_shape, coord, fs)
        inside, _ = domain(c, src.shape[1:])
        s = [trilinear(src[k], c) for k in range(3)]
        out = np.empty((3,) + tuple(out_shape), np.float32)
        d = []
        for j in range(3):
            t = (R[j, 0] * s[0] + R[j, 1] * s[1]) + R[j, 2] * s[2]
            v = beta * t if add is None else alpha * add[j].astype(np.float64) + beta * t
            out[j] = v.astype(np.float32)
            d.append(out[j].astype(np.float64) - (0.0 if ref is None else ref[j].astype(np.float64)))
        d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        nan = np.isnan(d2)
        q = np.floor(np.where(d2 < 256.0, d2, 256.0)[~nan] * float(Q) + 0.5).astype(np.int64)
    total = sum(int(v) for v in q) if q.size < 4096 else int(q.sum())
    return out, [int((~inside).sum()), int(nan.sum()), total, int(q.max()) if q.size else 0]


def check_combine(eng, src, out_shape, A, b, **kw):
    got, counts = eng.field_combine(src, out_shape, A, b, **kw)
    want, wc = combine_oracle(src, out_shape, A, b, **kw)
    assert [counts[k] for k in nat.FIELD_COUNTS] == wc, (counts, wc)
    assert same_bits(got, want), np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5]
    return got, wc


def rand_field(shape, seed, spacing=None):
    return make_field("random", shape, seed, spacing)


ROT = np.array([[0.0, -0.8, 0.6], [1.0, 0.0, 0.0], [0.0, 0.6, 0.8]]) @ np.diag([1.0, -1.0, 0.5])  # a non-trivial R
FIELDS = ["null", "zeros", "shift", "random", "special"]
SHAPE_IDS = ["x".join(map(str, s[0])) for s in SHAPES]


# ------------------------------------------------------------------------------------------------ cases
def run_combine_cases(eng, shapes, kind):
    """Every `make_field` kind as `coord`, rot_scale() as the map, a non-trivial R, all four pointers, alpha and beta not 1."""
    out_shape, src_shape = shapes
    A, b = (np.eye(3), np.zeros(3)) if out_shape == (1, 1, 1) else rot_scale()
    coord = make_field(kind, out_shape, 3, SPACING)
    src, add, ref = rand_field(src_shape, 4, SPACING), rand_field(out_shape, 5, SPACING), rand_field(out_shape, 6, SPACING)
    check_combine(eng, src, out_shape, A, b, R=ROT, add=add, coord=coord, ref=ref, alpha=0.75, beta=-1.25, spacing=SPACING)
    _, counts = check_combine(eng, src, out_shape, A, b, coord=coord, spacing=SPACING)
    if kind == "special":
        assert counts[0] >= 1  # a NaN coordinate is outside


def run_pointer_patterns(eng, shapes):
    """The four uses of the header's table, with their NULL pointers."""
    out_shape, src_shape = shapes
    I, z = np.eye(3), np.zeros(3)
    A, b = rot_scale()
    u, w = rand_field(out_shape, 7, SPACING), rand_field(out_shape, 8, SPACING)
    check_combine(eng, u, out_shape, I, z, coord=w, ref=w, beta=-1.0, spacing=SPACING)              # an inversion step
    u2 = rand_field(src_shape, 9, SPACING)
    check_combine(eng, u2, out_shape, A, b, R=ROT, add=u, coord=u, alpha=1.0, beta=1.0, spacing=SPACING)  # a composition
    zeros = np.zeros((3,) + tuple(out_shape), np.float32)
    check_combine(eng, u2, out_shape, A, b, R=ROT, add=zeros, coord=zeros, spacing=SPACING)           # a transport onto a grid
    check_combine(eng, u, out_shape, I, z, add=w, alpha=1.0, beta=-1.0)                               # a difference
    check_combine(eng, u, out_shape, I, z, add=u, coord=u, ref=u, alpha=0.5, beta=0.5, spacing=SPACING)  # add, coord, src, ref: one buffer


def run_nan_inputs(eng):
    """A NaN in each input: in src it reaches the voxels that sample it, in add and ref its own voxel, in coord it is outside."""
    shape = (3, 5, 7)
    I, z = np.eye(3), np.zeros(3)
    base = {k: rand_field(shape, 10 + i) * np.float32(0.2) for i, k in enumerate(("src", "add", "coord", "ref"))}
    for name in base:
        f = {k: v.copy() for k, v in base.items()}
        f[name][1, 1, 2, 3] = np.nan
        f[name][0, 2, 4, 6] = np.inf
        src = f.pop("src")
        _, counts = check_combine(eng, src, shape, I, z, **f)
        if name == "coord":  # (clamped to an edge: what is sampled there is a number)
            assert counts[0] >= 2
        else:
            assert counts[1] >= 1, name


def run_cap(eng):
    """A constant difference of (20, 20, 20): d2 = 1200 passes the cap of 256, every voxel counts 2^30."""
    shape = (5, 7, 9)
    src, ref = np.full((3,) + shape, 20.0, np.float32), np.zeros((3,) + shape, np.float32)
    got, counts = check_combine(eng, src, shape, np.eye(3), np.zeros(3), ref=ref)
    n = int(np.prod(shape))
    assert counts == [0, 0, n * 2 ** 30, 2 ** 30] and np.all(got == 20.0)
    src[:] = np.float32(2.0 ** -11)  # one unit of the resolution along one axis: q = 1
    src[1:] = 0.0
    assert check_combine(eng, src, shape, np.eye(3), np.zeros(3))[1] == [0, 0, n, 1]


def run_properties(eng):
    shape = (3, 37, 130)
    I, z = np.eye(3), np.zeros(3)
    u, v = rand_field(shape, 20), rand_field(shape, 21)
    got, counts = check_combine(eng, u, shape, I, z)
    assert same_bits(got, u) and counts[0] == 0                      # the identity: the source comes back
    assert same_bits(check_combine(eng, u, shape, I, z, beta=-1.0)[0], -u)
    got, _ = check_combine(eng, u, shape, I, z, add=v, alpha=1.0, beta=-1.0)
    assert same_bits(got, (v.astype(np.float64) - u.astype(np.float64)).astype(np.float32))
    _, counts = check_combine(eng, u, shape, I, z, ref=u)            # ref = the result: no difference
    assert counts == [0, 0, 0, 0]
    # with R = I, no add and beta = 1, component j is lm_warp_dev's linear gather of src_j wherever the coordinate is inside
    for out_shape, src_shape in SHAPES:
        A, b = rot_scale()
        coord, src = rand_field(out_shape, 22, SPACING), rand_field(src_shape, 23)
        got, counts = check_combine(eng, src, out_shape, A, b, coord=coord, spacing=SPACING)
        inside, _ = domain(coordinate(A, b, out_shape, coord, scales(SPACING)[0]), src_shape)
        assert counts[0] == int((~inside).sum())
        for j in range(3):
            old = eng.warp(src[j], coord, A, b, out_shape, "linear", -7.0, np.float32, SPACING)
            assert same_bits(got[j][inside], old[inside]) and np.all(old[~inside] == -7.0)
    # a whole-voxel shift equals np.roll in the interior (a power-of-two spacing, so that coord / spacing is exact)
    sp = (2.0, 0.5, 4.0)
    shape = (6, 9, 12)
    src = rand_field(shape, 24)
    got, counts = check_combine(eng, src, shape, I, z, coord=make_field("shift", shape, spacing=sp), spacing=sp)
    rolled = np.roll(src, (-1, 2, -3), axis=(1, 2, 3))
    assert same_bits(got[:, :5, 2:, :9], rolled[:, :5, 2:, :9]) and counts[0] == 6 * 9 * 12 - 5 * 7 * 9
    assert same_bits(got[:, 5, 2:, :9], src[:, 5, :7, 3:])  # outside: the edge value, not a fill


def run_dirty_outputs(eng):
    """`out` is fully written and `counts` zeroed by the call; without counts the field is the same."""
    shape = (2, 3, 5)
    u = rand_field(shape, 25)
    want, wc = combine_oracle(u, shape, np.eye(3), np.zeros(3), ref=u, beta=-1.0)
    with eng.scope() as dev:
        ud, out, counts = dev.upload(u), dev.empty(u.shape, np.float32), dev.empty((4,), np.int64)
        out.upload(np.full(u.shape, -77.0, np.float32))
        counts.upload(np.full(4, -1, np.int64))
        eng.field_combine_dev(ud, shape, np.eye(3), np.zeros(3), ref=ud, beta=-1.0, out=out, counts=counts)
        eng.sync()
        assert same_bits(out.download(), want) and [int(v) for v in counts.download()] == wc
        again = dev.add(eng.field_combine_dev(ud, shape, np.eye(3), np.zeros(3), beta=-1.0))
        eng.sync()
        assert same_bits(again.download(), want)


# ------------------------------------------------------------------------------------------------ invert, compose
FIXED = rs.Grid((20, 30, 32), (0.8, 0.75, 2.0), (-12.0, 30.0, 4.5), [[0, 1, 0], [1, 0, 0], [0, 0, -1]])
MOVING = rs.Grid((26, 40, 44), (0.7, 0.7, 1.8), (12.5, 27.5, -37.0), [[0, -1, 0], [1, 0, 0], [0, 0, 1]])  # (covers FIXED's box by ~3 mm)
ROUND_TRIP_BAR_MM = 0.5 * min(FIXED.spacing)  # "sub-voxel": half the fixed grid's smallest spacing


def smooth_field(grid, seed=0, peak_mm=3.0):
    """Three Gaussian blobs per component (sigma 5 to 8 mm, centres inside the box), scaled to a longest vector of `peak_mm`."""
    rng = np.random.default_rng(seed)
    sp = np.asarray(dfm.spacing_zyx(grid))
    o = np.meshgrid(*[np.arange(n, dtype=np.float64) * s for n, s in zip(grid.shape, sp)], indexing="ij")
    box = (np.asarray(grid.shape) - 1) * sp
    f = np.zeros((3,) + grid.shape)
    for i in range(3):
        for _ in range(3):
            centre, sigma, amp = rng.uniform(0.2, 0.8, 3) * box, rng.uniform(5.0, 8.0), rng.uniform(1.0, 2.5) * rng.choice((-1.0, 1.0))
            f[i] += amp * np.exp(-sum((o[a] - centre[a]) ** 2 for a in range(3)) / (2.0 * sigma * sigma))
    f *= peak_mm / np.sqrt((f ** 2).sum(axis=0)).max()
    return f.astype(np.float32)


def gradient_norm(field, grid):
    """The largest singular value of the field's gradient (mm per mm), central differences."""
    sp = dfm.spacing_zyx(grid)
    G = np.stack([np.stack([np.gradient(field[i].astype(np.float64), sp[j], axis=j) for j in range(3)], axis=-1) for i in range(3)], axis=-2)
    return float(np.linalg.svd(G, compute_uv=False).max())


def oracle_invert(u, spacing, iterations, tolerance_mm):
    """`deformable.invert`'s step one written with the oracle -> (w, the max count of every iteration, converged)."""
    _, threshold = dfm.check_inversion(iterations, tolerance_mm)
    shape = u.shape[1:]
    w, peaks = np.zeros_like(u), []
    for _ in range(iterations):
        w, c = combine_oracle(u, shape, np.eye(3), np.zeros(3), coord=w, ref=w, beta=-1.0, spacing=spacing)
        peaks.append(c[3])
        if c[3] <= threshold:
            return w, peaks, True
    return w, peaks, False


def run_invert_constant(eng):
    grid = rs.Grid((4, 6, 9), (0.8, 0.7, 2.5))
    d = np.array([1.25, -0.3, 2.7], np.float32)
    field = dfm.DisplacementField(np.broadcast_to(d.reshape(3, 1, 1, 1), (3,) + grid.shape), grid)
    inv, info = dfm.invert(field, engine=eng)
    assert same_bits(inv.array, -field.array) and inv.grid is grid
    assert (info["iterations"], info["converged"], info["residual_max_mm"], info["residual_rms_mm"]) == (2, True, 0.0, 0.0)
    assert len(info["residuals"]) == 2 and abs(info["residuals"][0] - float(np.sqrt((d.astype(np.float64) ** 2).sum()))) <= 2.0 ** -11
    json.dumps(info)
    # zeros under an affine, onto another grid: zeros under the inverse affine
    T = rs.Affine.rotation((0, 0, 1), 5.0).compose(rs.Affine.translation((1.0, -2.0, 0.5)))
    inv, info = dfm.invert(dfm.DisplacementField.zeros(FIXED, T), onto=MOVING, engine=eng)
    assert not inv.array.any() and inv.grid is MOVING and info["converged"] and info["iterations"] == 1
    assert np.array_equal(inv.affine.matrix, T.inverse().matrix) and np.array_equal(inv.affine.translation_vector, T.inverse().translation_vector)


def run_invert_smooth(eng):
    """The residuals and the field equal the loop written with the oracle; the consistency figure is the next residual."""
    u = smooth_field(FIXED, 1)
    rate = gradient_norm(u, FIXED)
    assert rate < 0.6  # a contraction
    field = dfm.DisplacementField(u, FIXED)
    tol = 0.005
    inv, info = dfm.invert(field, tolerance_mm=tol, engine=eng)
    want, peaks, converged = oracle_invert(u, dfm.spacing_zyx(FIXED), 30, tol)
    assert same_bits(inv.array, want) and converged and info["converged"] and info["iterations"] == len(peaks)
    assert info["residuals"] == [dfm._q_mm(q) for q in peaks] and info["residual_max_mm"] == info["residuals"][-1] <= tol
    assert info["nonfinite"] == 0 and 0.0 < info["residual_rms_mm"] <= info["residual_max_mm"]
    ratios = [b / a for a, b in zip(info["residuals"][1:-1], info["residuals"][2:])]
    print(f"invert: gradient norm {rate:.3f}, {info['iterations']} iterations to {info['residual_max_mm']:.5f} mm, step ratios "
          f"{min(ratios):.2f} .. {max(ratios):.2f}, outside {info['outside']}")
    assert max(ratios) < 1.0
    ic = dfm.inverse_consistency(inv, field, engine=eng)
    assert ic["max_mm"] <= tol and ic["nonfinite"] == 0 and ic["rms_mm"] <= ic["max_mm"]
    return inv, info


def run_invert_folded(eng):
    """A ramp of slope -1.5 along x on a slab (the folding field of the Jacobian's test): no inverse, no convergence, no exception."""
    fold = np.zeros((3, 4, 9, 20), np.float32)
    fold[2, :, :, 8:14] = -1.5 * np.arange(6, dtype=np.float32)
    inv, info = dfm.invert(dfm.DisplacementField(fold, rs.Grid(fold.shape[1:])), iterations=12, engine=eng)
    assert info["converged"] is False and info["iterations"] == 12 and info["residual_max_mm"] > 1.0 and len(info["residuals"]) == 12
    assert np.all(np.isfinite(inv.array))


def physical(grid, idx):
    """LPS positions [..., 3] of array indices given as three arrays (z, y, x)."""
    xyz = np.stack([idx[2] * grid.spacing[0], idx[1] * grid.spacing[1], idx[0] * grid.spacing[2]], axis=-1)
    return xyz @ grid.direction.T + np.asarray(grid.origin)


def to_index(grid, pts):
    """Array indices (three arrays z, y, x) of LPS positions [..., 3]."""
    xyz = ((pts - np.asarray(grid.origin)) @ grid.direction) / np.asarray(grid.spacing)
    return [xyz[..., 2], xyz[..., 1], xyz[..., 0]]


def transform_points(field, idx):
    """T(x) = affine(x + u(x)) in numpy for the points at the (fractional) indices `idx` of the field's grid: u trilinear."""
    u = np.stack([trilinear(field.array[k], idx) for k in range(3)], axis=-1)  # (z, y, x) components
    return field.affine.apply(physical(field.grid, idx) + u[..., ::-1] @ field.grid.direction.T)


def run_round_trip(eng):
    """|T^-1(T(x)) - x| in numpy stays below half the fixed grid's smallest spacing wherever T(x) is inside the moving grid."""
    centre = FIXED.index_to_physical([(n - 1) / 2.0 for n in FIXED.shape])
    T = rs.Affine.translation((1.5, -2.0, 1.0)).compose(rs.Affine.rotation((0.2, -0.1, 1.0), 5.0, centre))
    field = dfm.DisplacementField(smooth_field(FIXED, 2), FIXED, T)
    inv, info = dfm.invert(field, onto=MOVING, engine=eng)
    assert info["converged"] and inv.grid is MOVING and np.allclose(inv.affine.compose(T).matrix, np.eye(3), atol=1e-12)
    o = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in FIXED.shape], indexing="ij")
    x = physical(FIXED, o)
    y = transform_points(field, o)
    m = to_index(MOVING, y)
    inside = np.ones(FIXED.shape, bool)
    for a in range(3):
        inside &= (m[a] >= 0.0) & (m[a] <= MOVING.shape[a] - 1.0)
    err = np.sqrt(((transform_points(inv, m) - x) ** 2).sum(axis=-1))
    deep = inside.copy()
    for a in range(3):
        deep &= (m[a] >= 4.0) & (m[a] <= MOVING.shape[a] - 5.0)
    print(f"round trip: {int(inside.sum())} of {inside.size} voxels inside, error {err[inside].max():.4f} mm at most, {err[deep].max():.4f} mm "
          f"at least four voxels inside; {info['iterations']} iterations to {info['residual_max_mm']:.5f} mm; bar {ROUND_TRIP_BAR_MM} mm")
    assert inside.sum() > 0.5 * inside.size
    assert err[inside].max() < ROUND_TRIP_BAR_MM
    ic = dfm.inverse_consistency(field, inv, engine=eng)
    assert ic["nonfinite"] == 0 and 0 < ic["outside"] < inside.size
    return err[inside].max()


def run_compose(eng):
    # on one grid whose index map is the exact identity (power-of-two spacings): zeros on either side change nothing
    grid = rs.Grid((3, 7, 10), (0.5, 2.0, 1.0), (3.0, -1.0, 2.0))
    f = dfm.DisplacementField(rand_field(grid.shape, 30, dfm.spacing_zyx(grid)), grid)
    zeros = dfm.DisplacementField.zeros(grid)
    for got in (dfm.compose(f, zeros, engine=eng), dfm.compose(zeros, f, engine=eng)):
        assert same_bits(got.array, f.array) and got.grid is grid and np.array_equal(got.affine.matrix, np.eye(3))
    # two constant fields add, through a rotated affine and two different directions: the expected vector, in LPS, in numpy
    T1 = rs.Affine.rotation((0, 0.3, 1), 5.0, (2.0, 1.0, -3.0)).compose(rs.Affine.scale((1.02, 0.97, 1.05)))
    T2 = rs.Affine.rotation((1, 0, 0), -3.0).compose(rs.Affine.translation((0.5, 1.0, -1.5)))
    d1, d2 = np.array([1.25, -0.5, 2.0], np.float32), np.array([-0.75, 1.5, 0.6], np.float32)
    first = dfm.DisplacementField(np.broadcast_to(d1.reshape(3, 1, 1, 1), (3,) + FIXED.shape), FIXED, T1)
    second = dfm.DisplacementField(np.broadcast_to(d2.reshape(3, 1, 1, 1), (3,) + MOVING.shape), MOVING, T2)
    got = dfm.compose(first, second, engine=eng)
    lps = FIXED.direction @ d1[::-1].astype(np.float64) + np.linalg.inv(T1.matrix) @ (MOVING.direction @ d2[::-1].astype(np.float64))
    want = (FIXED.direction.T @ lps)[::-1]
    assert got.grid is FIXED and np.allclose(got.affine.matrix, T2.matrix @ T1.matrix, atol=1e-15)
    assert np.allclose(got.affine.translation_vector, T2.matrix @ T1.translation_vector + T2.translation_vector, atol=1e-12)
    for k in range(3):  # one float32 rounding of the sum, and the float64 sums' own
        assert np.all(np.abs(got.array[k].astype(np.float64) - want[k]) <= np.spacing(np.float32(abs(want[k])))), (k, want[k], got.array[k].ravel()[:3])
    # the composed transform maps a point where the two transforms map it one after the other
    x = physical(FIXED, [np.array([7.0]), np.array([11.0]), np.array([13.0])])
    once = got.affine.apply(x + got.lps()[7, 11, 13])
    twice = T2.apply(T1.apply(x + first.lps()[7, 11, 13]) + second.lps()[0, 0, 0])
    assert np.allclose(once, twice, atol=1e-5)


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("kind", FIELDS)
@pytest.mark.parametrize("shapes", SHAPES, ids=SHAPE_IDS)
def test_combine(emu_engine, shapes, kind):
    run_combine_cases(emu_engine, shapes, kind)


@pytest.mark.parametrize("shapes", SHAPES, ids=SHAPE_IDS)
def test_pointer_patterns(emu_engine, shapes):
    run_pointer_patterns(emu_engine, shapes)


def test_nan_in_each_input(emu_engine):
    run_nan_inputs(emu_engine)


def test_cap_and_resolution(emu_engine):
    run_cap(emu_engine)


def test_exact_properties(emu_engine):
    run_properties(emu_engine)


def test_dirty_outputs(emu_engine):
    run_dirty_outputs(emu_engine)


def test_refusals(emu_engine):
    eng = emu_engine
    I, z = np.eye(3), np.zeros(3)
    lib = eng.L.lib
    with eng.scope() as dev:
        u, v = dev.upload(np.zeros((3, 2, 3, 4), np.float32)), dev.upload(np.zeros((3, 2, 3, 4), np.float32))
        out, counts = dev.empty((3, 2, 3, 4), np.float32), dev.empty((4,), np.int64)
        for kw in (dict(), dict(add=out), dict(coord=out), dict(ref=out)):  # out aliasing an input
            with pytest.raises(nat.LMError, match="in-place"):
                eng.field_combine_dev(out if not kw else u, (2, 3, 4), I, z, out=out, **kw)
        p = nat.FieldCombineParams()
        p.out_dims[:] = [2, 3, 4]
        p.A[:] = p.R[:] = list(np.eye(3).reshape(9))
        p.field_scale[:] = [1.0, 1.0, 1.0]
        p.alpha = p.beta = 1.0
        call = lambda add, coord, src, ref, o, c=None: lib.lm_field_combine_dev(eng.h, add, coord, src, 2, 3, 4, ref, p, o, c)  # noqa: E731
        assert call(None, None, u.ptr, None, out.ptr, counts.ptr) == 0 and call(v.ptr, v.ptr, u.ptr, v.ptr, out.ptr) == 0
        for args in ((None, None, out.ptr, None), (out.ptr, None, u.ptr, None), (None, out.ptr, u.ptr, None), (None, None, u.ptr, out.ptr)):
            assert call(*args, out.ptr) < 0 and b"in-place" in lib.lm_last_error()
        assert call(None, None, None, None, out.ptr) < 0 and b"bad arguments" in lib.lm_last_error()
        assert call(None, None, u.ptr, None, None) < 0 and b"bad arguments" in lib.lm_last_error()
        for name, pos in (("A", 4), ("b", 1), ("R", 8), ("field_scale", 2)):  # non-finite parameters
            for bad in (np.nan, np.inf, -np.inf):
                keep = getattr(p, name)[pos]
                getattr(p, name)[pos] = bad
                assert call(None, None, u.ptr, None, out.ptr) < 0 and b"finite" in lib.lm_last_error(), name
                assert lib.lm_last_error() == b"lm_field_combine_dev: field_scale, A, b, R, alpha and beta must be finite"
                getattr(p, name)[pos] = keep
        for name in ("alpha", "beta"):
            setattr(p, name, np.nan)
            assert call(None, None, u.ptr, None, out.ptr) < 0 and b"finite" in lib.lm_last_error()
            setattr(p, name, 1.0)
        p.out_dims[2] = 4097  # the dimension limits, refused before anything is read
        assert call(None, None, u.ptr, None, out.ptr) < 0 and b"4096" in lib.lm_last_error()
        p.out_dims[2] = 0
        assert call(None, None, u.ptr, None, out.ptr) < 0 and b"4096" in lib.lm_last_error()
        assert lib.lm_last_error() == b"lm_field_combine_dev: output too large or empty (1 <= out_dims[2] <= 4096, got 0)"  # the whole text
        p.out_dims[:] = [2048, 1024, 1024]
        assert call(None, None, u.ptr, None, out.ptr) < 0
        assert lib.lm_last_error() == b"lm_field_combine_dev: output too large (N_0 * N_1 * N_2 must stay below 2^31)"
        p.out_dims[:] = [2, 3, 4]
        assert lib.lm_field_combine_dev(eng.h, None, None, 8, 1, 1, 4097, None, p, 16, None) < 0 and b"too large" in lib.lm_last_error()
        assert call(None, None, u.ptr, None, out.ptr) == 0
        # a wrong component count, dtype or shape
        with pytest.raises(nat.LMError, match="float32 field"):
            eng.field_combine_dev(dev.upload(np.zeros((2, 2, 3, 4), np.float32)), (2, 3, 4), I, z)
        with pytest.raises(nat.LMError, match="float32 field"):
            eng.field_combine_dev(dev.upload(np.zeros((3, 2, 3, 4), np.float64)), (2, 3, 4), I, z)
        for name in ("add", "coord", "ref"):
            with pytest.raises(nat.LMError, match="field must be"):
                eng.field_combine_dev(u, (2, 3, 4), I, z, **{name: dev.upload(np.zeros((3, 2, 3, 5), np.float32))})
        with pytest.raises(nat.LMError, match="field must be"):
            eng.field_combine_dev(u, (2, 3, 5), I, z, out=out)
        with pytest.raises(nat.LMError, match="counts"):
            eng.field_combine_dev(u, (2, 3, 4), I, z, counts=dev.empty((3,), np.int64))
    with pytest.raises(nat.LMError, match="too large"):
        eng.field_combine(np.zeros((3, 1, 1, 2), np.float32), (1, 1, 4097), I, z)
    with pytest.raises(ValueError, match="out_shape"):
        eng.field_combine(np.zeros((3, 1, 1, 2), np.float32), (1, 2), I, z)
    with pytest.raises(ValueError, match="spacing"):
        eng.field_combine(np.zeros((3, 1, 1, 2), np.float32), (1, 1, 2), I, z, spacing=(1.0, 0.0, 1.0))


def test_invert_constant_and_zero_fields(emu_engine):
    run_invert_constant(emu_engine)


def test_invert_equals_the_oracle_loop(emu_engine):
    run_invert_smooth(emu_engine)


def test_invert_of_a_folded_field_does_not_converge(emu_engine):
    run_invert_folded(emu_engine)


def test_round_trip_through_a_second_grid(emu_engine):
    """Measured on the emulation library (the device gives the same bits): 19 200 fixed voxels, the moving grid of 26 x 40 x 44, a 5
    degree rotation and a translation under a field of 3 mm at most."""
    run_round_trip(emu_engine)


def test_compose(emu_engine):
    run_compose(emu_engine)


def test_registration_inverse_and_resample_to_moving(emu_engine):
    """DeformableRegistration.inverse is `invert(field, onto=the moving grid)`, kept; resample_to_moving warps through it."""
    eng = emu_engine
    T = rs.Affine.translation((1.0, -0.5, 0.25))
    field = dfm.DisplacementField(smooth_field(FIXED, 3, 2.0), FIXED, T)
    reg = dfm.DeformableRegistration(field, [], None, None, {"folded": 0, "nonfinite": 0})
    with pytest.raises(ValueError, match="moving grid"):
        reg.inverse(engine=eng)
    reg.moving_grid = MOVING
    assert "inverse" not in reg.meta()
    inv, info = reg.inverse(engine=eng)
    want, winfo = dfm.invert(field, onto=MOVING, engine=eng)
    assert same_bits(inv.array, want.array) and info == winfo and reg.inverse(engine=eng)[0] is inv
    assert reg.meta()["inverse"] == info and reg.inverse_field is inv
    labels = np.zeros(FIXED.shape, np.uint8)
    labels[5:15, 8:22, 6:25] = 1
    labels[5:15, 8:22, 16:25] = 2
    got = reg.resample_to_moving(FIXED.like(labels), engine=eng)
    assert same_bits(got.array, dfm.warp_labels(FIXED.like(labels), inv, "linear", engine=eng).array) and got.array.shape == MOVING.shape
    assert set(np.unique(got.array)) == {0, 1, 2}
    img = FIXED.like(labels.astype(np.int16) * 100)
    assert same_bits(reg.resample_to_moving(img, kind="image", engine=eng).array, dfm.warp_image(img, inv, 1, engine=eng).array)
