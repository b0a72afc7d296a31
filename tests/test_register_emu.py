"""lm_joint_hist_dev on the emulation library, bit for bit against a numpy restatement of the definition in include/lungmask_hip.h
(`joint_hist_oracle`, also used by test_gpu_register.py), its properties and refusals, and a whole registration at the coarse size.

Shapes: the smallest at which each part can go wrong -- (1, 1, 1); extents that differ on every axis; (3, 37, 130), where lines
cross and do not fill a workgroup's share; and a constant (41, 41, 41) volume whose 68 921 full-weight samples pass 2^32 in one bin."""
import numpy as np
import pytest

from lungmask_amd import _native as nat

Q = 65536
INT_MAX, INT_MIN = 2 ** 31 - 1, -(2 ** 31)


# ------------------------------------------------------------------------------------------------ the oracle
def _hu(values):
    """The statistics' HU rule -> (int64 values, nan mask)."""
    v = np.asarray(values)
    if v.dtype.kind in "iu":
        return np.clip(v.astype(np.int64), INT_MIN, INT_MAX), np.zeros(v.shape, bool)
    nan = np.isnan(v)
    with np.errstate(invalid="ignore"):
        r = np.rint(np.where(nan, 0, v).astype(np.float64))
    out = np.where(r >= 2147483648.0, INT_MAX, np.where(r < -2147483648.0, INT_MIN, np.where(np.isfinite(r), r, 0))).astype(np.int64)
    return out, nan


def _bin(hu, lo, width, bins):
    return (np.clip(hu, lo, lo + bins * width - 1) - lo) // width


def joint_hist_oracle(fixed, moving, A, b, bins, fixed_bins, moving_bins, start=(0, 0, 0), step=(1, 1, 1), mode="linear", labels=None,
                      keep=None):
    A, b = np.asarray(A, np.float64).reshape(3, 3), np.asarray(b, np.float64).reshape(3)
    (f_lo, f_w), (m_lo, m_w) = fixed_bins, moving_bins
    hist = np.zeros((bins, bins), np.int64)
    axes = [np.arange(start[i], fixed.shape[i], step[i]) for i in range(3)]
    o = np.stack([g.reshape(-1) for g in np.meshgrid(*axes, indexing="ij")])  # [3][P]
    if labels is not None:
        table = np.zeros(256, bool)
        table[list(range(1, 256)) if keep is None else list(keep)] = True
        o = o[:, table[labels[o[0], o[1], o[2]]]]
    counts = [o.shape[1], 0, 0, 0]
    fhu, fnan = _hu(fixed[o[0], o[1], o[2]])
    counts[3] += int(fnan.sum())
    o, fhu = o[:, ~fnan], fhu[~fnan]
    bi = _bin(fhu, f_lo, f_w, bins)
    od = o.astype(np.float64)
    e = moving.shape
    with np.errstate(invalid="ignore", over="ignore"):
        c = [((A[i, 0] * od[0] + A[i, 1] * od[1]) + A[i, 2] * od[2]) + b[i] for i in range(3)]
        t = [np.floor(ci + 0.5) for ci in c]
        inside = np.ones(o.shape[1], bool)
        for i in range(3):
            inside &= (t[i] >= 0.0) & (t[i] < float(e[i]))
    counts[2] = int((~inside).sum())
    bi = bi[inside]
    c = [ci[inside] for ci in c]
    j = [ti[inside].astype(np.int64) for ti in t]
    if mode == "nearest":
        mhu, mnan = _hu(moving[j[0], j[1], j[2]])
        counts[3] += int(mnan.sum())
        np.add.at(hist, (bi[~mnan], _bin(mhu[~mnan], m_lo, m_w, bins)), Q)
        counts[1] = int((~mnan).sum())
        return hist, counts
    i0, i1, f = [], [], []
    for i in range(3):
        ci = np.minimum(np.maximum(c[i], 0.0), float(e[i] - 1))
        fl = np.floor(ci)
        i0.append(fl.astype(np.int64))
        f.append(ci - fl)
        i1.append(np.minimum(i0[i] + 1, e[i] - 1))
    mv = moving.astype(np.float64)

    def lerp(a, bb, ff):
        return a * (1.0 - ff) + bb * ff

    with np.errstate(invalid="ignore", over="ignore"):
        row = lambda z, y: lerp(mv[z, y, i0[2]], mv[z, y, i1[2]], f[2])  # noqa: E731
        v = lerp(lerp(row(i0[0], i0[1]), row(i0[0], i1[1]), f[1]), lerp(row(i1[0], i0[1]), row(i1[0], i1[1]), f[1]), f[0])
        vnan = np.isnan(v)
        counts[3] += int(vnan.sum())
        v, bi = v[~vnan], bi[~vnan]
        u = np.minimum(np.maximum((v - float(m_lo)) / float(m_w), 0.0), bins - 1.0)
    k0f = np.floor(u)
    k0 = k0f.astype(np.int64)
    k1 = np.minimum(k0 + 1, bins - 1)
    q1 = np.floor((u - k0f) * float(Q) + 0.5).astype(np.int64)
    np.add.at(hist, (bi, k0), Q - q1)
    np.add.at(hist, (bi, k1), q1)
    counts[1] = int(v.size)
    return hist, counts


# ------------------------------------------------------------------------------------------------ cases
def volume(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.uint8:
        return rng.integers(0, 7, shape).astype(np.uint8)
    v = rng.normal(-500.0, 400.0, shape)
    if np.dtype(dtype).kind == "f":
        v = v.astype(dtype)
        flat = v.reshape(-1)
        special = [np.nan, np.inf, -np.inf, 3e9, -3e9, 2147483647.5, 0.5, 1.5, -0.5]
        pos = rng.choice(flat.size, min(len(special), flat.size), replace=False)
        flat[pos] = special[:pos.size]
        return v
    if np.dtype(dtype) == np.int64:
        v = np.rint(v).astype(np.int64)
        flat = v.reshape(-1)
        flat[:: max(1, flat.size // 5)] = [2 ** 40, -(2 ** 40)][0]
        return v
    return np.rint(v).astype(dtype)


def rot_scale():
    a = np.radians(4.0)
    R = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])
    return R @ np.diag([0.8, 1.05, 0.93]), np.array([0.3, -0.7, 1.2])


MAPS = {
    "identity": (np.eye(3), np.zeros(3)),
    "shift": (np.eye(3), np.array([1.0, -2.0, 3.0])),
    "rotation": rot_scale(),
    "permute_flip": (np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]]), np.array([0.0, 0.0, 3.0])),
    "outside": (np.eye(3), np.array([5000.0, 0.0, 0.0])),
}
SHAPES = [((1, 1, 1), (1, 1, 1)), ((5, 7, 9), (4, 6, 11)), ((3, 37, 130), (3, 37, 130))]


def run(eng, fixed, moving, A, b, bins=32, fixed_bins=(-1024, 64), moving_bins=(-1024, 64), **kw):
    return eng.joint_hist(fixed, moving, A, b, bins, fixed_bins=fixed_bins, moving_bins=moving_bins, **kw)


def check(eng, fixed, moving, A, b, bins=32, fixed_bins=(-1024, 64), moving_bins=(-1024, 64), **kw):
    hist, counts = run(eng, fixed, moving, A, b, bins, fixed_bins, moving_bins, **kw)
    want, wc = joint_hist_oracle(fixed, moving, A, b, bins, fixed_bins, moving_bins, **kw)
    got = [counts["sampled"], counts["contributed"], counts["outside"], counts["nan"]]
    assert got == wc, (got, wc)
    assert np.array_equal(hist, want)
    assert int(hist.sum()) == Q * got[1] and got[0] == got[1] + got[2] + got[3]
    return hist, got


@pytest.mark.parametrize("mode", ["linear", "nearest"])
@pytest.mark.parametrize("name", sorted(MAPS))
@pytest.mark.parametrize("shapes", SHAPES, ids=lambda s: "x".join(map(str, s[0])))
def test_maps_and_shapes(emu_engine, shapes, name, mode):
    fixed, moving = volume(shapes[0], np.int16, 1), volume(shapes[1], np.int16, 2)
    A, b = MAPS[name]
    hist, counts = check(emu_engine, fixed, moving, A, b, mode=mode)
    if name == "outside":
        assert counts[1] == 0 and not hist.any() and counts[2] == counts[0]


@pytest.mark.parametrize("mode", ["linear", "nearest"])
@pytest.mark.parametrize("start,step", [((0, 0, 0), (1, 1, 1)), ((1, 2, 3), (2, 3, 4)), ((0, 1, 0), (9, 50, 200)), ((5, 0, 0), (1, 1, 1))])
def test_steps(emu_engine, start, step, mode):
    fixed, moving = volume((5, 37, 130), np.int16, 3), volume((4, 30, 131), np.int16, 4)
    A, b = MAPS["rotation"]
    hist, counts = check(emu_engine, fixed, moving, A, b, start=start, step=step, mode=mode)
    assert (counts[0] == 0 and not hist.any()) == (start[0] >= 5)  # a start beyond the extent: an empty lattice


@pytest.mark.parametrize("bins", [2, 32, 64])
def test_bins(emu_engine, bins):
    fixed, moving = volume((5, 7, 9), np.int16, 5), volume((4, 6, 11), np.int16, 6)
    A, b = MAPS["rotation"]
    width = -(-2048 // bins)
    for mode in ("linear", "nearest"):
        check(emu_engine, fixed, moving, A, b, bins, (-1024, width), (-1000, width + 1), mode=mode)


DTYPES = [np.uint8, np.int16, np.int32, np.int64, np.float32, np.float64]


@pytest.mark.parametrize("mode", ["linear", "nearest"])
@pytest.mark.parametrize("mdtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("fdtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_dtypes(emu_engine, fdtype, mdtype, mode):
    fixed, moving = volume((5, 7, 9), fdtype, 7), volume((4, 6, 11), mdtype, 8)
    A, b = MAPS["rotation"]
    fb = (0, 1) if fdtype == np.uint8 else (-1024, 64)
    mb = (0, 1) if mdtype == np.uint8 else (-1024, 64)
    hist, counts = check(emu_engine, fixed, moving, A, b, 32, fb, mb, mode=mode)
    if np.dtype(fdtype).kind == "f":
        assert counts[3] >= 1  # the NaN of the fixed volume


@pytest.mark.parametrize("mode", ["linear", "nearest"])
def test_labels_and_keep(emu_engine, mode):
    fixed, moving = volume((5, 37, 130), np.float32, 9), volume((5, 37, 130), np.int16, 10)
    labels = np.random.default_rng(11).integers(0, 4, fixed.shape).astype(np.uint8)
    A, b = MAPS["shift"]
    _, all_labels = check(emu_engine, fixed, moving, A, b, labels=labels, mode=mode)
    _, kept = check(emu_engine, fixed, moving, A, b, labels=labels, keep=(1, 3), mode=mode)
    assert kept[0] == int(np.isin(labels, (1, 3)).sum()) < all_labels[0] == int((labels > 0).sum())
    check(emu_engine, fixed, moving, A, b, labels=labels, keep=(2,), start=(1, 0, 2), step=(2, 3, 4), mode=mode)


def test_label_volumes_nearest(emu_engine):
    a, b_ = volume((5, 7, 9), np.uint8, 12), volume((4, 6, 11), np.uint8, 13)
    hist, _ = check(emu_engine, a, b_, *MAPS["identity"], 8, (0, 1), (0, 1), mode="nearest")
    assert hist[:, 7].sum() == 0


def test_constant_volume_passes_2_to_32_in_one_bin(emu_engine):
    vol = np.full((41, 41, 41), -700, np.int16)
    for mode in ("linear", "nearest"):
        hist, counts = check(emu_engine, vol, vol, *MAPS["identity"], 32, (-1024, 64), (-1024, 1), mode=mode)
        assert counts[1] == 68921 and hist[5, 31] == 68921 * Q > 2 ** 32 and np.count_nonzero(hist) == 1


def test_whole_voxel_shift_linear_equals_nearest(emu_engine):
    fixed = volume((5, 37, 130), np.int16, 14)
    moving = np.random.default_rng(15).integers(-20, 40, (6, 30, 128)).astype(np.int16)
    A, b = MAPS["shift"]
    lin, cl = run(emu_engine, fixed, moving, A, b, 64, (-1024, 32), (-20, 1), mode="linear")
    near, cn = run(emu_engine, fixed, moving, A, b, 64, (-1024, 32), (-20, 1), mode="nearest")
    assert np.array_equal(lin, near) and cl == cn and cl["contributed"] > 0


def test_independent_of_workspace_and_output_contents(emu_engine):
    eng = emu_engine
    fixed, moving = volume((3, 37, 130), np.int16, 16), volume((3, 37, 130), np.float32, 17)
    A, b = MAPS["rotation"]
    with eng.scope() as dev:
        fd, md = dev.upload(fixed), dev.upload(moving)
        out = dev.empty((32 * 32 + 4,), np.int64)
        first = eng.joint_hist_dev(fd, md, A, b, out=out).download()
        eng.sync()
        assert eng.debug_fill_workspaces(0xA5) > 0
        second = eng.joint_hist_dev(fd, md, A, b, out=out).download()  # into the dirty output
        out.upload(np.full(32 * 32 + 4, -1, np.int64))
        third = eng.joint_hist_dev(fd, md, A, b, out=out).download()
    want, wc = joint_hist_oracle(fixed, moving, A, b, 32, (-1024, 64), (-1024, 64))
    for got in (first, second, third):
        assert np.array_equal(got[:1024].reshape(32, 32), want) and list(got[1024:]) == wc


@pytest.mark.parametrize("kw,text", [
    (dict(bins=1), "2 .. 64"), (dict(bins=65), "2 .. 64"), (dict(fixed_bins=(-1024, 0)), ">= 1"), (dict(moving_bins=(0, 0)), ">= 1"),
    (dict(step=(1, 0, 1)), ">= 1")])
def test_refusals(emu_engine, kw, text):
    vol = np.zeros((2, 3, 4), np.int16)
    with pytest.raises(nat.LMError, match=text):
        emu_engine.joint_hist(vol, vol, np.eye(3), np.zeros(3), **kw)


def test_refuses_a_dimension_of_4097(emu_engine):
    vol = np.zeros((1, 1, 4097), np.int16)
    with pytest.raises(nat.LMError, match="4096"):
        emu_engine.joint_hist(vol, np.zeros((1, 1, 2), np.int16), np.eye(3), np.zeros(3))
    with pytest.raises(nat.LMError, match="4096"):
        emu_engine.joint_hist(np.zeros((1, 1, 2), np.int16), vol, np.eye(3), np.zeros(3))


# ------------------------------------------------------------------------------------------------ a whole registration
# The fixed image is cut from inside the moving one, so that no fill value enters: moving = the phantom (48, 112, 112) at spacing
# (2.0, 1.5, 1.5); fixed = the inner (36, 88, 88) box, offset (6, 12, 12), of the moving image resampled under a known transform about
# the box's centre (scipy, cubic), plus independent N(0, 20) noise, rounded to int16.
REG_SPACING = (2.0, 1.5, 1.5)
RIGID_CASES = {"a": (3.0, -2.0, 4.0, 3.0, -4.5, 6.0), "b": (-4.0, 3.0, -2.0, 5.0, 2.2, -3.4)}
AFFINE_CASE = RIGID_CASES["a"] + (3.0, -3.0, 2.0, 0.0, 0.0, 0.0)  # a 3 % anisotropic scale
TRE_BOUND_MM = 0.5 * min(REG_SPACING)  # "sub-voxel": half of the fixed grid's smallest spacing
_CASES = {}


def registration_case(kind, parameters):
    """(fixed Volume, moving array, the true Affine from the fixed to the moving space), built once per case."""
    from scipy import ndimage

    from lungmask_amd import resample as rs
    from lungmask_amd import synthetic as syn

    key = (kind, tuple(parameters))
    if key not in _CASES:
        moving = syn.phantom(48, 112, 112)
        moving_grid = rs.Grid.of(moving, REG_SPACING)
        fixed_grid = rs.Grid((36, 88, 88), moving_grid.spacing, tuple(moving_grid.index_to_physical((6, 12, 12))))
        centre = fixed_grid.index_to_physical([(e - 1) / 2.0 for e in fixed_grid.shape])
        truth = rs.Affine.from_parameters(kind, parameters, centre)
        A, b = rs.index_map(moving_grid, fixed_grid, truth)
        img = ndimage.affine_transform(moving.astype(np.float64), A, offset=b, output_shape=fixed_grid.shape, order=3, mode="nearest")
        img = np.rint(img + np.random.default_rng(7).normal(0.0, 20.0, img.shape)).astype(np.int16)
        fixed = fixed_grid.like(img)
        fixed.array.setflags(write=False)
        moving.setflags(write=False)
        _CASES[key] = (fixed, moving, truth)
    return _CASES[key]


def target_registration_error(transform, truth, fixed):
    """(mean, max, mean before registration) in mm of |transform(p) - truth(p)| over the fixed voxels between -950 and -700 HU, every
    fourth of them."""
    from lungmask_amd import resample as rs

    grid = rs.Grid.of(fixed)
    sel = np.argwhere((fixed.array > -950) & (fixed.array < -700))[::4]
    pts = np.asarray(grid.origin) + (sel[:, ::-1] * np.asarray(grid.spacing)) @ grid.direction.T
    d = np.linalg.norm(transform.apply(pts) - truth.apply(pts), axis=1)
    return float(d.mean()), float(d.max()), float(np.linalg.norm(pts - truth.apply(pts), axis=1).mean())


def lung_classes(values):
    """Air, lung, body of the phantom (-1000, -850, +40 HU) as labels 0, 1, 2."""
    return np.digitize(values, (-925, -400)).astype(np.uint8)


@pytest.mark.parametrize("case", sorted(RIGID_CASES))
def test_rigid_registration_is_sub_voxel_at_the_coarse_levels(emu_engine, case):
    from lungmask_amd import registration as reg

    fixed, moving, truth = registration_case("rigid", RIGID_CASES[case])
    r = reg.register(fixed, moving, "rigid", levels_mm=(8.0, 4.0), moving_spacing=REG_SPACING, engine=emu_engine)
    mean, worst, before = target_registration_error(r.transform, truth, fixed)
    print(f"rigid {case}: TRE mean {mean:.4f} mm, max {worst:.4f} mm (before: {before:.2f} mm), {r.evaluations} evaluations")
    assert 6.5 < before < 9.5
    assert mean < TRE_BOUND_MM
    assert [lv["step"] for lv in r.levels] == [[4, 5, 5], [2, 3, 3]]
    assert r.evaluations == sum(lv["evaluations"] for lv in r.levels) + 1 <= 4000
    assert r.kind == "rigid" and r.metric == "nmi" and 1.0 < r.value <= 2.0 and len(r.parameters) == 6
    assert r.counts["sampled"] == r.counts["contributed"] + r.counts["outside"] + r.counts["nan"]
    import json

    meta = json.loads(json.dumps(r.meta()))
    assert meta["matrix"] == [float(v) for v in r.transform.matrix.reshape(-1)] and meta["translation"] == list(r.transform.translation_vector)
    again = reg.register(fixed, moving, "rigid", levels_mm=(8.0, 4.0), moving_spacing=REG_SPACING, engine=emu_engine)
    assert again.parameters == r.parameters and again.evaluations == r.evaluations  # deterministic
    # the result applies unchanged: the moving image on the fixed grid agrees with the fixed image up to the noise of both
    img = r.resample(moving, order=1, moving_spacing=REG_SPACING, engine=emu_engine).array
    assert img.shape == fixed.array.shape and np.abs(img - fixed.array).mean() < 40.0


def test_affine_registration_is_sub_voxel(emu_engine):
    from lungmask_amd import registration as reg

    fixed, moving, truth = registration_case("affine", AFFINE_CASE)
    r = reg.register(fixed, moving, "affine", levels_mm=(4.0,), moving_spacing=REG_SPACING, engine=emu_engine)
    mean, worst, before = target_registration_error(r.transform, truth, fixed)
    print(f"affine: TRE mean {mean:.4f} mm, max {worst:.4f} mm (before: {before:.2f} mm), {r.evaluations} evaluations")
    assert mean < TRE_BOUND_MM and len(r.parameters) == 12 and r.evaluations <= 4000


def test_label_driven_registration_is_sub_voxel(emu_engine):
    """Two uint8 label volumes, mode "nearest": one bin per label.  One level at the full grid: the cost is a step function of the
    parameters whose steps are as fine as the sampling."""
    from lungmask_amd import registration as reg

    fixed, moving, truth = registration_case("rigid", RIGID_CASES["a"])
    r = reg.register(fixed.like(lung_classes(fixed.array)), lung_classes(moving), "rigid", mode="nearest", bins=4, hu_range=(0, 3),
                     levels_mm=(2.0,), moving_spacing=REG_SPACING, engine=emu_engine)
    mean, worst, before = target_registration_error(r.transform, truth, fixed)
    print(f"labels: TRE mean {mean:.4f} mm, max {worst:.4f} mm (before: {before:.2f} mm), {r.evaluations} evaluations")
    assert mean < TRE_BOUND_MM


def test_register_arguments_labels_and_initial(emu_engine):
    from lungmask_amd import registration as reg
    from lungmask_amd import resample as rs

    from scipy import ndimage

    fixed, moving, truth = registration_case("rigid", RIGID_CASES["b"])
    # the lungs and a rim of four voxels: the lungs' inside alone is one grey value and holds no information
    labels = ndimage.binary_dilation(lung_classes(fixed.array) == 1, iterations=4).astype(np.uint8)
    moving_labels = (lung_classes(moving) == 1).astype(np.uint8)
    kw = dict(levels_mm=(8.0,), moving_spacing=REG_SPACING, engine=emu_engine)
    # sampled inside the labels only, about their centroid, from the centroids' translation
    r = reg.register(fixed, moving, "rigid", labels=fixed.like(labels), initial="centroids", moving_labels=moving_labels, **kw)
    grid = rs.Grid.of(fixed)
    np.testing.assert_allclose(r.centre, grid.index_to_physical(reg.label_centroid_index(labels)), atol=1e-9)
    assert r.counts["sampled"] == int(labels[::4, ::5, ::5].sum())
    assert target_registration_error(r.transform, truth, fixed)[0] < TRE_BOUND_MM
    # max_evaluations bounds the work; an Affine to start from
    short = reg.register(fixed, moving, "translation", initial=r.transform, max_evaluations=20, **kw)
    assert short.evaluations <= 21 and np.abs(short.parameters).max() < 0.5
    hist, counts = reg.joint_histogram(fixed, moving, r.transform, step=(4, 5, 5), labels=labels, moving_spacing=REG_SPACING, engine=emu_engine)
    assert counts == r.counts and hist.sum() == Q * counts["contributed"]
    assert abs(reg.mutual_information(hist) - r.value) < 1e-15
    for bad, text in ((dict(transform="elastic"), "transform"), (dict(metric="ssd"), "metric"), (dict(bins=1), "bins"), (dict(min_overlap=2), "min_overlap"),
                      (dict(initial="centre"), "initial"), (dict(initial="centroids"), "moving_labels"), (dict(mode="cubic"), "mode")):
        with pytest.raises(ValueError, match=text):
            reg.register(fixed, moving, **{**kw, **bad})
    with pytest.raises(ValueError, match="shape"):
        reg.register(fixed, moving, labels=labels[1:], **kw)
    with pytest.raises(ValueError, match="no voxel"):
        reg.register(fixed, moving, labels=np.zeros_like(labels), **kw)


def test_joint_histogram_host_form(emu_engine):
    from lungmask_amd import registration as reg
    from lungmask_amd import resample as rs
    from lungmask_amd import volume_io

    fixed = volume_io.Volume(volume((5, 7, 9), np.int16, 20), (0.7, 0.8, 2.5), (-12.0, 30.0, 4.5), [[0, 1, 0], [1, 0, 0], [0, 0, -1]])
    moving = volume_io.Volume(volume((4, 6, 11), np.float32, 21), (0.9, 0.6, 2.0), (-10.0, 31.0, 5.5))
    T = rs.Affine.rotation((0, 0, 1), 5.0).compose(rs.Affine.translation((1.0, -2.0, 0.5)))
    hist, counts = reg.joint_histogram(fixed, moving, T, bins=16, hu_range=(-1000, 199), step=(1, 2, 1), engine=emu_engine)
    A, b = rs.index_map(rs.Grid.of(moving), rs.Grid.of(fixed), T)
    want, wc = joint_hist_oracle(fixed.array, moving.array, A, b, 16, (-1000, 75), (-1000, 75), step=(1, 2, 1))
    assert np.array_equal(hist, want) and [counts[k] for k in ("sampled", "contributed", "outside", "nan")] == wc and wc[1] > 0


def test_apply_registered_on_the_emulator(emu_engine, monkeypatch):
    from lungmask_amd import morphology, registration as reg
    from tests.test_mask_wrappers_emu import Harness

    fixed, moving, truth = registration_case("rigid", RIGID_CASES["a"])
    labels = (lung_classes(fixed.array) == 1).astype(np.uint8)
    labels[:, :, 44:] *= 2  # two labels
    h = Harness(emu_engine, labels)
    try:
        kw = dict(levels_mm=(8.0, 4.0), max_evaluations=300)
        want = reg.register(fixed, moving, "rigid", labels=morphology.dilate(fixed.like(labels), 6.0, engine=emu_engine), moving_spacing=REG_SPACING,
                            engine=emu_engine, **kw)
        for host in (False, True):  # the one-GPU device branch, and the detour of the multi-GPU forms
            if host:
                monkeypatch.setattr(h.inf, "_shard", object())
            out, r = h.inf.apply_registered(fixed, moving, margin_mm=6.0, moving_spacing=REG_SPACING, **kw)
            assert np.array_equal(out, labels) and h.applied == (1 if host else 0)
            assert r.parameters == want.parameters and r.evaluations == want.evaluations and r.counts == want.counts and r.centre == want.centre
            assert np.array_equal(r.transform.matrix, want.transform.matrix)
            assert np.array_equal(r.image, want.resample(moving, moving_spacing=REG_SPACING, engine=emu_engine).array)
            assert r.image.dtype == np.float32 and r.image.shape == labels.shape
        assert 0 < r.counts["sampled"] < labels[::2, ::3, ::3].size
        with pytest.raises(TypeError, match="unexpected"):
            h.inf.apply_registered(fixed, moving, moving_spacing=REG_SPACING, labels=labels)
        with pytest.raises(ValueError, match="transform"):
            h.inf.apply_registered(fixed, moving, "elastic", moving_spacing=REG_SPACING)
    finally:
        monkeypatch.undo()
        h.inf.close()
    e = Harness(emu_engine, np.zeros_like(labels))
    try:
        with pytest.raises(ValueError, match="no voxel is labelled"):
            e.inf.apply_registered(fixed, moving, moving_spacing=REG_SPACING)
    finally:
        e.inf.close()


def test_compare_labels_with_a_transform(emu_engine):
    from lungmask_amd import metrics
    from lungmask_amd import resample as rs

    fixed, moving, truth = registration_case("rigid", RIGID_CASES["a"])
    a = fixed.like(lung_classes(fixed.array))
    b = rs.Grid.of(moving, REG_SPACING).like(lung_classes(moving))
    plain = metrics.compare_labels(a, b, resample_b=True, engine=emu_engine)
    placed = metrics.compare_labels(a, b, resample_b=True, transform=truth, engine=emu_engine)
    assert placed["labels"]["1"]["dice"] > plain["labels"]["1"]["dice"]  # (speckle of the noisy classes keeps it below 1)
    want = metrics.compare_labels(a, rs.resample_labels(b, rs.Grid.of(a), truth, engine=emu_engine), engine=emu_engine)
    assert placed == want
    with pytest.raises(ValueError, match="resample_b"):
        metrics.compare_labels(a, b, transform=truth, engine=emu_engine)
