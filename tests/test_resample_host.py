"""CPU suite: the host side of lungmask_amd.resample -- grids, affine transforms, the index map, compare_labels(resample_b=True),
LMInferer.apply_resampled and the command line -- with the device passes on the emulator."""
import json

import numpy as np
import pytest

from lungmask_amd import metrics
from lungmask_amd import resample as rs
from lungmask_amd import stats as lmstats
from lungmask_amd import volume_io
from tests.test_mask_wrappers_emu import DIRECTION, IMAGE, LABELS, ORIGIN, SHAPE, SPACING, Harness
from tests.test_resample_emu import restate
from tests.test_roi_emu import blobs, same_bits


def arr(x):
    return x.array if isinstance(x, volume_io.Volume) else x


def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.diag(r))  # (orthonormal; the determinant may be -1: a flipped image)


def random_grid(rng):
    shape = tuple(int(v) for v in rng.integers(3, 40, 3))
    return rs.Grid(shape, rng.uniform(0.4, 3.0, 3), rng.uniform(-200, 200, 3), random_rotation(rng))


def test_index_map_against_a_direct_evaluation():
    """A @ o + b against S_src^-1 D_src^T (T(D_out S_out o + O_out) - O_src) evaluated point by point in float64.  Both are a few
    products and sums of numbers up to ~500 mm divided by a spacing >= 0.4: index values up to ~2000, so 1e-9 of a voxel is a
    thousandfold the rounding error of either (2000 * 2^-52 * a dozen operations ~ 5e-12)."""
    rng = np.random.default_rng(1)
    for trial in range(20):
        src, out = random_grid(rng), random_grid(rng)
        T = rs.Affine(random_rotation(rng) * rng.uniform(0.8, 1.2), rng.uniform(-30, 30, 3)) if trial % 2 else None
        A, b = rs.index_map(src, out, T)
        assert A.dtype == np.float64 and A.shape == (3, 3) and b.shape == (3,)
        for _ in range(10):
            o = rng.uniform(-5, 45, 3)  # array axis order
            p = out.direction @ (np.asarray(out.spacing) * o[::-1]) + np.asarray(out.origin)
            if T is not None:
                p = T.matrix @ p + T.translation_vector
            want = ((src.direction.T @ (p - np.asarray(src.origin))) / np.asarray(src.spacing))[::-1]
            assert np.abs(A @ o + b - want).max() < 1e-9
    g = random_grid(rng)
    A, b = rs.index_map(g, g)
    assert np.abs(A - np.eye(3)).max() < 1e-12 and np.abs(b).max() < 1e-9
    with pytest.raises(ValueError, match="finite"):
        rs.index_map(g, g, rs.Affine(np.full((3, 3), np.inf)))


def test_affine_compose_and_inverse():
    rng = np.random.default_rng(2)
    pts = rng.uniform(-100, 100, (50, 3))
    for _ in range(10):
        a = rs.Affine.rotation(rng.normal(size=3), rng.uniform(-180, 180), rng.uniform(-50, 50, 3))
        b = rs.Affine.scale(rng.uniform(0.5, 2.0, 3), rng.uniform(-50, 50, 3)).compose(rs.Affine.translation(rng.uniform(-20, 20, 3)))
        np.testing.assert_allclose(a.compose(b).apply(pts), a.apply(b.apply(pts)), atol=1e-9)
        for t in (a, b, a.compose(b)):
            np.testing.assert_allclose(t.inverse().apply(t.apply(pts)), pts, atol=1e-9)
            np.testing.assert_allclose(t.compose(t.inverse()).matrix, np.eye(3), atol=1e-12)
    np.testing.assert_allclose(rs.Affine.identity().apply(pts), pts)
    c = np.array([3.0, -4.0, 5.0])
    rot = rs.Affine.rotation((0, 0, 1), 90.0, c)
    np.testing.assert_allclose(rot.apply(c), c, atol=1e-12)  # the centre stays
    np.testing.assert_allclose(rot.apply(c + [1.0, 0, 0]), c + [0, 1.0, 0], atol=1e-12)  # right-handed about +z
    np.testing.assert_allclose(rs.Affine.scale(2.0, c).apply(c + [1.0, 1.0, 1.0]), c + 2.0, atol=1e-12)
    with pytest.raises(ValueError, match="axis"):
        rs.Affine.rotation((0, 0, 0), 10)


def test_grid_forms_and_isotropic_extents():
    vol = volume_io.Volume(IMAGE, SPACING[::-1], ORIGIN, DIRECTION)
    g = rs.Grid.of(vol)
    assert g.shape == SHAPE and g.spacing == SPACING[::-1] and g.origin == ORIGIN and np.array_equal(g.direction, np.asarray(DIRECTION, float))
    np.testing.assert_allclose(g.index_to_physical((1, 2, 3)), vol.index_to_physical((3, 2, 1)))
    bare = rs.Grid.of(IMAGE, spacing=SPACING)
    assert bare.spacing == SPACING[::-1] and bare.origin == (0.0, 0.0, 0.0) and np.array_equal(bare.direction, np.eye(3))
    assert rs.Grid.of(IMAGE).spacing == (1.0, 1.0, 1.0) and rs.Grid.of(g) is g
    back = g.like(IMAGE)
    assert isinstance(back, volume_io.Volume) and back.spacing == vol.spacing and back.origin == vol.origin
    with pytest.raises(ValueError, match="shape"):
        g.like(IMAGE[1:])
    with pytest.raises(ValueError, match="spacing"):
        rs.Grid.of(vol, spacing=SPACING)
    # N_i = floor((e_i - 1) * s_i / t_i) + 1
    iso = rs.Grid.isotropic(vol, 0.5)
    assert iso.shape == (int(4 * 1.5 / 0.5) + 1, int(11 * 0.8 / 0.5) + 1, int(8 * 0.7 / 0.5) + 1) == (13, 18, 12)
    assert iso.spacing == (0.5, 0.5, 0.5) and iso.origin == ORIGIN and np.array_equal(iso.direction, g.direction)
    aniso = rs.Grid.isotropic(vol, (3.0, 0.8, 10.0))
    assert aniso.shape == (3, 12, 1) and aniso.spacing == (10.0, 0.8, 3.0)
    assert rs.Grid.isotropic(vol, SPACING).shape == SHAPE  # its own spacing: the same grid
    assert g.same_as(rs.Grid.isotropic(vol, SPACING)) and not g.same_as(iso)
    with pytest.raises(ValueError, match="spacing_mm"):
        rs.Grid.isotropic(vol, 0.0)


def test_resample_image_and_labels_return_forms(emu_engine):
    vol = volume_io.Volume(IMAGE, SPACING[::-1], ORIGIN, DIRECTION)
    iso = rs.Grid.isotropic(vol, 1.0)
    A, b = rs.index_map(rs.Grid.of(vol), iso)
    out = rs.resample_image(vol, iso, order=3, engine=emu_engine)
    assert isinstance(out, volume_io.Volume) and out.spacing == (1.0, 1.0, 1.0) and out.origin == ORIGIN
    assert same_bits(out.array, restate(IMAGE, A, b, iso.shape, "cubic"))
    lab = rs.resample_labels(vol.like(LABELS), iso, mode="linear", engine=emu_engine)
    assert same_bits(lab.array, restate(LABELS, A, b, iso.shape, "label_linear", fill=0))
    # a bare array without a spacing comes back bare, on unit voxels; with one as a Volume
    bare = rs.resample_image(IMAGE, rs.Grid((5, 6, 7), (1.0, 2.0, 1.0)), order=1, dtype=np.int16, engine=emu_engine)
    assert isinstance(bare, np.ndarray) and bare.dtype == np.int16 and np.array_equal(bare[:, :, :], IMAGE[:, ::2, :7])
    assert isinstance(rs.resample_labels(LABELS, rs.Grid(SHAPE, SPACING[::-1]), spacing=SPACING, engine=emu_engine), volume_io.Volume)
    # order 0 keeps the dtype; a translation moves the content against its direction (output -> source)
    moved = rs.resample_image(IMAGE, rs.Grid(SHAPE), transform=rs.Affine.translation((2.0, 0.0, 0.0)), order=0, fill=-7, engine=emu_engine)
    assert moved.dtype == IMAGE.dtype and np.array_equal(moved[:, :, :-2], IMAGE[:, :, 2:]) and np.all(moved[:, :, -2:] == -7)
    for bad in (dict(order=2), dict(order=0, dtype=np.float32), dict(order=1, dtype=np.float64)):
        with pytest.raises((ValueError, TypeError)):
            rs.resample_image(IMAGE, iso, engine=emu_engine, **bad)
    with pytest.raises(ValueError, match="mode"):
        rs.resample_labels(LABELS, iso, mode="cubic", engine=emu_engine)


def test_align_centroids(emu_engine):
    fixed = np.zeros((8, 20, 24), np.uint8)
    fixed[2:6, 4:10, 6:14] = 3
    moving = np.zeros((8, 20, 24), np.uint8)
    moving[3:7, 9:15, 4:12] = 1  # the same block moved by (+1, +5, -2) voxels
    sp = (2.0, 0.5, 1.5)
    t = rs.align_centroids(fixed, moving, spacing=sp, moving_spacing=sp, engine=emu_engine)
    np.testing.assert_allclose(t.translation_vector, [-2 * 1.5, 5 * 0.5, 1 * 2.0], atol=1e-12)  # (x, y, z) millimetres
    assert np.array_equal(t.matrix, np.eye(3))
    grid = rs.Grid(fixed.shape, sp[::-1])
    back = rs.resample_labels(moving, grid, transform=t, spacing=sp, engine=emu_engine)
    assert np.array_equal(back.array > 0, fixed > 0)
    with pytest.raises(ValueError, match="no voxel"):
        rs.align_centroids(fixed, np.zeros_like(moving), engine=emu_engine)


def test_compare_labels_resample_b(emu_engine):
    shape = (10, 24, 28)
    mask = blobs(shape, 3, n_labels=2)
    a = volume_io.Volume(mask, (0.8, 0.8, 2.0), (5.0, -3.0, 10.0))
    coarse_grid = rs.Grid.isotropic(a, (4.0, 1.6, 1.6))  # double spacing
    coarse = rs.resample_labels(a, coarse_grid, engine=emu_engine)
    assert coarse.array.shape == (5, 12, 14) and coarse.spacing == (1.6, 1.6, 4.0)
    round_trip = rs.resample_labels(coarse, rs.Grid.of(a), engine=emu_engine)
    want = metrics.compare_labels(a, round_trip, engine=emu_engine)
    assert metrics.compare_labels(a, coarse, resample_b=True, engine=emu_engine) == want
    assert 0.5 < want["labels"]["1"]["dice"] < 1.0
    # a b on a's grid is taken as it is, and the results without the flag are unchanged
    assert metrics.compare_labels(a, a.like(mask.copy()), resample_b=True, engine=emu_engine) == metrics.compare_labels(a, a, engine=emu_engine)
    with pytest.raises(ValueError, match="must have the same shape"):
        metrics.compare_labels(a, coarse, engine=emu_engine)
    same_shape = volume_io.Volume(mask, (1.6, 1.6, 4.0), a.origin)
    with pytest.raises(ValueError, match="disagree in geometry"):
        metrics.compare_labels(a, same_shape, engine=emu_engine)
    assert metrics.compare_labels(a, same_shape, resample_b=True, engine=emu_engine)["labels"]["1"]["dice"] < 1.0


@pytest.fixture(scope="module")
def lung(emu_engine):
    h = Harness(emu_engine, LABELS)
    yield h
    h.inf.close()


@pytest.mark.parametrize("form", ["numpy", "spacing", "volume"])
def test_apply_resampled_on_the_emulator(lung, emu_engine, form, monkeypatch):
    vol = volume_io.Volume(IMAGE, SPACING[::-1], ORIGIN, DIRECTION)
    image, kw = {"numpy": (IMAGE, {}), "spacing": (IMAGE, {"spacing": SPACING}), "volume": (vol, {})}[form]
    for host in (False, True):  # the one-GPU device branch, and the detour of the multi-GPU forms
        if host:
            monkeypatch.setattr(lung.inf, "_shard", object())
        lung.reset()
        labels, res = lung.inf.apply_resampled(image, spacing_out=0.75, order=3, **kw)
        assert np.array_equal(labels, LABELS) and lung.applied == (1 if host else 0)
        grid = rs.Grid.isotropic(image, 0.75, **kw)
        assert res.grid.shape == grid.shape == res.image.shape == res.labels.shape and res.grid.same_as(grid)
        assert same_bits(arr(rs.resample_image(image, grid, order=3, engine=emu_engine, **kw)), res.image)
        assert same_bits(arr(rs.resample_labels(vol.like(LABELS) if form == "volume" else LABELS, grid, mode="linear", engine=emu_engine, **kw)),
                         res.labels)
        assert res.meta()["shape"] == list(grid.shape) and res.meta()["order"] == 3 and json.dumps(res.meta())
        if form == "numpy":
            with pytest.raises(ValueError, match="no geometry"):
                res.as_volume()
        else:
            assert res.as_volume().spacing == (0.75, 0.75, 0.75) and res.labels_volume().array.dtype == np.uint8
    like = rs.Grid((4, 5, 6), (1.0, 1.5, 2.0), ORIGIN, DIRECTION)
    _, res = lung.inf.apply_resampled(vol, like=like, order=1, label_mode="nearest", dtype=np.float16, fill=0)
    assert res.image.dtype == np.float16 and res.image.shape == (4, 5, 6)
    assert same_bits(res.image, rs.resample_image(vol, like, order=1, dtype=np.float16, fill=0, engine=emu_engine).array)
    with pytest.raises(ValueError, match="label_mode"):
        lung.inf.apply_resampled(vol, label_mode="cubic")
    with pytest.raises(ValueError, match="order"):
        lung.inf.apply_resampled(vol, order=2)


def test_cli_flags_and_file_round_trip(lung, emu_engine, tmp_path, monkeypatch):
    import lungmask_amd.__main__ as cli

    vol = volume_io.Volume(IMAGE, SPACING[::-1], ORIGIN, DIRECTION)
    ip, out = tmp_path / "in.nii.gz", str(tmp_path / "o.npy")
    volume_io.write_nifti(str(ip), vol)
    a = cli.build_parser().parse_args([str(ip), out, "--resampled", "r.nii", "--resampled-labels", "l.mha", "--resample-spacing", "1", "2", "3",
                                       "--resample-order", "1", "--resample-label-mode", "nearest", "--compare-resample", "--roi", "x.nii"])
    assert (a.resampled, a.resampled_labels, a.resample_spacing, a.resample_order, a.resample_label_mode, a.compare_resample) == \
        ("r.nii", "l.mha", [1.0, 2.0, 3.0], 1, "nearest", True)
    d = cli.build_parser().parse_args([str(ip), out])
    assert d.resampled is None and d.resample_spacing is None and d.resample_order is None and not d.compare_resample
    for bad in (["--resample-spacing", "1"], ["--resample-order", "3"], ["--resample-like", str(ip)], ["--resample-label-mode", "linear"],
                ["--resampled", "r.txt"], ["--resampled", "r.nii", "--resample-spacing", "1", "2"], ["--resampled", "r.nii", "--resample-spacing", "0"],
                ["--resampled", "r.nii", "--resample-like", str(tmp_path / "none.nii")], ["--compare-resample"],
                ["--resampled", "r.nii", "--resample-like", str(ip), "--resample-spacing", "1"]):
        with pytest.raises(SystemExit):  # refused before anything is loaded
            cli.main([str(ip), out] + bad)
    with pytest.raises(SystemExit):
        cli.main([str(ip), out, "--resampled", "r.nii", "--resample-order", "2"])
    monkeypatch.setattr(cli, "LMInferer", lambda *a, **kw: lung.inf)
    monkeypatch.setattr(emu_engine, "n_classes", lambda slot: 3, raising=False)
    loaded = volume_io.load_input_image(str(ip))
    # the default grid: 1 mm isotropic, cubic image and label-linear labels, written with the grid's geometry
    rp, lp = tmp_path / "r.nii.gz", tmp_path / "l.mha"
    assert cli.main([str(ip), out, "--noprogress", "--resampled", str(rp), "--resampled-labels", str(lp)]) == 0
    grid = rs.Grid.isotropic(loaded, 1.0)
    for path, want in ((rp, rs.resample_image(loaded, grid, order=3, engine=emu_engine)),
                       (lp, rs.resample_labels(loaded.like(LABELS), grid, mode="linear", engine=emu_engine))):
        back = volume_io.load_input_image(str(path))
        assert same_bits(np.ascontiguousarray(back.array), want.array)
        np.testing.assert_allclose(back.spacing, grid.spacing, rtol=1e-6)
        np.testing.assert_allclose(back.origin, grid.origin, atol=1e-4)
        np.testing.assert_allclose(np.asarray(back.direction).reshape(3, 3), grid.direction, atol=1e-6)
    assert np.array_equal(np.load(out), LABELS)
    # onto another image's grid, beside --stats (from the labels it returned), three spacings in x y z order
    like = volume_io.Volume(np.zeros((4, 6, 5), np.int16), (1.5, 1.2, 2.0), ORIGIN, DIRECTION)
    volume_io.write_nifti(str(tmp_path / "like.nii"), like)
    assert cli.main([str(ip), out, "--noprogress", "--resampled", str(tmp_path / "r2.npy"), "--resample-like", str(tmp_path / "like.nii"),
                     "--resample-order", "1", "--stats", str(tmp_path / "s.json")]) == 0
    like_grid = rs.Grid.of(volume_io.load_input_image(str(tmp_path / "like.nii")))
    assert same_bits(np.load(tmp_path / "r2.npy"), rs.resample_image(loaded, like_grid, order=1, engine=emu_engine).array)
    assert json.load(open(tmp_path / "s.json"))["labels"]["1"]["voxels"] == int((LABELS == 1).sum())
    assert cli.main([str(ip), out, "--noprogress", "--resampled-labels", str(tmp_path / "l3.npy"), "--resample-spacing", "0.7", "0.8", "3.0",
                     "--resample-label-mode", "nearest"]) == 0
    assert np.load(tmp_path / "l3.npy").shape == rs.Grid.isotropic(loaded, (3.0, 0.8, 0.7)).shape
    # --compare-resample: a ground truth at another spacing
    coarse = rs.resample_labels(loaded.like(LABELS), rs.Grid.isotropic(loaded, (3.0, 1.6, 1.4)), engine=emu_engine)
    volume_io.write_nifti(str(tmp_path / "gt.nii.gz"), coarse)
    with pytest.raises(ValueError, match="same shape"):
        cli.main([str(ip), out, "--noprogress", "--compare-to", str(tmp_path / "gt.nii.gz"), "--metrics", str(tmp_path / "m.json")])
    assert cli.main([str(ip), out, "--noprogress", "--compare-to", str(tmp_path / "gt.nii.gz"), "--metrics", str(tmp_path / "m.json"),
                     "--compare-resample"]) == 0
    gt = volume_io.load_input_image(str(tmp_path / "gt.nii.gz"))
    assert json.load(open(tmp_path / "m.json")) == json.loads(json.dumps(
        metrics.compare_labels(loaded.like(LABELS), gt, n_labels=3, names=lmstats.label_names("R231", 3), resample_b=True, engine=emu_engine)))
