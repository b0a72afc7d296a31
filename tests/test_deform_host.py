"""The host side of lungmask_amd.deformable, without a library: the displacement field's files and geometry, the scales the device
gets, the stopping rule, the total Jacobian, and argument refusals."""
import json

import numpy as np
import pytest

from lungmask_amd import deformable as dfm
from lungmask_amd import resample as rs

GRID = rs.Grid((3, 4, 5), (0.7, 0.8, 2.5), (-12.0, 30.0, 4.5), [[0, 1, 0], [1, 0, 0], [0, 0, -1]])  # permuted and mirrored
AFFINE = rs.Affine.rotation((0, 0, 1), 5.0).compose(rs.Affine.translation((1.0, -2.0, 0.5)))


def a_field(affine=AFFINE):
    arr = np.random.default_rng(1).normal(0.0, 3.0, (3,) + GRID.shape).astype(np.float32)
    arr[0, 0, 0, 0], arr[1, 1, 1, 1] = np.float32(-0.0), np.float32(1e-40)  # a signed zero and a subnormal survive too
    return dfm.DisplacementField(arr, GRID, affine)


def test_npz_round_trip_is_exact(tmp_path):
    f = a_field()
    path = str(tmp_path / "field.npz")
    f.save(path)
    g = dfm.load(path)
    assert g.array.dtype == np.float32 and np.array_equal(g.array.view(np.uint32), f.array.view(np.uint32))
    assert g.grid.shape == GRID.shape and g.grid.spacing == GRID.spacing and g.grid.origin == GRID.origin
    assert np.array_equal(g.grid.direction, GRID.direction)
    assert np.array_equal(g.affine.matrix, AFFINE.matrix) and np.array_equal(g.affine.translation_vector, AFFINE.translation_vector)
    assert json.loads(json.dumps(g.meta())) == f.meta() and f.meta()["shape"] == [3, 4, 5] and len(f.meta()["matrix"]) == 9


@pytest.mark.parametrize("name", ["field.nii", "field.nii.gz"])
def test_nifti_round_trip(tmp_path, name):
    from lungmask_amd import volume_io

    f = a_field()
    path = str(tmp_path / name)
    f.save(path)
    g = dfm.DisplacementField.load(path)
    assert np.array_equal(g.array.view(np.uint32), f.array.view(np.uint32))  # the components, bit for bit
    assert g.grid.same_as(GRID) and np.array_equal(g.affine.matrix, np.eye(3))  # the geometry as NIfTI keeps it; no affine
    vol, stack = volume_io.read_nifti_channels(path)
    assert stack.shape == (3,) + GRID.shape and vol.array.shape == GRID.shape  # 4-D, the component as the 4th NIfTI axis
    with pytest.raises(ValueError, match="3-D image"):
        volume_io.read_nifti(path)
    with pytest.raises(ValueError, match="npz"):
        f.save(str(tmp_path / "field.mha"))


def test_lps_vectors_under_a_permuted_and_mirrored_direction():
    f = a_field()
    v = f.lps()
    assert v.shape == GRID.shape + (3,) and v.dtype == np.float64
    z, y, x = (f.array[i].astype(np.float64) for i in range(3))
    # direction [[0, 1, 0], [1, 0, 0], [0, 0, -1]]: L <- the grid's y axis, P <- its x axis, S <- its z axis mirrored
    assert np.array_equal(v[..., 0], y) and np.array_equal(v[..., 1], x) and np.array_equal(v[..., 2], -z)
    # the displacement of a voxel equals the difference of the physical points of the displaced and the plain index
    o = np.array([1, 2, 3])
    d = f.array[:, 1, 2, 3].astype(np.float64) / np.asarray(dfm.spacing_zyx(GRID))
    np.testing.assert_allclose(GRID.index_to_physical(o + d) - GRID.index_to_physical(o), v[1, 2, 3], atol=1e-12)


def test_scales_from_a_spacing():
    fs, gs = dfm.field_scales((2.5, 0.8, 0.7))
    assert fs == [1.0 / 2.5, 1.0 / 0.8, 1.0 / 0.7] and gs == [v / 2.0 for v in fs]
    assert dfm.field_scales(None) == ([1.0, 1.0, 1.0], [0.5, 0.5, 0.5])
    assert dfm.spacing_zyx(GRID) == (2.5, 0.8, 0.7)
    with pytest.raises(ValueError, match="spacing"):
        dfm.field_scales((1.0, -1.0, 1.0))
    # a longest step of max_step: k = 2 * max_step, inv_k2 = 1 / k^2; the default is half the level's smallest spacing
    assert dfm.level_inv_k2(GRID, 0.25) == 4.0 and dfm.level_inv_k2(GRID, None) == 1.0 / (4.0 * 0.35 * 0.35)
    taps = dfm.field_taps(GRID, None)
    assert [t.size for t in taps] == [9, 9, 9] and dfm.field_taps(GRID, 0.0)[0].tolist() == [1.0]
    assert [t.size for t in dfm.field_taps(GRID, (2.5, 1.6, 0.7))] == [9, 17, 9]


def test_level_grids_cover_the_same_box():
    grid = rs.Grid((28, 44, 45), (0.7, 0.8, 2.5), (1.0, 2.0, 3.0))
    for mm in (8.0, 4.0, 2.0, 0.1):
        lv = dfm.level_grid(grid, mm)
        for e, s, n, t in zip(grid.shape, dfm.spacing_zyx(grid), lv.shape, dfm.spacing_zyx(lv)):
            assert 2 <= n <= e and abs((n - 1) * t - (e - 1) * s) < 1e-9 and t >= s * (1 - 1e-12)
        assert lv.origin == grid.origin
    assert dfm.level_grid(grid, 0.1).shape == grid.shape  # never finer than the native grid
    assert dfm.level_grid(grid, 8.0).shape == (9, 5, 5)  # round(27 * 2.5 / 8), round(43 * 0.8 / 8), round(44 * 0.7 / 8), each + 1
    assert dfm.level_grid(rs.Grid((1, 1, 7)), 2.0).shape == (1, 1, 4)
    assert [t.tolist() for t in dfm.antialias_taps(grid, grid)] == [[1.0]] * 3


def test_stopping_rule_on_hand_made_metric_lists():
    n = 1000
    falling = [(100 - k, n) for k in range(10)]
    assert dfm.run_stop_rule(falling, 3) == (10, "iterations")
    assert dfm.run_stop_rule(falling, 3, iterations=4) == (4, "iterations")
    # three iterations in a row that are not below the lowest value so far: equal does not count as fallen
    assert dfm.run_stop_rule([(100, n), (90, n), (90, n), (95, n), (91, n), (10, n)], 3) == (5, "patience")
    assert dfm.run_stop_rule([(100, n), (90, n), (90, n), (95, n), (89, n), (95, n), (95, n)], 3) == (7, "iterations")
    # ratios, not sums: 90 / 900 is not below 100 / 1000, 89 / 900 is; exact for integers beyond float64
    assert dfm.run_stop_rule([(100, 1000), (90, 900), (90, 900)], 2) == (3, "patience")
    assert dfm.run_stop_rule([(100, 1000), (89, 900), (90, 900)], 2) == (3, "iterations")
    big = 2 ** 70
    assert dfm.run_stop_rule([(big + 1, 7), (big, 7), (big, 7)], 1) == (3, "patience")
    assert dfm.run_stop_rule([(big + 1, 7), (big, 7), (big - 1, 7)], 1) == (3, "iterations")
    assert dfm.run_stop_rule([(5, 10), (0, 0), (1, 10)], 4) == (2, "no overlap")
    with pytest.raises(ValueError, match="patience"):
        dfm.StopRule(0)


def test_total_jacobian_against_numpy(monkeypatch):
    M = np.array([[1.1, 0.1, 0.0], [0.0, 0.9, 0.2], [0.05, 0.0, 1.2]])
    f = dfm.DisplacementField.zeros(GRID, rs.Affine(M, (1.0, 2.0, 3.0)))
    det = np.random.default_rng(2).uniform(0.5, 1.5, GRID.shape).astype(np.float32)

    class Eng:
        def jacobian(self, field, spacing):
            assert spacing == dfm.spacing_zyx(GRID) and field is f.array
            return det.copy(), 2, 1

    plain, info = dfm.jacobian_determinant(f, engine=Eng())
    assert np.array_equal(plain, det) and info == {"folded": 2, "nonfinite": 1, "min": float(det.min()), "max": float(det.max())}
    total, info = dfm.jacobian_determinant(f, total=True, engine=Eng())
    assert np.array_equal(total, (det.astype(np.float64) * np.linalg.det(M)).astype(np.float32)) and info["folded"] == 2


def test_argument_refusals():
    with pytest.raises(ValueError, match="shape"):
        dfm.DisplacementField(np.zeros((3, 3, 4, 6), np.float32), GRID)
    with pytest.raises(ValueError, match="shape"):
        dfm.DisplacementField(np.zeros(GRID.shape, np.float32), GRID)
    with pytest.raises(TypeError, match="Affine"):
        dfm.DisplacementField(np.zeros((3,) + GRID.shape, np.float32), GRID, np.eye(3))
    vol = np.zeros((3, 4, 5), np.int16)
    with pytest.raises(ValueError, match="same length"):
        dfm.register_deformable(vol, vol, levels_mm=(4.0, 2.0), iterations=(10,))
    with pytest.raises(ValueError, match="at least one"):
        dfm.register_deformable(vol, vol, levels_mm=(), iterations=())
    with pytest.raises(ValueError, match="patience"):
        dfm.register_deformable(vol, vol, patience=0)
    with pytest.raises(ValueError, match="den_min"):
        dfm.register_deformable(vol, vol, den_min=-1.0)
    with pytest.raises(TypeError, match="initial"):
        dfm.register_deformable(vol, vol, initial=np.eye(4))
    with pytest.raises(TypeError, match="DisplacementField"):
        dfm.warp_labels(np.zeros((3, 4, 5), np.uint8), None)
    with pytest.raises(ValueError, match="mode"):
        dfm.warp_labels(np.zeros((3, 4, 5), np.uint8), a_field(), mode="cubic")
    with pytest.raises(ValueError, match="order"):
        dfm.warp_image(vol, a_field(), order=2)


def test_cli_refusals(tmp_path, monkeypatch):
    import lungmask_amd.__main__ as cli
    from lungmask_amd import volume_io

    ip, out = str(tmp_path / "in.npy"), str(tmp_path / "o.npy")
    moving = tmp_path / "moving.npy"
    for f in (ip, moving):
        np.save(f, np.zeros((2, 3, 4), np.int16))
    monkeypatch.setattr(volume_io, "load_input_image", lambda *a, **kw: pytest.fail("a bad combination is refused before anything is loaded"))
    a = cli.build_parser().parse_args([ip, out, "--register-moving", "m.nii", "--register-deformable", "--deformation", "f.npz", "--jacobian", "j.npy"])
    assert (a.register_deformable, a.deformation, a.jacobian) == (True, "f.npz", "j.npy")
    d = cli.build_parser().parse_args([ip, out])
    assert d.register_deformable is False and d.deformation is None and d.jacobian is None
    m = ["--register-moving", str(moving)]
    for bad in (["--register-deformable"], ["--deformation", "f.npz"], ["--jacobian", "j.npy"], m + ["--deformation", "f.npz"], m + ["--jacobian", "j.npy"],
                m + ["--register-deformable"], m + ["--register-deformable", "--deformation", "f.mha"],
                m + ["--register-deformable", "--jacobian", "j.txt"]):
        with pytest.raises(SystemExit):
            cli.main([ip, out] + bad)
