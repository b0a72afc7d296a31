"""The host side of the fields-as-operands part of lungmask_amd.deformable, without a library: the refusals of `invert`, `compose` and
`inverse_consistency`, the geometry they hand to the device, the keys of `info` and `meta()`, an inverse field's file, and the command
line's refusals for --inverse-deformation and --labels-on-moving."""
import json
import math

import numpy as np
import pytest

from lungmask_amd import _native as nat
from lungmask_amd import deformable as dfm
from lungmask_amd import resample as rs

GRID = rs.Grid((3, 4, 5), (0.7, 0.8, 2.5), (-12.0, 30.0, 4.5), [[0, 1, 0], [1, 0, 0], [0, 0, -1]])  # permuted and mirrored
OTHER = rs.Grid((4, 3, 6), (0.9, 0.6, 2.0), (-10.0, 31.0, 5.5), [[0, -1, 0], [1, 0, 0], [0, 0, 1]])
AFFINE = rs.Affine.rotation((0, 0, 1), 5.0).compose(rs.Affine.translation((1.0, -2.0, 0.5)))


def a_field(affine=None, grid=GRID):
    return dfm.DisplacementField(np.random.default_rng(1).normal(0.0, 1.0, (3,) + grid.shape).astype(np.float32), grid, affine)


def test_argument_checking():
    f = a_field()
    for call in (lambda: dfm.invert(f.array), lambda: dfm.compose(f, f.array), lambda: dfm.compose(None, f),
                 lambda: dfm.inverse_consistency(f, None), lambda: dfm.inverse_consistency(f.array, f)):
        with pytest.raises(TypeError, match="DisplacementField"):
            call()
    with pytest.raises(ValueError, match="2\\^-11"):  # below the resolution of the device's count
        dfm.invert(f, tolerance_mm=0.0005)
    for bad in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="tolerance_mm"):
            dfm.invert(f, tolerance_mm=bad)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="iterations"):
            dfm.invert(f, iterations=bad)
    with pytest.raises(ValueError, match="pass the moving grid"):
        dfm.invert(a_field(AFFINE))
    with pytest.raises(ValueError, match="singular"):
        dfm.compose_rotation(GRID, rs.Affine(np.zeros((3, 3))), OTHER)
    # the threshold: the largest step is at most the tolerance, in the count's integers
    assert dfm.check_inversion(30, 0.01) == (30, int(math.floor(0.01 * 0.01 * 2 ** 22 + 0.5))) and dfm.check_inversion(1, 0.001)[1] == 4
    assert dfm.check_inversion(5, 0.01, AFFINE, OTHER)[0] == 5 and nat.FIELD_Q == 2 ** 22 and dfm.FIELD_RESOLUTION_MM == 2.0 ** -11
    assert nat.FIELD_COUNTS == ("outside", "nan", "sum_q", "max_q")


def test_compose_rotation_is_the_pull_back_of_a_vector():
    """R takes a vector in the second grid's array axes to the first grid's, through the inverse of the first affine's matrix."""
    M = AFFINE.matrix @ np.diag([1.1, 0.9, 1.05])
    R = dfm.compose_rotation(GRID, rs.Affine(M, (1.0, 2.0, 3.0)), OTHER)
    v = np.array([0.3, -1.2, 2.0])  # (z, y, x) on OTHER
    lps = np.linalg.inv(M) @ (OTHER.direction @ v[::-1])
    assert np.allclose(R @ v, (GRID.direction.T @ lps)[::-1], atol=1e-14)
    assert np.array_equal(dfm.compose_rotation(rs.Grid((2, 2, 2)), rs.Affine(), rs.Grid((3, 3, 3))), np.eye(3))  # nothing to rotate


def test_figures_from_the_counts():
    fig = dfm._field_figures([7, 2, 3 * 2 ** 22, 2 ** 22], 5)
    assert fig == {"max_mm": 1.0, "rms_mm": 1.0, "outside": 7, "nonfinite": 2}
    assert dfm._field_figures([0, 5, 0, 0], 5)["rms_mm"] is None and dfm._q_mm(2 ** 30) == 16.0 and dfm._q_mm(1) == 2.0 ** -11


def test_meta_gains_the_inverse_only_once_it_is_known():
    reg = dfm.DeformableRegistration(a_field(AFFINE), [], [16, 1], [0, 1], {"folded": 0, "nonfinite": 0})
    before = reg.meta()
    assert "inverse" not in before and reg.moving_grid is None and reg.inverse_field is None and reg.labels_on_moving is None
    with pytest.raises(ValueError, match="moving grid"):
        reg.inverse()
    with pytest.raises(ValueError, match="kind"):
        reg.resample_to_moving(np.zeros(GRID.shape, np.uint8), kind="mask")
    info = {"iterations": 3, "converged": True, "residual_max_mm": 0.004, "residual_rms_mm": 0.001, "residuals": [1.0, 0.1, 0.004], "outside": 2,
            "nonfinite": 0}
    reg.inverse_field, reg.inverse_info, reg.moving_grid, reg._inverse_key = a_field(AFFINE.inverse(), OTHER), info, OTHER, (30, 0.01)
    after = reg.meta()
    assert after["inverse"] == info and {k: v for k, v in after.items() if k != "inverse"} == before
    assert json.loads(json.dumps(after)) == after
    assert reg.inverse() == (reg.inverse_field, info)  # kept: no device call for the same arguments


def test_an_inverse_field_survives_npz(tmp_path):
    inv = a_field(AFFINE.inverse(), OTHER)
    path = str(tmp_path / "inverse.npz")
    inv.save(path)
    back = dfm.load(path)
    assert np.array_equal(back.array.view(np.uint32), inv.array.view(np.uint32)) and back.grid.shape == OTHER.shape
    assert back.grid.spacing == OTHER.spacing and back.grid.origin == OTHER.origin and np.array_equal(back.grid.direction, OTHER.direction)
    assert np.array_equal(back.affine.matrix, AFFINE.inverse().matrix)
    assert np.array_equal(back.affine.translation_vector, AFFINE.inverse().translation_vector)
    assert np.allclose(back.affine.compose(AFFINE).matrix, np.eye(3), atol=1e-15)


def test_cli_refusals(tmp_path, monkeypatch):
    import lungmask_amd.__main__ as cli
    from lungmask_amd import volume_io

    ip, out = str(tmp_path / "in.npy"), str(tmp_path / "o.npy")
    moving = tmp_path / "moving.npy"
    for f in (ip, moving):
        np.save(f, np.zeros((2, 3, 4), np.int16))
    monkeypatch.setattr(volume_io, "load_input_image", lambda *a, **kw: pytest.fail("a bad combination is refused before anything is loaded"))
    a = cli.build_parser().parse_args([ip, out, "--register-moving", "m.nii", "--register-deformable", "--inverse-deformation", "i.npz",
                                       "--labels-on-moving", "l.nii.gz"])
    assert (a.inverse_deformation, a.labels_on_moving) == ("i.npz", "l.nii.gz")
    d = cli.build_parser().parse_args([ip, out])
    assert d.inverse_deformation is None and d.labels_on_moving is None
    m = ["--register-moving", str(moving)]
    for bad in (["--inverse-deformation", "i.npz"], ["--labels-on-moving", "l.npy"], m + ["--inverse-deformation", "i.npz"],
                m + ["--labels-on-moving", "l.npy"], m + ["--registered", "r.npy", "--labels-on-moving", "l.npy"],
                ["--register-deformable", "--inverse-deformation", "i.npz"], m + ["--register-deformable", "--inverse-deformation", "i.mha"],
                m + ["--register-deformable", "--labels-on-moving", "l.txt"]):
        with pytest.raises(SystemExit):
            cli.main([ip, out] + bad)
