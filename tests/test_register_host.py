"""CPU suite: the host side of lungmask_amd.registration that needs no library -- the metric on hand-made histograms, the
parameterisation (`Affine.from_parameters`), the optimiser on analytic cost functions, the overlap rule and the command line's
refusals."""
import math

import numpy as np
import pytest

from lungmask_amd import registration as reg
from lungmask_amd import resample as rs


# ------------------------------------------------------------------------------------------------ the metric
def test_mutual_information_of_independent_axes():
    hist = np.outer([1, 2, 3, 4], [5, 1, 2]) * 65536
    assert abs(reg.mutual_information(hist, normalized=False)) < 1e-12
    assert abs(reg.mutual_information(hist) - 1.0) < 1e-12


def test_mutual_information_of_a_diagonal():
    hist = np.diag([3, 1, 4, 1, 5]).astype(np.int64) * 65536
    p = np.array([3, 1, 4, 1, 5]) / 14.0
    entropy = -float(np.sum(p * np.log(p)))
    assert abs(reg.mutual_information(hist) - 2.0) < 1e-12
    assert abs(reg.mutual_information(hist, normalized=False) - entropy) < 1e-12
    shuffled = hist[:, [2, 0, 4, 1, 3]]  # any one-to-one relation of the bins
    assert abs(reg.mutual_information(shuffled) - 2.0) < 1e-12


def test_mutual_information_without_information():
    assert reg.mutual_information(np.zeros((4, 4), np.int64)) is None
    single = np.zeros((4, 4), np.int64)
    single[2, 1] = 7 * 65536
    assert reg.mutual_information(single) is None and reg.mutual_information(single, normalized=False) is None


def test_mutual_information_by_hand():
    hist = np.array([[2, 1], [1, 4]])
    p = hist / 8.0
    h = lambda q: -sum(v * math.log(v) for v in np.ravel(q) if v > 0)  # noqa: E731
    hf, hm, hj = h(p.sum(1)), h(p.sum(0)), h(p)
    assert abs(reg.mutual_information(hist) - (hf + hm) / hj) < 1e-15
    assert abs(reg.mutual_information(hist, normalized=False) - (hf + hm - hj)) < 1e-15


# ------------------------------------------------------------------------------------------------ the parameterisation
CENTRE = np.array([12.0, -30.0, 45.5])
PTS = np.random.default_rng(3).uniform(-150, 150, (40, 3))


def rigid_reference(p):
    out = rs.Affine.identity()
    for axis, angle in zip(np.eye(3), p[:3]):
        out = rs.Affine.rotation(axis, angle, CENTRE).compose(out)
    return rs.Affine.translation(p[3:6]).compose(out)


def test_identity_parameters_give_the_identity():
    for kind, n in reg.TRANSFORMS.items():
        t = rs.Affine.from_parameters(kind, np.zeros(n), CENTRE)
        assert np.array_equal(t.matrix, np.eye(3)) and np.abs(t.translation_vector).max() < 1e-12


def test_from_parameters_against_the_named_constructors():
    t = rs.Affine.from_parameters("translation", (1.5, -2.0, 3.25))
    np.testing.assert_allclose(t.apply(PTS), rs.Affine.translation((1.5, -2.0, 3.25)).apply(PTS), atol=1e-12)
    rigid = np.array([3.0, -2.0, 4.0, 3.0, -4.5, 6.0])
    np.testing.assert_allclose(rs.Affine.from_parameters("rigid", rigid, CENTRE).apply(PTS), rigid_reference(rigid).apply(PTS), atol=1e-10)
    for axis in range(3):  # one angle alone: the rotation about that LPS axis through the centre, which stays
        p = np.zeros(6)
        p[axis] = 17.0
        t = rs.Affine.from_parameters("rigid", p, CENTRE)
        np.testing.assert_allclose(t.apply(PTS), rs.Affine.rotation(np.eye(3)[axis], 17.0, CENTRE).apply(PTS), atol=1e-10)
        np.testing.assert_allclose(t.apply(CENTRE), CENTRE, atol=1e-10)
    sim = np.append(rigid, 5.0)  # 5 % of log-scale
    want = rigid_reference(rigid).compose(rs.Affine.scale(math.exp(0.05), CENTRE))
    np.testing.assert_allclose(rs.Affine.from_parameters("similarity", sim, CENTRE).apply(PTS), want.apply(PTS), atol=1e-10)
    aff = np.concatenate([rigid, [3.0, -2.0, 1.0], [4.0, -1.0, 2.5]])
    shear = rs.Affine(np.array([[1.0, 0.04, -0.01], [0.0, 1.0, 0.025], [0.0, 0.0, 1.0]]))
    shear = rs.Affine.translation(CENTRE).compose(shear).compose(rs.Affine.translation(-CENTRE))  # about the centre
    want = rigid_reference(rigid).compose(shear).compose(rs.Affine.scale(np.exp(np.array([3.0, -2.0, 1.0]) / 100.0), CENTRE))
    got = rs.Affine.from_parameters("affine", aff, CENTRE)
    np.testing.assert_allclose(got.apply(PTS), want.apply(PTS), atol=1e-10)
    assert abs(np.linalg.det(got.matrix) - math.exp(0.02)) < 1e-12  # rotations and shears keep the volume
    with pytest.raises(ValueError, match="one of"):
        rs.Affine.from_parameters("projective", np.zeros(15))
    with pytest.raises(ValueError, match="takes 6 parameters"):
        rs.Affine.from_parameters("rigid", np.zeros(7))


# ------------------------------------------------------------------------------------------------ the optimiser
@pytest.mark.parametrize("n", [6, 12])
def test_optimiser_on_a_shifted_anisotropic_quadratic(n):
    rng = np.random.default_rng(n)
    q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    H = q @ np.diag(np.geomspace(0.05, 5.0, n)) @ q.T  # condition 100, axes not the parameters'
    target = rng.uniform(-6, 6, n)
    calls = []

    def cost(x):
        calls.append(np.array(x))
        d = x - target
        return float(d @ H @ d) - 1.5

    x, fx, evaluations = reg.minimize(cost, np.zeros(n), np.full(n, 2.0), tolerance=0.01, max_evaluations=4000)
    assert evaluations == len(calls) <= 4000
    assert np.abs(x - target).max() < 0.01  # the stopping tolerance, in parameter units
    assert fx == cost(x) and fx < -1.5 + 1e-4
    again = reg.minimize(cost, np.zeros(n), np.full(n, 2.0), tolerance=0.01, max_evaluations=4000)
    assert np.array_equal(again[0], x) and again[2] == evaluations  # deterministic


def test_optimiser_stops_at_max_evaluations_with_the_best_point():
    target = np.array([3.0, -2.0, 5.0, 1.0])
    seen = []

    def cost(x):
        seen.append((float(np.sum((x - target) ** 2)), np.array(x)))
        return seen[-1][0]

    x, fx, evaluations = reg.minimize(cost, np.zeros(4), np.ones(4), max_evaluations=25)
    assert evaluations == 25 == len(seen)
    best = min(seen, key=lambda s: s[0])
    assert fx == best[0] and np.array_equal(x, best[1])
    with pytest.raises(ValueError, match="positive step"):
        reg.minimize(cost, np.zeros(4), np.zeros(4))


# ------------------------------------------------------------------------------------------------ the overlap rule
def test_min_overlap_rejects_an_evaluation():
    hist = np.diag([3, 1, 4]).astype(np.int64) * 65536
    ok = {"sampled": 16, "contributed": 8, "outside": 8, "nan": 0}
    low = {"sampled": 16, "contributed": 7, "outside": 9, "nan": 0}
    none = {"sampled": 16, "contributed": 0, "outside": 16, "nan": 0}
    assert reg.evaluation_cost(hist, ok, "nmi", 0.5) == -reg.mutual_information(hist)
    assert reg.evaluation_cost(hist, ok, "mi", 0.5) == -reg.mutual_information(hist, normalized=False)
    worst_valid = 0.0  # minus a metric that is never negative
    assert reg.evaluation_cost(hist, low, "nmi", 0.5) > worst_valid
    assert reg.evaluation_cost(hist, none, "nmi", 0.5) > reg.evaluation_cost(hist, low, "nmi", 0.5)  # falls towards more overlap
    assert reg.evaluation_cost(hist, low, "nmi", 0.25) == -reg.mutual_information(hist)
    assert reg.evaluation_cost(np.zeros((3, 3), np.int64), {"sampled": 0, "contributed": 0, "outside": 0, "nan": 0}) > worst_valid
    single = np.zeros((3, 3), np.int64)
    single[0, 0] = 65536 * 16
    assert reg.evaluation_cost(single, {"sampled": 16, "contributed": 16, "outside": 0, "nan": 0}) > worst_valid  # no metric: not valid


def test_levels_and_bins():
    assert reg._level_step(8.0, (2.0, 1.5, 1.5)) == (4, 5, 5)
    assert reg._level_step(4.0, (2.0, 1.5, 1.5)) == (2, 3, 3)
    assert reg._level_step(2.0, (2.0, 1.5, 1.5)) == (1, 1, 1)
    assert reg._level_step(0.5, (2.0, 1.5, 1.5)) == (1, 1, 1)
    assert reg._bins_of((-1024, 1023), 32) == (-1024, 64) and reg._bins_of((-1000, 199), 32) == (-1000, 38) and reg._bins_of((0, 7), 8) == (0, 1)
    for bad in (1, 65, 2.5):
        with pytest.raises(ValueError, match="bins"):
            reg._bins_of((-1024, 1023), bad)
    labels = np.zeros((4, 5, 6), np.uint8)
    labels[1, 2, 3] = 1
    labels[3, 4, 5] = 2
    assert reg.label_centroid_index(labels) == [2.0, 3.0, 4.0] and reg.label_centroid_index(labels, keep=(2,)) == [3.0, 4.0, 5.0]
    assert reg.label_centroid_index(labels, keep=(7,)) is None


# ------------------------------------------------------------------------------------------------ the command line
def test_cli_refusals(tmp_path, monkeypatch):
    import lungmask_amd.__main__ as cli

    ip, out = str(tmp_path / "in.npy"), str(tmp_path / "o.npy")
    moving = tmp_path / "moving.npy"
    for f in (ip, moving):
        np.save(f, np.zeros((2, 3, 4), np.int16))
    from lungmask_amd import volume_io

    monkeypatch.setattr(volume_io, "load_input_image", lambda *a, **kw: pytest.fail("a bad combination is refused before anything is loaded"))
    a = cli.build_parser().parse_args([ip, out, "--register-moving", "m.nii", "--registered", "r.nii", "--registration", "t.json",
                                       "--register-transform", "affine"])
    assert (a.register_moving, a.registered, a.registration, a.register_transform) == ("m.nii", "r.nii", "t.json", "affine")
    d = cli.build_parser().parse_args([ip, out])
    assert d.register_moving is None and d.registered is None and d.registration is None and d.register_transform is None
    m = ["--register-moving", str(moving)]
    for bad in (["--registered", "r.nii"], ["--registration", "t.json"], ["--register-transform", "rigid"], m,
                m + ["--registered", "r.txt"], m + ["--registration", "t.txt"],
                ["--register-moving", str(tmp_path / "none.nii"), "--registration", "t.json"]):
        with pytest.raises(SystemExit):
            cli.main([ip, out] + bad)
    with pytest.raises(SystemExit):
        cli.main([ip, out] + m + ["--registration", "t.json", "--register-transform", "projective"])
