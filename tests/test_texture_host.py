"""The host side of lungmask_amd.texture: the IBSI GLCM / GLRLM features from given matrices (closed-form cases, a deliberately naive
second evaluation of every formula), the aggregation over directions, and texture_features' dict (JSON, the lung entry, input
validation) on the emulation engine."""
import json
import math

import numpy as np
import pytest

from lungmask_amd import texture as tx
from lungmask_amd import volume_io
from tests.test_texture_emu import oracle_texture, random_case


def test_constant_region():
    length, a = 7, 5
    lab = np.ones((2, 3, length), np.uint8)
    vol = np.full(lab.shape, -1000 + 25 * a + 3, np.int16)
    m = oracle_texture(lab, vol, 2)
    g = tx.glcm_features(m["glcm"][1][0])
    assert m["glcm"][1][0].sum() == 6 * (length - 1)
    assert g["joint_maximum"] == 1.0 and g["joint_entropy"] == 0.0 and g["contrast"] == 0.0 and g["correlation"] is None
    assert g["information_correlation_1"] is None and g["joint_average"] == a + 1
    r = tx.glrlm_features(m["glrlm"][1][0])
    assert r["run_percentage"] == pytest.approx(1 / length, rel=1e-15) and r["long_run_emphasis"] == float(length ** 2)
    assert r["run_entropy"] == 0.0 and r["grey_level_variance"] == 0.0


def test_alternating_levels():
    a, b = 3, 9
    lab = np.ones((2, 3, 10), np.uint8)
    vol = np.empty(lab.shape, np.int16)
    vol[..., 0::2], vol[..., 1::2] = -1000 + 25 * a, -1000 + 25 * b
    m = oracle_texture(lab, vol, 2)
    g = tx.glcm_features(m["glcm"][1][0])
    assert g["contrast"] == float((a - b) ** 2) and g["correlation"] == pytest.approx(-1.0, abs=1e-15)
    assert g["dissimilarity"] == abs(a - b) and g["joint_maximum"] == 0.5
    r = tx.glrlm_features(m["glrlm"][1][0])
    assert m["glrlm"][1][0].shape[1] >= 1 and m["glrlm"][1][0][:, 1:].sum() == 0 and m["glrlm"][1][0].sum() == 60
    assert r["short_run_emphasis"] == 1.0 and r["run_percentage"] == 1.0 and r["run_length_variance"] == 0.0


def naive_glcm(counts):
    ng = len(counts)
    tot = sum(counts[i][j] + counts[j][i] for i in range(ng) for j in range(ng))
    p = [[(counts[i][j] + counts[j][i]) / tot for j in range(ng)] for i in range(ng)]
    lg = lambda v: math.log2(v) if v > 0 else 0.0
    px = [sum(p[i][j] for j in range(ng)) for i in range(ng)]
    mu = sum((i + 1) * px[i] for i in range(ng))
    var = sum((i + 1 - mu) ** 2 * px[i] for i in range(ng))
    pd = [sum(p[i][j] for i in range(ng) for j in range(ng) if abs(i - j) == k) for k in range(ng)]
    ps = {k: sum(p[i][j] for i in range(ng) for j in range(ng) if i + j + 2 == k) for k in range(2, 2 * ng + 1)}
    mud = sum(k * pd[k] for k in range(ng))
    mus = sum(k * v for k, v in ps.items())
    f = dict.fromkeys(tx.GLCM_FEATURES, 0.0)
    hxy1 = hxy2 = 0.0
    for i in range(ng):
        for j in range(ng):
            v, I, J = p[i][j], i + 1, j + 1
            f["joint_maximum"] = max(f["joint_maximum"], v)
            f["joint_average"] += I * v
            f["joint_variance"] += (I - mu) ** 2 * v
            f["joint_entropy"] -= v * lg(v)
            f["angular_second_moment"] += v * v
            f["contrast"] += (I - J) ** 2 * v
            f["dissimilarity"] += abs(I - J) * v
            f["inverse_difference"] += v / (1 + abs(I - J))
            f["inverse_difference_normalised"] += v / (1 + abs(I - J) / ng)
            f["inverse_difference_moment"] += v / (1 + (I - J) ** 2)
            f["inverse_difference_moment_normalised"] += v / (1 + (I - J) ** 2 / ng ** 2)
            if I != J:
                f["inverse_variance"] += v / (I - J) ** 2
            f["correlation"] += (I - mu) * (J - mu) * v / var
            f["autocorrelation"] += I * J * v
            f["cluster_tendency"] += (I + J - 2 * mu) ** 2 * v
            f["cluster_shade"] += (I + J - 2 * mu) ** 3 * v
            f["cluster_prominence"] += (I + J - 2 * mu) ** 4 * v
            hxy1 -= v * lg(px[i] * px[j])
            hxy2 -= px[i] * px[j] * lg(px[i] * px[j])
    hx = -sum(v * lg(v) for v in px)
    f["difference_average"], f["sum_average"] = mud, mus
    f["difference_variance"] = sum((k - mud) ** 2 * pd[k] for k in range(ng))
    f["sum_variance"] = sum((k - mus) ** 2 * v for k, v in ps.items())
    f["difference_entropy"] = -sum(v * lg(v) for v in pd)
    f["sum_entropy"] = -sum(v * lg(v) for v in ps.values())
    f["information_correlation_1"] = (f["joint_entropy"] - hxy1) / hx
    f["information_correlation_2"] = math.sqrt(1 - math.exp(-2 * (hxy2 - f["joint_entropy"])))
    return f


def naive_glrlm(r):
    ng, nr = len(r), len(r[0])
    ns = sum(sum(row) for row in r)
    nv = sum((j + 1) * r[i][j] for i in range(ng) for j in range(nr))
    f = dict.fromkeys(tx.GLRLM_FEATURES, 0.0)
    mui = sum((i + 1) * r[i][j] / ns for i in range(ng) for j in range(nr))
    muj = sum((j + 1) * r[i][j] / ns for i in range(ng) for j in range(nr))
    for i in range(ng):
        for j in range(nr):
            v, I, J = r[i][j], i + 1, j + 1
            f["short_run_emphasis"] += v / J ** 2 / ns
            f["long_run_emphasis"] += v * J ** 2 / ns
            f["low_grey_level_run_emphasis"] += v / I ** 2 / ns
            f["high_grey_level_run_emphasis"] += v * I ** 2 / ns
            f["short_run_low_grey_level_emphasis"] += v / (I ** 2 * J ** 2) / ns
            f["short_run_high_grey_level_emphasis"] += v * I ** 2 / J ** 2 / ns
            f["long_run_low_grey_level_emphasis"] += v * J ** 2 / I ** 2 / ns
            f["long_run_high_grey_level_emphasis"] += v * I ** 2 * J ** 2 / ns
            f["grey_level_variance"] += (I - mui) ** 2 * v / ns
            f["run_length_variance"] += (J - muj) ** 2 * v / ns
            if v:
                f["run_entropy"] -= v / ns * math.log2(v / ns)
    f["grey_level_non_uniformity"] = sum(sum(r[i]) ** 2 for i in range(ng)) / ns
    f["grey_level_non_uniformity_normalised"] = f["grey_level_non_uniformity"] / ns
    f["run_length_non_uniformity"] = sum(sum(r[i][j] for i in range(ng)) ** 2 for j in range(nr)) / ns
    f["run_length_non_uniformity_normalised"] = f["run_length_non_uniformity"] / ns
    f["run_percentage"] = ns / nv
    return f


def test_features_against_naive_evaluation():
    rng = np.random.default_rng(1)
    counts = rng.integers(0, 50, (7, 7))
    counts[rng.random((7, 7)) < 0.3] = 0
    got, want = tx.glcm_features(counts), naive_glcm(counts.tolist())
    assert set(got) == set(tx.GLCM_FEATURES) == set(want) and len(tx.GLCM_FEATURES) == 25
    for k in tx.GLCM_FEATURES:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, err_msg=k)
    runs = rng.integers(0, 30, (6, 9))
    runs[rng.random((6, 9)) < 0.3] = 0
    got, want = tx.glrlm_features(runs), naive_glrlm(runs.tolist())
    assert set(got) == set(tx.GLRLM_FEATURES) == set(want) and len(tx.GLRLM_FEATURES) == 16
    for k in tx.GLRLM_FEATURES:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, err_msg=k)


def test_average_and_merge():
    """Two directions with different matrices: the mean of the features is not the feature of the summed matrix; empty directions
    stay out of the mean; an empty region reports None."""
    g = np.zeros((13, 4, 4), np.int64)
    g[0, 0, 1], g[2, 0, 3], g[2, 1, 1] = 30, 4, 6
    avg, mrg = tx.glcm_features(g, "average"), tx.glcm_features(g, "merge")
    c0, c2 = tx.glcm_features(g[0])["contrast"], tx.glcm_features(g[2])["contrast"]
    assert c0 == 1.0 and c2 == pytest.approx(0.4 * 9, rel=1e-15)
    assert avg["contrast"] == pytest.approx((c0 + c2) / 2, rel=1e-15)
    assert mrg["contrast"] == pytest.approx((30 * 1 + 4 * 9) / 40, rel=1e-15) and mrg["contrast"] != avg["contrast"]
    r = np.zeros((13, 4, 5), np.int64)
    r[1, 2, 0], r[5, 2, 4] = 8, 2
    assert tx.glrlm_features(r, "average")["long_run_emphasis"] == pytest.approx((1 + 25) / 2)
    assert tx.glrlm_features(r, "merge")["long_run_emphasis"] == pytest.approx((8 + 2 * 25) / 10)
    assert all(v is None for v in tx.glcm_features(np.zeros((13, 4, 4))).values())
    assert all(v is None for v in tx.glrlm_features(np.zeros((13, 4, 5)), "merge").values())
    with pytest.raises(ValueError):
        tx.glcm_features(g, "median")


def _expected(lab, vol, n_labels, names=None, aggregate="average", **kw):
    raw = oracle_texture(lab, vol, n_labels, **kw)
    return tx.finalize(raw, oracle_texture((lab > 0).astype(np.uint8), vol, 2, **kw), names, aggregate)


@pytest.mark.parametrize("aggregate", ["average", "merge"])
def test_texture_features_dict(emu_engine, aggregate):
    rng = np.random.default_rng(2)
    lab, vol = random_case(rng, (3, 12, 30), 3, extra=0)
    names = {1: "right lung", 2: "left lung"}
    got = tx.texture_features(vol, lab, names=names, aggregate=aggregate, engine=emu_engine)
    assert got == _expected(lab, vol, 3, names, aggregate)
    assert json.loads(json.dumps(got)) == got
    assert set(got) == {"hu_range", "bin_width", "levels", "distance", "aggregate", "labels", "lung"}
    assert got["levels"] == 48 and got["hu_range"] == [-1000, 199] and set(got["labels"]) == {"1", "2"}
    one = got["labels"]["1"]
    assert one["name"] == "right lung" and one["valid"] == one["voxels"] - one["below"] - one["above"] - one["nonfinite"] > 0
    assert set(one["glcm"]) == set(tx.GLCM_FEATURES) and set(one["glrlm"]) == set(tx.GLRLM_FEATURES)
    assert all(isinstance(v, float) for v in one["glcm"].values())
    # the lung is one region: its pairs cross the border between the labels
    lung = got["lung"]
    assert lung["name"] == "lung" and lung["valid"] == sum(got["labels"][k]["valid"] for k in "12")
    weighted = sum(got["labels"][k]["glrlm"]["run_percentage"] * got["labels"][k]["valid"] for k in "12") / lung["valid"]
    assert lung["glrlm"]["run_percentage"] < weighted * (1 - 1e-9)  # fewer runs than the two labels' together
    other = tx.texture_features(volume_io.Volume(vol, (1.0, 1.0, 2.0)), lab, hu_range=(-1000, 0), bin_width=50, distance=2, engine=emu_engine)
    assert other == _expected(lab, vol, 3, None, "average", hi=0, bin_width=50, distance=2) and other["levels"] == 21


def test_texture_features_empty_label(emu_engine):
    lab = np.zeros((2, 4, 8), np.uint8)
    lab[0, 0, 0] = 2
    vol = np.full(lab.shape, -900, np.int16)
    got = tx.texture_features(vol, lab, engine=emu_engine)
    assert got["labels"]["1"]["voxels"] == 0 and all(v is None for v in got["labels"]["1"]["glrlm"].values())
    two = got["labels"]["2"]
    assert all(v is None for v in two["glcm"].values()) and two["glrlm"]["run_percentage"] == 1.0 and two["longest_run"] == 1


def test_texture_input_validation(emu_engine):
    vol = np.zeros((2, 4, 8), np.int16)
    lab = np.ones((2, 4, 8), np.uint8)
    with pytest.raises(ValueError, match="same shape"):
        tx.texture_features(vol, lab[:, :, :7], engine=emu_engine)
    with pytest.raises(ValueError, match="same shape"):
        tx.texture_matrices(vol[0], lab[0], engine=emu_engine)
    for kw in (dict(hu_range=(0, -1)), dict(bin_width=0), dict(bin_width=2.5), dict(hu_range=(-1000, 600)), dict(distance=0),
               dict(distance=9), dict(hu_range=(-1000,)), dict(n_labels=17), dict(n_labels=0)):
        with pytest.raises(ValueError):
            tx.texture_matrices(vol, lab, engine=emu_engine, **kw)
    with pytest.raises(ValueError, match="aggregate"):
        tx.texture_features(vol, lab, aggregate="sum", engine=emu_engine)
    with pytest.raises(ValueError, match="0..255"):
        tx.texture_matrices(vol, lab.astype(np.int32) * 300, engine=emu_engine)
