"""The host side of lungmask_amd.pairs, without an engine: the analysis dict from a hand-written table for the three `roles`, None
on zero denominators, the JSON round trip, every ValueError of the argument checks and jac_scale from an Affine."""
import json
import math

import numpy as np
import pytest

from lungmask_amd import _native as nat
from lungmask_amd import pairs
from lungmask_amd import resample as rs

# selected, valid, outside, nonfinite, folded, sum J (2^-20), sum change (1/16), sum change^2 (1/16), excluded, codes 1 .. 4
TABLE = [[0] * 13,
         [100, 80, 10, 6, 4, 88 << 20, -16 * 400, 16 * 8000, 20, 30, 15, 10, 5],
         [50, 50, 0, 0, 0, 45 << 20, 16 * 125, 16 * 1250, 50, 0, 0, 0, 0],
         [7, 0, 7, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]]
SPACING = (2.0, 0.5, 0.5)  # 0.5 mm^3 = 0.0005 ml per voxel


@pytest.mark.parametrize("roles,names,thresholds", [
    (("inspiration", "expiration"), ("normal", "uncategorised", "fsad", "emphysema"), (-950.0, -856.0)),
    (("expiration", "inspiration"), ("normal", "fsad", "uncategorised", "emphysema"), (-856.0, -950.0)),
    (None, ("neither", "fixed_only", "moving_only", "both"), (-950.0, -950.0))])
def test_analysis_from_a_hand_written_table(roles, names, thresholds):
    cfg = pairs.check_arguments(roles)
    assert cfg["class_names"] == names and (cfg["fixed_thr"], cfg["moving_thr"]) == thresholds
    a = pairs.analysis_from_table(np.array(TABLE, np.int64), cfg, {1: "right", 2: "left"}, SPACING, 1.25, "affine")
    assert a["roles"] == (None if roles is None else list(roles)) and a["class_names"] == list(names)
    assert (a["fixed_threshold"], a["moving_threshold"], a["hu_range"], a["air_hu"], a["jac_scale"]) == thresholds + ([-1000.0, -500.0], -1000.0, 1.25)
    assert a["n_labels"] == 4 and a["voxel_volume_ml"] == 0.0005 and sorted(a["labels"]) == ["0", "1", "2", "3"]
    r = a["labels"]["1"]
    assert (r["name"], r["voxels"], r["analysed"], r["outside"], r["nonfinite"], r["folded"], r["excluded"], r["classified"]) == \
        ("right", 100, 80, 10, 6, 4, 20, 60)
    assert [r["classes"][n]["voxels"] for n in names] == [30, 15, 10, 5]
    assert [r["classes"][n]["fraction"] for n in names] == [0.5, 0.25, 10 / 60, 5 / 60]
    assert r["classes"][names[0]]["ml"] == 30 * 0.0005
    assert (r["mean_jacobian"], r["mean_change_hu"], r["rms_change_hu"]) == (1.1, -5.0, 10.0)
    assert r["volume_fixed_ml"] == 100 * 0.0005 and r["volume_moving_ml"] == 1.1 * 80 * 0.0005
    assert a["labels"]["2"]["name"] == "left" and a["labels"]["3"]["name"] == "label 3" and a["labels"]["0"]["name"] == "background"
    # the lung row is the exact column sum of the rows of the labels >= 1
    lung = a["lung"]
    assert (lung["name"], lung["voxels"], lung["analysed"], lung["outside"], lung["excluded"], lung["classified"]) == ("lung", 157, 130, 17, 70, 60)
    assert lung["mean_jacobian"] == (133 << 20) / 2 ** 20 / 130 and lung["mean_change_hu"] == (-400 + 125) / 130
    assert lung["rms_change_hu"] == math.sqrt((8000 + 1250) / 130)
    assert json.loads(json.dumps(a)) == a


def test_zero_denominators_give_none():
    cfg = pairs.check_arguments()
    a = pairs.analysis_from_table(TABLE, cfg, None, None)
    empty, unclassified, outside = a["labels"]["0"], a["labels"]["2"], a["labels"]["3"]
    for r in (empty, outside):
        assert r["mean_jacobian"] is None and r["mean_change_hu"] is None and r["rms_change_hu"] is None and r["volume_moving_ml"] is None
        assert all(c["fraction"] is None for c in r["classes"].values())
    assert unclassified["mean_jacobian"] == 0.9 and unclassified["classified"] == 0
    assert all(c["fraction"] is None and c["voxels"] == 0 for c in unclassified["classes"].values())
    # without a spacing there are no volumes anywhere
    assert a["spacing_mm"] is None and a["voxel_volume_ml"] is None
    assert all(r["volume_fixed_ml"] is None and r["volume_moving_ml"] is None and all(c["ml"] is None for c in r["classes"].values())
               for r in list(a["labels"].values()) + [a["lung"]])
    assert json.loads(json.dumps(a)) == a


@pytest.mark.parametrize("kw,text", [
    (dict(roles=("inspiration", "inspiration")), "roles"),
    (dict(roles="insp"), "roles"),
    (dict(fixed_threshold=-400.0), "fixed_threshold"),
    (dict(moving_threshold=-1001.0), "moving_threshold"),
    (dict(moving_threshold=float("nan")), "moving_threshold"),
    (dict(hu_range=(-500, -1000)), "hu_range"),
    (dict(hu_range=(-1000,)), "hu_range"),
    (dict(hu_range=(-1000, float("inf"))), "hu_range"),
    (dict(air_hu=float("nan")), "air_hu"),
    (dict(n_labels=0), "n_labels"),
    (dict(n_labels=17), "n_labels"),
    (dict(maps=("classes", "labels")), "maps"),
    (dict(keep=(1, 256)), "keep")])
def test_argument_errors(kw, text):
    with pytest.raises(ValueError, match=text):
        pairs.check_arguments(**kw)


def test_shape_and_label_errors_come_before_the_engine():
    vol, lab = np.zeros((2, 3, 4), np.int16), np.zeros((2, 3, 4), np.uint8)
    with pytest.raises(ValueError, match="must have the fixed volume's shape"):
        pairs.pair_analysis(vol, vol, np.zeros((2, 3, 5), np.uint8), engine=object())
    high = lab.copy()
    high[0, 0, 0] = 16
    with pytest.raises(ValueError, match="n_labels"):
        pairs.pair_analysis(vol, vol, high, engine=object())
    assert pairs.label_count(high, 4, None) == 4 and pairs.label_count(high, None, {1: "a", 5: "b"}) == 6 and pairs.label_count(lab, None, None) == 1
    with pytest.raises(ValueError, match="3-D"):
        pairs.pair_analysis(np.zeros((3, 4), np.int16), vol, lab, engine=object())
    with pytest.raises(TypeError, match="transform"):
        pairs.pair_analysis(vol, vol, lab, transform=np.eye(4), engine=object())
    from lungmask_amd import deformable as dfm

    field = dfm.DisplacementField.zeros(rs.Grid((2, 3, 5), (1.0, 1.0, 1.0)))
    with pytest.raises(ValueError, match="field's grid"):
        pairs.pair_analysis(vol, vol, lab, transform=field, engine=object())


def test_jac_scale_of_an_affine():
    assert pairs.jac_scale(None) == 1.0 and pairs.jac_scale(rs.Affine()) == 1.0
    assert pairs.jac_scale(rs.Affine.translation((3.0, -2.0, 1.0))) == 1.0
    assert abs(pairs.jac_scale(rs.Affine.rotation((0, 0, 1), 30.0)) - 1.0) < 1e-12
    m = np.array([[0.0, 2.0, 0.0], [1.5, 0.0, 0.0], [0.0, 0.0, 0.5]])  # a reflection: the scale is the ABSOLUTE determinant
    assert np.linalg.det(m) < 0 and abs(pairs.jac_scale(rs.Affine(m, (1.0, 2.0, 3.0))) - 1.5) < 1e-12
    with pytest.raises(ValueError, match="singular"):
        pairs.jac_scale(rs.Affine(np.zeros((3, 3)), (0.0, 0.0, 0.0)))
    assert pairs.split_transform(None) == (None, None)
    a = rs.Affine.translation((1.0, 0.0, 0.0))
    assert pairs.split_transform(a) == (a, None)
    assert nat.LM_PAIR_COLS == 13 == len(nat.PAIR_COLS)
