"""Host side of the label agreement metrics (lungmask_amd.metrics): the finaliser applied to raw rows against the medpy recipe
written out with scipy on float64, the None rules, the JSON round trip, spacing / geometry errors and names.  No engine."""
import json
import math

import numpy as np
import pytest

from lungmask_amd import metrics as lm
from lungmask_amd import volume_io
from tests.test_metrics_emu import blobs, oracle_agreement

ndi = pytest.importorskip("scipy.ndimage")


def medpy_distances(A, B, spacing):
    """medpy.metric.binary.__surface_distances: distances from the surface of A to the surface of B."""
    fp = ndi.generate_binary_structure(3, 1)
    sa = A ^ ndi.binary_erosion(A, structure=fp, iterations=1)
    sb = B ^ ndi.binary_erosion(B, structure=fp, iterations=1)
    return ndi.distance_transform_edt(~sb, sampling=spacing)[sa]


@pytest.mark.parametrize("spacing", [None, (2.5, 0.7421875, 0.7421875)])
def test_finalize_matches_the_medpy_recipe(spacing):
    rng = np.random.default_rng(1)
    a = blobs(rng, (8, 20, 30), 3)
    b = np.roll(a, (1, 1, 2), (0, 1, 2))
    b[rng.random(b.shape) < 0.03] = 0
    qs = (50, 95)
    out = lm.finalize(oracle_agreement(a, b, 3, spacing, qs) | {"percentiles": list(qs)}, spacing, {1: "right lung", 2: "left lung"})
    assert out["unit"] == ("voxel" if spacing is None else "mm") and out["spacing_mm"] == (None if spacing is None else list(spacing))
    assert out["labels"]["1"]["name"] == "right lung" and out["lung"]["name"] == "lung" and set(out["labels"]) == {"1", "2"}
    vox_ml = None if spacing is None else float(np.prod(spacing)) / 1000.0
    for key, A, B in (("1", a == 1, b == 1), ("2", a == 2, b == 2), ("lung", a >= 1, b >= 1)):
        row = out["lung"] if key == "lung" else out["labels"][key]
        va, vb, i = int(A.sum()), int(B.sum()), int((A & B).sum())
        assert (row["voxels_a"], row["voxels_b"], row["intersection"]) == (va, vb, i)
        assert row["dice"] == pytest.approx(2 * i / (va + vb), rel=1e-15) and row["jaccard"] == pytest.approx(i / (va + vb - i), rel=1e-15)
        assert row["relative_volume_difference"] == pytest.approx((va - vb) / vb, rel=1e-15)
        if spacing is None:
            assert row["volume_a_ml"] is None and row["volume_difference_ml"] is None
        else:
            assert row["volume_a_ml"] == pytest.approx(va * vox_ml) and row["volume_difference_ml"] == pytest.approx((va - vb) * vox_ml)
        dab, dba = medpy_distances(A, B, spacing), medpy_distances(B, A, spacing)
        assert (row["surface_voxels_a"], row["surface_voxels_b"]) == (dab.size, dba.size)
        assert row["hausdorff"] == pytest.approx(max(dab.max(), dba.max()), rel=1e-6)
        assert row["mean_a_to_b"] == pytest.approx(dab.mean(), rel=1e-6) and row["mean_b_to_a"] == pytest.approx(dba.mean(), rel=1e-6)
        assert row["assd"] == pytest.approx(np.concatenate([dab, dba]).mean(), rel=1e-6)
        for q in qs:
            p = row["percentiles"][str(q)]
            assert p["a_to_b"] == pytest.approx(np.percentile(dab, q), rel=1e-6)
            assert p["b_to_a"] == pytest.approx(np.percentile(dba, q), rel=1e-6)
            assert p["pooled"] == pytest.approx(np.percentile(np.hstack((dab, dba)), q), rel=1e-6)  # q = 95: medpy's hd95
    assert json.loads(json.dumps(out)) == out


def test_none_rules():
    a = np.zeros((4, 6, 8), np.uint8)
    b = np.zeros((4, 6, 8), np.uint8)
    a[1:3, 1:4, 2:6] = 1  # label 1 only in a; label 2 in neither
    out = lm.finalize(oracle_agreement(a, b, 3, None, (95,)) | {"percentiles": [95]}, None, None)
    r1, r2 = out["labels"]["1"], out["labels"]["2"]
    assert r1["name"] == "label 1" and r1["dice"] == 0.0 and r1["jaccard"] == 0.0 and r1["relative_volume_difference"] is None
    assert r1["bbox"] == [1, 3, 1, 4, 2, 6] and r1["surface_voxels_a"] == 24 and r1["surface_voxels_b"] == 0
    for f in ("hausdorff", "mean_a_to_b", "mean_b_to_a", "assd"):
        assert r1[f] is None and r2[f] is None
    assert r1["percentiles"] == {"95": {"a_to_b": None, "b_to_a": None, "pooled": None}}
    assert r2["dice"] is None and r2["jaccard"] is None and r2["bbox"] is None and r2["voxels_a"] == 0
    assert json.loads(json.dumps(out)) == out
    same = lm.finalize(oracle_agreement(a, a, 2, (1.0, 1.0, 1.0), (95,)) | {"percentiles": [95]}, (1.0, 1.0, 1.0), None)
    assert same["labels"]["1"]["dice"] == 1.0 and same["labels"]["1"]["hausdorff"] == 0.0 and same["labels"]["1"]["assd"] == 0.0
    assert same["labels"]["1"]["relative_volume_difference"] == 0.0 and same["labels"]["1"]["volume_difference_ml"] == 0.0


def test_percentile_interpolation_is_numpys():
    rng = np.random.default_rng(3)
    for n in (1, 2, 7, 100):
        v = np.sort(rng.random(n))
        for q in (0, 12.5, 50, 95, 99.9, 100):
            pos = (q / 100.0) * (n - 1)
            lo, hi = v[min(math.floor(pos), n - 1)], v[min(math.ceil(pos), n - 1)]
            assert lm._lerp_percentile(lo, hi, n, q) == pytest.approx(np.percentile(v, q), rel=1e-14, abs=0)


def test_input_checks():
    a = np.zeros((2, 4, 4), np.int16)
    vol = volume_io.Volume(np.zeros((2, 4, 4), np.uint8), (0.7, 0.8, 2.5))
    la, lb, sp = lm.label_inputs(a, vol)
    assert la.dtype == np.uint8 and sp == (2.5, 0.8, 0.7)  # the Volume's spacing, in array axis order
    assert lm.label_inputs(a, a, (2.0, 1.0, 1.0))[2] == (2.0, 1.0, 1.0) and lm.label_inputs(a, a)[2] is None
    with pytest.raises(ValueError, match="do not pass"):
        lm.label_inputs(a, vol, (1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="same shape"):
        lm.label_inputs(a, np.zeros((2, 4, 5), np.uint8))
    with pytest.raises(ValueError, match="0..255"):
        lm.label_inputs(a + 300, a)
    with pytest.raises(ValueError, match="0..255"):
        lm.label_inputs(a, a - 1)
    with pytest.raises(ValueError, match="integer"):
        lm.label_inputs(a.astype(np.float32), a)
    with pytest.raises(ValueError):
        lm.label_inputs(a, a, (1.0, 1.0))
    with pytest.raises(ValueError, match="geometry"):
        lm.label_inputs(vol, volume_io.Volume(vol.array, (0.7, 0.8, 2.0)))
    flipped = volume_io.Volume(vol.array, vol.spacing, direction=np.diag([1.0, -1.0, 1.0]))
    with pytest.raises(ValueError, match="geometry"):
        lm.label_inputs(vol, flipped)
    assert lm.label_inputs(vol, volume_io.Volume(vol.array, (0.7 * (1 + 1e-7), 0.8, 2.5)))[2] == (2.5, 0.8, 0.7)
    with pytest.raises(ValueError):
        lm.distance_transform(np.zeros((4, 4), np.uint8))
    with pytest.raises(ValueError):
        lm.distance_transform(np.zeros((2, 4, 4), np.uint8), spacing=(1.0, 1.0))


def test_cli_refuses_half_a_pair(tmp_path):
    from lungmask_amd.__main__ import main

    f = tmp_path / "v.npy"
    np.save(f, np.zeros((1, 16, 16), np.int16))
    for extra in (["--compare-to", str(f)], ["--metrics", str(tmp_path / "m.json")], ["--compare-to", str(f), "--metrics", str(tmp_path / "m.txt")],
                  ["--compare-to", str(tmp_path / "missing.npy"), "--metrics", str(tmp_path / "m.json")]):
        with pytest.raises(SystemExit) as ei:
            main([str(f), str(tmp_path / "o.npy")] + extra)
        assert isinstance(ei.value.code, str), extra  # refused with a message, before anything is loaded
