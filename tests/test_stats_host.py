"""The host-side finaliser of the per-label statistics (lungmask_amd.stats) on synthetic accumulators and histograms, against numpy on
the expanded values; the JSON round trip; the CLI's --stats argument."""
import json

import numpy as np
import pytest

from lungmask_amd import stats as st
from lungmask_amd import volume_io


def accumulators(values: np.ndarray, index_sum=(0, 0, 0), bbox=(0, 1, 0, 1, 0, 1), nonfinite=0) -> dict:
    hist = np.bincount(np.clip(values, -1024, 3071) + 1024, minlength=4096).astype(np.int64)
    return {"voxels": values.size + nonfinite, "nonfinite": nonfinite, "clipped_low": int((values < -1024).sum()),
            "clipped_high": int((values > 3071).sum()), "hu_min": int(values.min()) if values.size else 0,
            "hu_max": int(values.max()) if values.size else 0, "index_sum": list(index_sum), "bbox": list(bbox), "hist": hist}


CASES = [
    np.random.default_rng(1).normal(-850, 20, 100_000).round().astype(np.int64),
    np.random.default_rng(2).integers(-2000, 4000, 3_333).astype(np.int64),
    np.array([-1024], np.int64),
    np.array([5, 5, 5, 5], np.int64),
    np.array([-960, -950, -951, -949, 100], np.int64),
    np.random.default_rng(3).normal(-700, 250, 7_919).round().astype(np.int64),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_density_figures_against_numpy(case):
    v = CASES[case]
    c = np.clip(v, -1024, 3071)
    qs = (0, 15, 50, 99.9, 100)
    ts = (-950, -910.5, -1024, 3072, -2000)
    got = st.finalize_label(accumulators(v), spacing=(2.5, 0.7, 0.7), percentiles=qs, thresholds=ts)
    assert got["mean"] == np.mean(c)  # exactly
    assert got["std"] == pytest.approx(float(np.std(c)), rel=1e-9, abs=1e-12)
    for q in qs:
        assert got["percentiles"][f"{q:g}"] == pytest.approx(float(np.percentile(c, q)), abs=1e-9), q
    for t in ts:
        assert got["below"][f"{t:g}"] == np.mean(c < t), t  # exactly
    assert got["volume_ml"] == v.size * float(np.prod([2.5, 0.7, 0.7])) / 1000.0
    assert got["hu_min"] == int(v.min()) and got["hu_max"] == int(v.max())


def test_nonfinite_and_empty_labels():
    v = np.array([-900, -800], np.int64)
    got = st.finalize_label(accumulators(v, nonfinite=3), spacing=(1.0, 1.0, 1.0))
    assert got["voxels"] == 5 and got["nonfinite"] == 3 and got["mean"] == -850.0 and got["volume_ml"] == 0.005
    only_nan = st.finalize_label(accumulators(np.zeros(0, np.int64), nonfinite=4), spacing=(1.0, 1.0, 1.0))
    assert only_nan["voxels"] == 4 and only_nan["mean"] is None and only_nan["percentiles"]["15"] is None and only_nan["volume_ml"] == 0.004
    empty = st.finalize_label(accumulators(np.zeros(0, np.int64)), spacing=(1.0, 1.0, 1.0))
    assert empty["voxels"] == 0
    for f in ("volume_ml", "mean", "std", "hu_min", "hu_max", "centroid_index", "centroid_mm", "bbox"):
        assert empty[f] is None, f


def test_centroid_mm_for_a_permuted_flipped_direction():
    direction = np.array([[0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    vol = volume_io.Volume(np.zeros((4, 5, 6), np.int16), spacing=(0.8, 1.25, 3.0), origin=(-10.0, 20.5, 7.0), direction=direction)
    arr, sp, to_phys = st.geometry(vol)
    assert sp == (3.0, 1.25, 0.8)  # array axis order
    idx_sum, n = (7, 11, 13), 5
    got = st.finalize_label(accumulators(np.full(n, -800, np.int64), index_sum=idx_sum), sp, index_to_physical=to_phys)
    c = [s / n for s in idx_sum]
    assert got["centroid_index"] == c
    np.testing.assert_allclose(got["centroid_mm"], vol.index_to_physical(c[::-1]), rtol=0, atol=1e-12)
    with pytest.raises(ValueError, match="spacing"):
        st.geometry(vol, spacing=(1.0, 1.0, 1.0))


def test_finalize_json_round_trip_and_lung_aggregate():
    rng = np.random.default_rng(9)
    a, b = rng.integers(-1000, -700, 50).astype(np.int64), rng.integers(-900, 200, 70).astype(np.int64)
    raw = {f: np.zeros(4, np.int64) for f in ("voxels", "nonfinite", "clipped_low", "clipped_high", "hu_min", "hu_max")}
    raw["index_sum"] = np.zeros((4, 3), np.int64)
    raw["bbox"] = np.full((4, 6), -1, np.int32)
    raw["hist"] = np.zeros((4, 4096), np.int64)
    for k, v, box in ((1, a, (0, 3, 1, 4, 2, 9)), (2, b, (1, 5, 0, 2, 3, 7))):
        acc = accumulators(v, index_sum=(k, 2 * k, 3 * k), bbox=box)
        for f in ("voxels", "nonfinite", "clipped_low", "clipped_high", "hu_min", "hu_max"):
            raw[f][k] = acc[f]
        raw["index_sum"][k], raw["bbox"][k], raw["hist"][k] = acc["index_sum"], acc["bbox"], acc["hist"]
    raw["voxels"][0] = 11
    raw["other"] = 2
    out = st.finalize(raw, spacing=(1.0, 0.5, 0.5), percentiles=(15, 50), names={1: "right lung", 2: "left lung"})
    assert json.loads(json.dumps(out)) == out
    assert out["labels"]["1"]["name"] == "right lung" and out["labels"]["3"]["voxels"] == 0 and out["other_voxels"] == 2
    both = np.concatenate([a, b])
    lung = out["lung"]
    assert lung["voxels"] == both.size and lung["mean"] == np.mean(both)
    assert lung["percentiles"]["15"] == pytest.approx(float(np.percentile(both, 15)), abs=1e-9)
    assert lung["bbox"] == [0, 5, 0, 4, 2, 9] and lung["hu_min"] == int(both.min())
    assert out["voxel_volume_ml"] == 0.25 / 1000.0 and out["hu_window"] == [-1024, 3071]


def test_label_names():
    assert st.label_names("R231", 3) == {1: "right lung", 2: "left lung"}
    assert st.label_names("LTRCLobes", 6)[4] == "right middle lobe"
    assert st.label_names("my_checkpoint.pth", 3) == {1: "label 1", 2: "label 2"}


def test_cli_stats_argument(tmp_path):
    from lungmask_amd.__main__ import build_parser, main

    ip = tmp_path / "in.npy"
    np.save(ip, np.zeros((2, 4, 4), np.int16))
    args = build_parser().parse_args([str(ip), str(tmp_path / "out.nii"), "--stats", "s.json"])
    assert args.stats == "s.json"
    with pytest.raises(SystemExit, match="--stats"):  # before any model is loaded (no GPU needed to get here)
        main([str(ip), str(tmp_path / "out.nii"), "--stats", str(tmp_path / "stats.txt")])
    assert not (tmp_path / "out.nii").exists()
