"""The Python layer of the component analysis (lungmask_amd.components) on the emulator engine: renumbering, derived columns, the
cluster summary and its exponent D, geometry from images, JSON, the command line and argument errors."""
import json

import numpy as np
import pytest

from lungmask_amd import components as cp
from lungmask_amd import stats as lmstats
from lungmask_amd import volume_io
from tests.cli_fake import FakeInferer
from tests.test_components_emu import oracle_components, random_case


def cubes_volume():
    """Two labels (split at x = 24) with cubes of -1000 HU in a -800 HU background: label 1 holds cubes of edge 1, 1, 1, 2, 2, 3, label 2
    cubes of edge 1, 2, 3, 4, 4.  Sizes 1, 8, 27, 64 voxels.  One more cube of edge 2 straddles the border: two clusters of 4 voxels per
    label, one of 8 for the lung."""
    lab = np.zeros((12, 20, 48), np.uint8)
    lab[1:11, 1:19, 1:24] = 1
    lab[1:11, 1:19, 24:47] = 2
    img = np.full(lab.shape, -800, np.int16)
    img[lab == 0] = -1000  # outside the labels: never selected

    def cube(z, y, x, e):
        img[z:z + e, y:y + e, x:x + e] = -1000

    for z, y, x, e in ((2, 2, 2, 1), (2, 2, 5, 1), (2, 2, 8, 1), (2, 6, 2, 2), (2, 6, 6, 2), (5, 12, 3, 3)):
        cube(z, y, x, e)
    for z, y, x, e in ((2, 2, 28, 1), (2, 6, 28, 2), (2, 12, 28, 3), (2, 2, 34, 4), (2, 10, 40, 4)):
        cube(z, y, x, e)
    cube(8, 2, 23, 2)  # x = 23 (label 1) and x = 24 (label 2)
    return img, lab


def test_renumbering_is_stable():
    vox = np.array([5, 9, 1, 9, 2, 5], np.int64)
    lut, old = cp.renumbering(vox, 1, "size")
    assert old.tolist() == [2, 4, 1, 6, 5, 3] and lut.tolist() == [0, 3, 1, 6, 2, 5, 4]
    lut, old = cp.renumbering(vox, 3, "raster")
    assert old.tolist() == [1, 2, 4, 6] and lut.tolist() == [0, 1, 2, 0, 3, 0, 4]
    lut, old = cp.renumbering(vox, 1, "raster")
    assert lut is None and old.tolist() == [1, 2, 3, 4, 5, 6]
    assert cp.renumbering(np.array([9, 5, 5, 1], np.int64), 1, "size")[0] is None  # already in order


def test_find_components_order_and_compaction(emu_engine):
    labels, image = random_case((5, 33, 70), 11)
    kw = dict(hu_range=(None, -500))
    ids0, T, _, rows0, _ = oracle_components(labels, image, **kw)
    base = cp.find_components(image, labels, engine=emu_engine, **kw)
    assert base.count == T and np.array_equal(base.ids, ids0) and np.array_equal(base.table["voxels"], rows0["voxels"])
    assert np.array_equal(base.counts["selected"], np.bincount(labels[ids0 > 0], minlength=256))
    assert cp.label_components(labels, image, engine=emu_engine, **kw)[1] == T
    assert np.array_equal(cp.label_components(labels, image, engine=emu_engine, **kw)[0], ids0)
    for order, mv in (("size", 1), ("raster", 3), ("size", 2)):
        got = cp.find_components(image, labels, order=order, min_voxels=mv, engine=emu_engine, **kw)
        old = np.flatnonzero(rows0["voxels"] >= mv) + 1
        if order == "size":
            old = np.array(sorted(old, key=lambda i: (-rows0["voxels"][i - 1], i)))
        lut = np.zeros(T + 1, np.int32)
        lut[old] = np.arange(1, len(old) + 1)
        assert got.count == len(old) and np.array_equal(got.ids, lut[ids0])
        for f in ("voxels", "first", "label", "bbox", "index_sum", "hu_sum", "hu_min", "hu_max", "faces"):  # rows follow the new ids
            assert np.array_equal(got.table[f], rows0[f][old - 1]), f
        if order == "size":
            assert (np.diff(got.table["voxels"]) <= 0).all()
        for i in (1, got.count):  # a row describes the voxels that carry its id
            assert got.table["voxels"][i - 1] == (got.ids == i).sum()


def test_derived_columns_of_a_box(emu_engine):
    lab = np.zeros((5, 6, 7), np.uint8)
    lab[1:3, 2:5, 1:5] = 4  # 2 x 3 x 4
    img = np.full(lab.shape, -7, np.int16)
    sp = (2.5, 0.5, 0.8)  # z, y, x
    c = cp.find_components(img, lab, spacing=sp, engine=emu_engine)
    t = c.table
    assert c.count == 1 and t["voxels"][0] == 24 and t["label"][0] == 4 and t["first"][0] == (1 * 6 + 2) * 7 + 1
    assert t["bbox"][0].tolist() == [1, 3, 2, 5, 1, 5] and t["faces"][0].tolist() == [24, 16, 12]
    assert t["centroid_index"][0].tolist() == [1.5, 3.0, 2.5] and t["centroid_mm"] is None
    assert t["volume_ml"][0] == pytest.approx(24 * 2.5 * 0.5 * 0.8 / 1000, rel=1e-15)
    assert t["surface_area_mm2"][0] == pytest.approx(24 * 0.5 * 0.8 + 16 * 2.5 * 0.8 + 12 * 2.5 * 0.5, rel=1e-15)
    assert t["equivalent_diameter_mm"][0] == pytest.approx((6 * 24 * 2.5 * 0.5 * 0.8 / np.pi) ** (1 / 3), rel=1e-14)
    assert t["mean_hu"][0] == -7.0 and t["hu_min"][0] == t["hu_max"][0] == -7 and t["hu_sum"][0] == -7 * 24
    none = cp.find_components(None, lab, engine=emu_engine)
    assert none.table["hu_sum"] is None and none.table["mean_hu"] is None and none.table["volume_ml"] is None
    # a Volume brings spacing (x, y, z), origin and a direction that is not the identity
    d = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])
    vol = volume_io.Volume(img, sp[::-1], (10.0, 20.0, 30.0), d)
    cv = cp.find_components(vol, lab, engine=emu_engine)
    want = np.array([10.0, 20.0, 30.0]) + d @ (np.array([2.5, 3.0, 1.5]) * np.array(sp[::-1]))
    np.testing.assert_allclose(cv.table["centroid_mm"][0], want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(cv.table["centroid_mm"][0], vol.index_to_physical([2.5, 3.0, 1.5]), rtol=0, atol=1e-12)
    assert cv.table["volume_ml"][0] == t["volume_ml"][0] and cv.table["surface_area_mm2"][0] == t["surface_area_mm2"][0]
    with pytest.raises(ValueError, match="spacing"):
        cp.find_components(vol, lab, spacing=sp, engine=emu_engine)  # spacing given twice
    m = json.loads(json.dumps(cv.meta()))
    assert m["count"] == 1 and m["table"]["voxels"] == [24] and m["counts"]["4"] == {"voxels": 24, "nonfinite": 0, "selected": 24}
    assert m["connectivity"] == 6 and m["per_label"] is True and "table" not in cv.meta(table=False)


def exponent_by_polyfit(sizes):
    s = np.unique(sizes)
    y = np.array([(np.asarray(sizes) >= v).sum() for v in s], np.float64)
    return -np.polyfit(np.log10(s.astype(np.float64)), np.log10(y), 1)[0]


def test_cluster_analysis_known_sizes(emu_engine):
    img, lab = cubes_volume()
    sp = (2.0, 0.5, 0.5)
    res = cp.cluster_analysis(img, lab, spacing=sp, names={1: "one", 2: "two", 3: "three"}, engine=emu_engine)
    assert res["threshold"] == -950 and res["hu_range"] == [None, -951] and res["connectivity"] == 6
    a, b, c, lung = res["labels"]["1"], res["labels"]["2"], res["labels"]["3"], res["lung"]
    sizes_a, sizes_b = [1, 1, 1, 8, 8, 27, 4], [1, 8, 27, 64, 64, 4]
    assert a["name"] == "one" and a["clusters"] == 7 and b["clusters"] == 6
    assert a["voxels"] == (lab == 1).sum() and a["nonfinite"] == 0 and a["selected"] == sum(sizes_a)
    assert a["fraction"] == sum(sizes_a) / (lab == 1).sum() and b["fraction"] == sum(sizes_b) / (lab == 2).sum()
    assert a["size_histogram"] == [3, 0, 1, 2, 1] and b["size_histogram"] == [1, 0, 1, 1, 1, 0, 2]  # bins 1, 2-3, 4-7, 8-15, 16-31, 32-63, 64-127
    assert (a["largest_voxels"], b["largest_voxels"]) == (27, 64) and a["median_voxels"] == 4.0 and b["median_voxels"] == 17.5
    assert a["mean_voxels"] == sum(sizes_a) / 7 and b["largest_ml"] == pytest.approx(64 * 0.5 / 1000, rel=1e-15)
    assert a["D"] == pytest.approx(exponent_by_polyfit(sizes_a), rel=1e-12) and b["D"] == pytest.approx(exponent_by_polyfit(sizes_b), rel=1e-12)
    assert a["D"] > 0
    assert c == {"name": "three", "voxels": 0, "nonfinite": 0, "selected": 0, "fraction": None, "clusters": None, "largest_voxels": None,
                 "largest_ml": None, "mean_voxels": None, "median_voxels": None, "size_histogram": None, "D": None}
    # the lung merges the cube that the border between the labels splits
    sizes_l = [1, 1, 1, 8, 8, 27, 1, 8, 27, 64, 64, 8]
    assert lung["clusters"] == 12 and lung["selected"] == sum(sizes_l) == a["selected"] + b["selected"]
    assert lung["size_histogram"] == [4, 0, 0, 4, 2, 0, 2] and lung["D"] == pytest.approx(exponent_by_polyfit(sizes_l), rel=1e-12)
    assert json.loads(json.dumps(res)) == res
    # two distinct sizes: no exponent
    two = cp.cluster_analysis(np.where(lab == 2, -800, img).astype(np.int16), np.where(lab == 2, 0, lab), hu_range=(None, -951),
                              engine=emu_engine)["labels"]["1"]
    assert two["clusters"] == 7 and two["D"] is not None  # sizes 1, 4, 8, 27
    img2 = img.copy()
    img2[5:8, 12:15, 3:6] = -800
    img2[8:10, 2:4, 23:25] = -800  # without the 27 and the 4: sizes 1 and 8
    only = cp.cluster_analysis(img2, np.where(lab == 2, 0, lab), engine=emu_engine)
    assert only["labels"]["1"]["clusters"] == 5 and only["labels"]["1"]["D"] is None and only["threshold"] == -950
    assert cp.cluster_exponent([3, 3, 7]) is None and cp.cluster_exponent([]) is None
    # a high-attenuation range instead of the threshold; an image brings its spacing
    hi = cp.cluster_analysis(volume_io.Volume(img, sp[::-1]), lab, hu_range=(-900, None), engine=emu_engine)
    assert hi["threshold"] is None and hi["hu_range"] == [-900, None] and hi["spacing_mm"] == list(sp)
    assert hi["labels"]["1"]["clusters"] == 1 and hi["labels"]["1"]["selected"] == (lab == 1).sum() - sum(sizes_a)
    assert hi["lung"]["clusters"] == 1 and hi["lung"]["largest_ml"] == pytest.approx(hi["lung"]["selected"] * 0.5 / 1000)


def test_selection_matches_the_statistics(emu_engine):
    labels, image = random_case((5, 33, 70), 3)
    labels = np.minimum(labels, 2)
    res = cp.cluster_analysis(image, labels, engine=emu_engine)
    st = lmstats.label_statistics(image, labels, engine=emu_engine)
    for k in ("1", "2"):
        assert res["labels"][k]["fraction"] == st["labels"][k]["below"]["-950"]
    assert res["lung"]["fraction"] == st["lung"]["below"]["-950"]


def test_cli_clusters(emu_engine, tmp_path, monkeypatch):
    import lungmask_amd.__main__ as cli

    arr, lab = cubes_volume()
    img = volume_io.Volume(arr, (0.7, 0.8, 2.5), (1.0, 2.0, 3.0))
    ip = tmp_path / "in.nii.gz"
    volume_io.write_nifti(str(ip), img)
    FakeInferer.engine, FakeInferer.labels = emu_engine, lab
    monkeypatch.setattr(cli, "LMInferer", FakeInferer)
    monkeypatch.setattr(emu_engine, "n_classes", lambda slot: 3, raising=False)  # (no model is loaded into the emulated engine)
    loaded = volume_io.load_input_image(str(ip))
    names = lmstats.label_names("R231", 3)
    assert cli.main([str(ip), str(tmp_path / "o.npy"), "--noprogress", "--clusters", str(tmp_path / "c.json"), "--cluster-ids",
                     str(tmp_path / "ids.npy")]) == 0
    want = cp.cluster_analysis(loaded, lab, names=names, engine=emu_engine)
    assert json.load(open(tmp_path / "c.json")) == json.loads(json.dumps(want)) and want["lung"]["clusters"] == 12
    ids = np.load(tmp_path / "ids.npy")
    ref = cp.find_components(loaded, lab, hu_range=(None, -951), per_label=False, order="size", engine=emu_engine)
    assert ids.dtype == np.int32 and np.array_equal(ids, ref.ids) and (ids == 1).sum() == 64
    assert np.array_equal(np.load(tmp_path / "o.npy"), lab)
    # beside --stats, another threshold and connectivity, ids into an image container
    assert cli.main([str(ip), str(tmp_path / "o2.npy"), "--noprogress", "--clusters", str(tmp_path / "c2.json"), "--cluster-threshold", "-700",
                     "--cluster-connectivity", "26", "--stats", str(tmp_path / "s.json"), "--cluster-ids", str(tmp_path / "ids.nii.gz")]) == 0
    want2 = cp.cluster_analysis(loaded, lab, threshold=-700, connectivity=26, names=names, engine=emu_engine)
    assert json.load(open(tmp_path / "c2.json")) == json.loads(json.dumps(want2)) and want2["lung"]["clusters"] == 1
    assert json.load(open(tmp_path / "s.json"))["labels"]["1"]["voxels"] == (lab == 1).sum()
    back = volume_io.load_input_image(str(tmp_path / "ids.nii.gz"))
    assert back.array.dtype == np.int32 and np.array_equal(back.array, (lab > 0).astype(np.int32))
    np.testing.assert_allclose(back.spacing, loaded.spacing, atol=1e-6)
    out = str(tmp_path / "o3.npy")
    for bad in (["--cluster-threshold", "-900"], ["--cluster-ids", "i.npy"], ["--cluster-connectivity", "26"],
                ["--clusters", "c.txt"], ["--clusters", "c.json", "--cluster-ids", "i.dcm"]):
        with pytest.raises(SystemExit, match="--cluster"):  # refused before anything is loaded
            cli.main([str(ip), out] + bad)
    with pytest.raises(SystemExit):
        cli.main([str(ip), out, "--clusters", "c.json", "--cluster-connectivity", "18"])
    a = cli.build_parser().parse_args([str(ip), out, "--clusters", "c.json", "--stats", "s.json", "--roi", "r.mha", "--mesh", "m.obj",
                                       "--texture", "t.json", "--closed", "c.npy", "--probabilities", "p.npy", "--metrics", "m.json",
                                       "--compare-to", "x.npy", "--modelname", "LTRCLobes_R231"])
    assert a.clusters == "c.json" and a.cluster_threshold is None and a.cluster_connectivity is None and a.cluster_ids is None


def test_argument_errors(emu_engine):
    labels, image = random_case((3, 8, 9), 2)
    for fn in (lambda **kw: cp.find_components(image, labels, engine=emu_engine, **kw),
               lambda **kw: cp.label_components(labels, image, engine=emu_engine, **kw)):
        with pytest.raises(ValueError, match="connectivity"):
            fn(connectivity=18)
        with pytest.raises(ValueError, match="lo <= hi"):
            fn(hu_range=(5, -5))
        with pytest.raises(ValueError, match="keep"):
            fn(keep=[0])
    with pytest.raises(ValueError, match="connectivity"):
        cp.cluster_analysis(image, labels, connectivity=18, engine=emu_engine)
    with pytest.raises(ValueError, match="lo <= hi"):
        cp.cluster_analysis(image, labels, hu_range=(5, -5), engine=emu_engine)
    with pytest.raises(ValueError, match="same shape"):
        cp.find_components(image[:, :, :5], labels, engine=emu_engine)
    with pytest.raises(ValueError, match="same shape"):
        cp.cluster_analysis(image[0], labels[0], engine=emu_engine)
    with pytest.raises(ValueError, match="0..255"):
        cp.find_components(image, labels.astype(np.int32) * 100, engine=emu_engine)
    with pytest.raises(ValueError, match="spacing"):
        cp.cluster_analysis(volume_io.Volume(image, (1.0, 1.0, 2.0)), labels, spacing=(2.0, 1.0, 1.0), engine=emu_engine)
    with pytest.raises(ValueError, match="spacing"):
        cp.find_components(image, labels, spacing=(1.0, 2.0), engine=emu_engine)
    with pytest.raises(ValueError, match="min_voxels"):
        cp.find_components(image, labels, min_voxels=0, engine=emu_engine)
    with pytest.raises(ValueError, match="order"):
        cp.find_components(image, labels, order="volume", engine=emu_engine)
    with pytest.raises(ValueError, match="hu_range needs an image"):
        cp.find_components(None, labels, hu_range=(None, -950), engine=emu_engine)
    with pytest.raises(ValueError, match="threshold"):
        cp.cluster_analysis(image, labels, threshold=-950.5, engine=emu_engine)
