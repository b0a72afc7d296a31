"""lungmask_amd.skeleton on the host and the emulator engine: skeleton_graph on hand-written skeletons with their expected segments,
lengths and attachments, vessel_tree's dict against a direct numpy evaluation of its definitions, the JSON round trip, names, the
LMInferer method around fixed labels, and the command line."""
import json
import math

import numpy as np
import pytest
from scipy import ndimage as ndi

from lungmask_amd import skeleton as sk
from lungmask_amd import vessels as vs
from lungmask_amd import volume_io
from tests.cli_fake import FakeInferer
from tests.test_filters_emu import assert_same_bits
from tests.test_skeleton_emu import S26, oracle_calibre, oracle_skeleton

SHAPE = (12, 40, 48)
SP = (2.0, 1.0, 0.8)
R2 = math.sqrt(2.0)


def codes_of(mask):
    """The code volume of a hand-written skeleton: 1 + the number of neighbours."""
    count = ndi.convolve(mask.astype(np.int32), np.ones((3, 3, 3), np.int32), mode="constant")
    return np.where(mask, count, 0).astype(np.uint8)


def plane(shape, voxels, z=2):
    m = np.zeros((5,) + shape, bool)
    for y, x in voxels:
        m[z, y, x] = True
    return m


def brief(seg):
    return seg["voxels"], round(seg["length_mm"], 9), seg["closed"], seg["ends"]


# ---- skeleton_graph on hand-written skeletons -------------------------------------------------------------------------------------------
def test_graph_of_a_y():
    stem = [(4, x) for x in range(4)]
    m = plane((9, 9), stem + [(4, 4), (3, 5), (2, 6), (1, 7), (5, 5), (6, 6), (7, 7)])
    codes = codes_of(m)
    assert codes[2, 4, 4] == 4 and (codes[m] >= 2).all() and (codes == 4).sum() == 1
    g = sk.skeleton_graph(codes)
    assert g["voxels"] == 11 and g["end_points"] == 3 and g["isolated"] == 0 and g["spacing_mm"] is None
    assert g["junctions"] == [{"id": 0, "voxels": 1, "index": (2 * 9 + 4) * 9 + 4}]
    # numbered by the first raster index: the arm towards y = 1, the stem, the arm towards y = 7
    assert [brief(s) for s in g["segments"]] == [(3, round(2 * R2, 9), False, [None, 0]), (4, 3.0, False, [None, 0]),
                                                 (3, round(2 * R2, 9), False, [0, None])]
    assert [s["first_index"] for s in g["segments"]] == [(2 * 9 + 1) * 9 + 7, (2 * 9 + 4) * 9 + 0, (2 * 9 + 5) * 9 + 5]
    assert all(s["radius_mm"] is None for s in g["segments"])
    # a spacing scales the steps per axis; radii are sampled on the segments
    radius = np.zeros(m.shape)
    radius[2, 4, :4] = [1.0, 2.0, 3.0, 6.0]
    g = sk.skeleton_graph(codes, spacing=(2.0, 1.0, 0.5), radius=radius)
    diag = math.sqrt(1.0 + 0.25)
    assert [round(s["length_mm"], 9) for s in g["segments"]] == [round(2 * diag, 9), 1.5, round(2 * diag, 9)]
    assert g["segments"][1]["radius_mm"] == {"min": 1.0, "mean": 3.0, "max": 6.0} and g["spacing_mm"] == [2.0, 1.0, 0.5]
    assert json.loads(json.dumps(g)) == g


def test_graph_of_a_ring():
    ring = [(0, 2), (1, 1), (2, 0), (3, 1), (4, 2), (3, 3), (2, 4), (1, 3)]
    codes = codes_of(plane((5, 5), ring))
    assert (codes[codes > 0] == 3).all()
    g = sk.skeleton_graph(codes)
    assert g["junctions"] == [] and g["end_points"] == 0
    assert [brief(s) for s in g["segments"]] == [(8, round(8 * R2, 9), True, [None, None])]
    # a ring and a free rod: two segments
    both = plane((5, 9), ring + [(2, 6), (2, 7), (2, 8)])
    g = sk.skeleton_graph(codes_of(both))
    assert [brief(s) for s in g["segments"]] == [(8, round(8 * R2, 9), True, [None, None]), (3, 2.0, False, [None, None])]


def test_graph_of_two_junction_clusters_joined_directly():
    """An H: each T is a cluster of four junction voxels, and the bridge between them is ONE curve voxel that touches both."""
    bars = [(y, 1) for y in range(7)] + [(y, 5) for y in range(7)]
    m = plane((7, 7), bars + [(3, 2), (3, 3), (3, 4)])
    codes = codes_of(m)
    assert codes[2, 3, 3] == 3 and (codes >= 4).sum() == 8
    g = sk.skeleton_graph(codes)
    assert g["junctions"] == [{"id": 0, "voxels": 4, "index": (2 * 7 + 2) * 7 + 1}, {"id": 1, "voxels": 4, "index": (2 * 7 + 2) * 7 + 5}]
    assert [brief(s) for s in g["segments"]] == [(2, 1.0, False, [None, 0]), (2, 1.0, False, [None, 1]), (1, 0.0, False, [0, 1]),
                                                 (2, 1.0, False, [0, None]), (2, 1.0, False, [1, None])]
    assert g["end_points"] == 4


def test_graph_of_a_single_voxel_and_of_nothing():
    m = np.zeros((3, 4, 5), bool)
    m[1, 2, 3] = True
    g = sk.skeleton_graph(codes_of(m))
    assert g["voxels"] == 1 and g["isolated"] == 1 and g["junctions"] == [] and g["end_points"] == 0
    assert [brief(s) for s in g["segments"]] == [(1, 0.0, False, [None, None])]
    g = sk.skeleton_graph(np.zeros((3, 4, 5), np.uint8))
    assert g["voxels"] == 0 and g["segments"] == [] and g["junctions"] == []
    with pytest.raises(ValueError, match="3-D"):
        sk.skeleton_graph(np.zeros((4, 5), np.uint8))
    with pytest.raises(ValueError, match="spacing"):
        sk.skeleton_graph(codes_of(m), spacing=(1.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="radius"):
        sk.skeleton_graph(codes_of(m), radius=np.zeros((3, 4, 4)))


def test_graph_of_a_mask_skeletonises_first(emu_engine):
    m = np.zeros((7, 9, 20), bool)
    m[2:5, 3:6, 1:19] = True
    codes = sk.skeletonize(m, engine=emu_engine)
    assert np.array_equal(codes, oracle_skeleton(m.astype(np.uint8))[0])
    assert sk.skeleton_graph(m, engine=emu_engine) == sk.skeleton_graph(codes)
    out, info = sk.skeletonize(np.zeros((3, 4, 5), bool), engine=emu_engine, return_info=True)
    assert not out.any() and info == {"selected": 0, "skeleton": 0, "passes": 0}
    labels = np.where(m, 7, 0).astype(np.int16)
    assert np.array_equal(sk.skeletonize(labels, keep=(7,), engine=emu_engine), codes)
    assert not sk.skeletonize(labels, keep=(3,), engine=emu_engine).any()


# ---- vessel_tree ------------------------------------------------------------------------------------------------------------------------
def scene():
    """Two label blocks on lung-like noise with bright rods of two calibres that cross (junctions) and one apart."""
    rng = np.random.default_rng(3)
    x = rng.integers(-900, -800, SHAPE).astype(np.int16)
    lab = np.zeros(SHAPE, np.uint8)
    lab[1:11, 4:36, 4:24] = 1
    lab[1:11, 4:36, 24:44] = 2
    x[5:7, 19:22, :] = 100      # a rod along x through both labels
    x[:, 18:23, 12:16] = 100    # a thicker one along z in label 1 that crosses it
    x[4, 28, 26:40] = 100       # a thin one in label 2
    x[lab == 0] = 50            # chest wall
    return x, lab


def restated_tree(r, lab, calibres, sp, names):
    """The label entries of the tree from the result's own volumes, by the definitions."""
    skel, mask = r.skeleton, r.mask
    voxel_ml = None if sp is None else float(np.prod(sp)) / 1000.0
    step = [1.0, 1.0, 1.0] if sp is None else list(sp)
    first_label, lengths = {}, {}
    for what, sel in (("junctions", skel >= 4), ("segments", (skel > 0) & (skel < 4))):
        comp, count = ndi.label(sel, structure=S26)
        first_label[what] = [int(lab.ravel()[np.flatnonzero(comp.ravel() == i + 1)[0]]) for i in range(count)]
        if what == "segments":
            for i in range(count):  # every link between two voxels of the segment, once: the path, or the cycle with its closing link
                pts = np.argwhere(comp == i + 1)
                d = (pts[:, None, :] - pts[None, :, :])
                near = (np.abs(d).max(axis=2) == 1)
                lengths[i] = float((np.sqrt(((d * np.asarray(step)) ** 2).sum(axis=2)) * near).sum() / 2)
    out = {}
    for k in sorted(names):
        own = mask & (lab == k)
        if not own.any():
            out[str(k)] = None
            continue
        segs = [i for i, l in enumerate(first_label["segments"]) if l == k]
        out[str(k)] = {"vessel_voxels": int(own.sum()), "skeleton_voxels": int(((skel > 0) & (lab == k)).sum()), "segments": len(segs),
                       "length_mm": sum(lengths[i] for i in segs), "junctions": first_label["junctions"].count(k),
                       "ends": int(((skel == 2) & (lab == k)).sum()),
                       "by_calibre": [int(((r.calibre == c) & (lab == k)).sum()) for c in range(1, len(calibres) + 2)]}
    return out, voxel_ml


@pytest.mark.parametrize("sp", [SP, None])
def test_tree_against_numpy(emu_engine, sp):
    x, lab = scene()
    names = {1: "right lung", 2: "left lung", 3: "spare"}
    calibres = (3.0, 8.0)
    kw = dict(sigmas_mm=(1.0, 1.5), threshold=0.4, erode_mm=2.0, spacing=sp, names=names, engine=emu_engine)
    r = sk.vessel_tree(x, lab, calibres_mm2=calibres, **kw)
    base = vs.vessel_result(x, lab, **kw)  # vessel_result's fields are what they were
    assert_same_bits(r.vesselness, base.vesselness)
    assert np.array_equal(r.scale, base.scale) and np.array_equal(r.mask, base.mask) and r.analysis == base.analysis
    assert r.mask.sum() > 100
    # the skeleton and the classes by their definitions
    assert np.array_equal(r.skeleton, oracle_skeleton(r.mask.astype(np.uint8))[0]) and (r.skeleton >= 4).any()
    edges = [math.sqrt(a / math.pi) for a in calibres]
    want_cls, counts, d2 = oracle_calibre(r.skeleton, r.mask.astype(np.uint8), edges, sp, None, lab, 16)
    assert np.array_equal(r.calibre, want_cls) and len(np.unique(want_cls)) >= 3
    t = r.tree
    assert t["calibres_mm2"] == list(calibres) and t["edges_mm"] == edges and t["spacing_mm"] == (None if sp is None else list(sp))
    want, voxel_ml = restated_tree(r, lab, calibres, sp, names)
    assert t["voxel_volume_ml"] == voxel_ml and sorted(t["labels"]) == ["1", "2", "3"]
    for k, entry in t["labels"].items():
        assert entry["name"] == names[int(k)]
        if want[k] is None:
            assert entry["vessel_voxels"] == 0 and all(entry[f] is None for f in ("skeleton_voxels", "segments", "length_mm", "junctions",
                                                                                 "ends", "by_calibre"))
            continue
        for f in ("vessel_voxels", "skeleton_voxels", "segments", "junctions", "ends"):
            assert entry[f] == want[k][f], (k, f, entry[f], want[k][f])
        assert entry["length_mm"] == pytest.approx(want[k]["length_mm"], rel=1e-12)
        assert [c["class"] for c in entry["by_calibre"]] == [1, 2, 3]
        assert [c["voxels"] for c in entry["by_calibre"]] == want[k]["by_calibre"] == [int(v) for v in counts[int(k), 1:4]]
        assert [c["ml"] for c in entry["by_calibre"]] == [None if voxel_ml is None else v * voxel_ml for v in want[k]["by_calibre"]]
    lung = t["lung"]
    for f in ("vessel_voxels", "skeleton_voxels", "segments", "junctions", "ends"):
        assert lung[f] == sum(want[k][f] for k in ("1", "2")), f
    assert lung["length_mm"] == pytest.approx(sum(s["length_mm"] for s in t["graph"]["segments"]))
    assert lung["vessel_voxels"] == int(r.mask.sum()) == sum(c["voxels"] for c in lung["by_calibre"])
    # the graph carries the radii: sqrt of the squared distances at the segment's voxels
    g = sk.skeleton_graph(r.skeleton, spacing=sp, radius=np.sqrt(d2.astype(np.float64)))
    assert t["graph"] == g and any(s["radius_mm"]["max"] > s["radius_mm"]["min"] for s in g["segments"])
    assert json.loads(json.dumps(t)) == t
    # without names: the labels that hold a vessel voxel, with default names
    r2 = sk.vessel_tree(x, lab, calibres_mm2=calibres, **dict(kw, names=None))
    assert sorted(r2.tree["labels"]) == ["1", "2"] and r2.tree["labels"]["1"]["name"] == "label 1"
    assert r2.tree["lung"] == t["lung"]


def test_tree_inputs_and_empties(emu_engine):
    x, lab = scene()
    img = volume_io.Volume(x, SP[::-1], (1.0, 2.0, 3.0))
    kw = dict(sigmas_mm=(1.0, 1.5), threshold=0.4, engine=emu_engine)
    a = sk.vessel_tree(img, lab, **kw)  # the image's own spacing
    b = sk.vessel_tree(x, lab, spacing=SP, **kw)
    assert a.tree == b.tree and np.array_equal(a.skeleton, b.skeleton) and np.array_equal(a.calibre, b.calibre)
    assert a.tree["calibres_mm2"] == [5.0, 10.0]
    empty = sk.vessel_tree(x, np.zeros_like(lab), names={1: "right lung"}, spacing=SP, **kw)
    assert not empty.skeleton.any() and not empty.calibre.any() and empty.tree["lung"]["vessel_voxels"] == 0
    assert empty.tree["labels"]["1"]["segments"] is None and empty.tree["graph"]["segments"] == []
    assert empty.analysis == vs.vessel_result(x, np.zeros_like(lab), names={1: "right lung"}, spacing=SP, **kw).analysis
    none = sk.vessel_tree(x, lab, spacing=SP, **dict(kw, threshold=1e9))  # labels, but no vessel voxel
    assert not none.mask.any() and not none.skeleton.any() and none.tree["lung"]["vessel_voxels"] == 0
    assert json.loads(json.dumps(none.tree)) == none.tree
    for bad in ((), (10.0, 5.0), (5.0, 5.0), (0.0,), (-1.0,), (float("nan"),), tuple(range(1, 9))):
        with pytest.raises(ValueError, match="calibres_mm2"):
            sk.vessel_tree(x, lab, calibres_mm2=bad, **kw)
    with pytest.raises(ValueError, match="labels"):
        sk.vessel_tree(x, None, **kw)
    with pytest.raises(ValueError, match="threshold"):
        sk.vessel_tree(x, lab, **dict(kw, threshold=0.0))


def test_apply_with_vessel_tree_on_the_emulator(emu_engine, monkeypatch):
    """LMInferer.apply_with_vessel_tree around fixed labels (test_mask_wrappers_emu's harness): the device branch, the host detour and
    the empty case."""
    from tests.test_mask_wrappers_emu import IMAGE, LABELS, NAMES, NO_LABELS, SPACING, Harness, forms

    kw = dict(sigmas_mm=(0.6, 1.0), threshold=0.3, erode_mm=0.5, calibres_mm2=(2.0, 6.0))
    lung = Harness(emu_engine, LABELS)
    try:
        for detour in (False, True):
            if detour:
                monkeypatch.setattr(lung.inf, "_on_host", lambda arr: True)
            for name, (image, sp) in forms(IMAGE).items():
                labels, res = lung.inf.apply_with_vessel_tree(image, spacing=sp, **kw)
                arr = image if isinstance(image, np.ndarray) else np.asarray(image.array)
                asp = sp if sp is not None else tuple(image.spacing[::-1])
                want = sk.vessel_tree(arr, LABELS, spacing=asp, names=NAMES, engine=emu_engine, **kw)
                assert np.array_equal(labels, LABELS) and res.tree == want.tree and res.analysis == want.analysis, name
                assert np.array_equal(res.skeleton, want.skeleton) and np.array_equal(res.calibre, want.calibre)
                assert np.array_equal(res.mask, want.mask)
                assert_same_bits(res.vesselness, want.vesselness)
        with pytest.raises(ValueError, match="calibres_mm2"):
            lung.inf.apply_with_vessel_tree(IMAGE, calibres_mm2=(3.0, 2.0))
    finally:
        lung.inf.close()
    empty = Harness(emu_engine, NO_LABELS)
    try:
        labels, res = empty.inf.apply_with_vessel_tree(IMAGE, spacing=SPACING, **kw)
        assert not labels.any() and not res.skeleton.any() and res.tree["lung"]["vessel_voxels"] == 0
        assert res.tree == sk.vessel_tree(IMAGE, NO_LABELS, spacing=SPACING, names=NAMES, engine=emu_engine, **kw).tree
    finally:
        empty.inf.close()


def test_cli_vessel_tree(emu_engine, tmp_path, monkeypatch):
    import lungmask_amd.__main__ as cli
    from lungmask_amd import stats as lmstats

    x, lab = scene()
    img = volume_io.Volume(x, SP[::-1], (1.0, 2.0, 3.0))
    ip = tmp_path / "in.nii.gz"
    volume_io.write_nifti(str(ip), img)
    FakeInferer.engine, FakeInferer.labels = emu_engine, lab
    monkeypatch.setattr(cli, "LMInferer", FakeInferer)
    monkeypatch.setattr(emu_engine, "n_classes", lambda slot: 3, raising=False)  # (no model is loaded into the emulated engine)
    loaded = volume_io.load_input_image(str(ip))
    names = lmstats.label_names("R231", 3)
    t = lambda name: str(tmp_path / name)  # noqa: E731
    common = ["--vessel-sigmas", "1", "1.5", "--vessel-threshold", "0.4"]
    assert cli.main([str(ip), t("o.npy"), "--noprogress", "--vessel-skeleton", t("k.npy"), "--vessel-calibre", t("c.nii.gz"),
                     "--vessel-tree", t("t.json"), "--vessel-mask", t("m.npy"), "--vessels", t("v.json")] + common) == 0
    want = sk.vessel_tree(loaded, lab, sigmas_mm=(1.0, 1.5), threshold=0.4, names=names, engine=emu_engine)
    assert np.array_equal(np.load(t("o.npy")), lab) and want.skeleton.any()
    k = np.load(t("k.npy"))
    assert k.dtype == np.uint8 and np.array_equal(k, want.skeleton)
    c = volume_io.load_input_image(t("c.nii.gz"))
    assert np.array_equal(np.asarray(c.array), want.calibre)
    np.testing.assert_allclose(c.spacing, loaded.spacing, atol=1e-6)
    assert json.load(open(t("t.json"))) == json.loads(json.dumps(want.tree))
    assert json.load(open(t("v.json"))) == json.loads(json.dumps(want.analysis))
    assert np.array_equal(np.load(t("m.npy")).astype(bool), want.mask)
    # other calibres, beside --stats (another apply_* method labels; the tree comes from its labels)
    assert cli.main([str(ip), t("o2.npy"), "--noprogress", "--stats", t("s.json"), "--vessel-tree", t("t2.json"), "--vessel-calibres", "2", "4",
                     "9"] + common) == 0
    want2 = sk.vessel_tree(loaded, lab, sigmas_mm=(1.0, 1.5), threshold=0.4, calibres_mm2=(2.0, 4.0, 9.0), names=names, engine=emu_engine)
    assert json.load(open(t("t2.json"))) == json.loads(json.dumps(want2.tree)) and len(want2.tree["lung"]["by_calibre"]) == 4
    assert "labels" in json.load(open(t("s.json")))
    # without the new flags the vessel outputs are what they were
    assert cli.main([str(ip), t("o3.npy"), "--noprogress", "--vessels", t("v3.json")] + common) == 0
    assert json.load(open(t("v3.json"))) == json.loads(json.dumps(want.analysis))
    # no labelled voxel
    FakeInferer.labels = np.zeros_like(lab)
    assert cli.main([str(ip), t("o4.npy"), "--noprogress", "--vessel-skeleton", t("k4.npy"), "--vessel-tree", t("t4.json")]) == 0
    assert not np.load(t("k4.npy")).any() and json.load(open(t("t4.json")))["lung"]["vessel_voxels"] == 0
    for bad in (["--vessel-calibres", "5"], ["--vessel-tree", "t.txt"], ["--vessel-skeleton", "k.txt"], ["--vessel-calibre", "c.json"],
                ["--vessel-tree", "t.json", "--vessel-calibres", "10", "5"], ["--vessel-tree", "t.json", "--vessel-calibres", "0"],
                ["--vessel-tree", "t.json", "--vessel-calibres"] + ["1"] * 8, ["--vessel-tree", "t.json", "--vessel-sigmas", "-1"]):
        with pytest.raises(SystemExit, match="--vessel"):  # refused before anything is loaded
            cli.main([str(ip), t("o5.npy")] + bad)
