"""lungmask_amd.vessels on the emulator engine: argument checking, the analysis dict against a numpy restatement, the JSON round trip,
empty labels, and the inputs that bring their own spacing."""
import json

import numpy as np
import pytest

from lungmask_amd import vessels as vs
from lungmask_amd import volume_io
from tests.cli_fake import FakeInferer
from tests.test_filters_emu import assert_same_bits
from tests.test_vessels_emu import oracle_vesselness

SHAPE = (12, 40, 48)
SP = (2.0, 1.0, 0.8)


def scene():
    """Two label blocks with bright rods of two calibres on lung-like noise."""
    rng = np.random.default_rng(3)
    x = rng.integers(-900, -800, SHAPE).astype(np.int16)
    lab = np.zeros(SHAPE, np.uint8)
    lab[1:11, 4:36, 4:24] = 1
    lab[1:11, 4:36, 24:44] = 2
    x[5:7, 19:22, :] = 100     # a rod along x through both labels
    x[:, 9:12, 12:15] = 100    # a thicker one along z in label 1
    x[lab == 0] = 50           # chest wall
    return x, lab


def test_argument_checking(emu_engine):
    x, lab = scene()
    with pytest.raises(ValueError, match="limit is 32"):
        vs.vesselness(x, sigmas_mm=(1.0, 9.0), engine=emu_engine)
    with pytest.raises(ValueError, match="limit is 32"):
        vs.hessian(x, 3.0, spacing=(1.0, 1.0, 0.3), engine=emu_engine)
    with pytest.raises(ValueError, match="same shape"):
        vs.vesselness(x, labels=lab[:, :, :-1], engine=emu_engine)
    with pytest.raises(ValueError, match="same shape"):
        vs.vessel_analysis(x, lab[1:], engine=emu_engine)
    img = volume_io.Volume(x, SP[::-1], (0.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="spacing"):
        vs.vesselness(img, spacing=SP, engine=emu_engine)
    with pytest.raises(ValueError, match="spacing"):
        vs.vessel_analysis(img, lab, spacing=SP, engine=emu_engine)
    with pytest.raises(ValueError, match="spacing"):
        vs.vesselness(x, spacing=(1.0, 0.0, 1.0), engine=emu_engine)
    with pytest.raises(ValueError, match="between 1 and 8"):
        vs.vesselness(x, sigmas_mm=[1.0] * 9, engine=emu_engine)
    with pytest.raises(ValueError, match="sigma"):
        vs.vesselness(x, sigmas_mm=(1.0, -1.0), engine=emu_engine)
    with pytest.raises(ValueError, match="one scale"):
        vs.hessian(x, (1.0, 2.0), engine=emu_engine)
    with pytest.raises(ValueError, match="beta"):
        vs.vesselness(x, beta=float("nan"), engine=emu_engine)
    with pytest.raises(ValueError, match="threshold"):
        vs.vessel_analysis(x, lab, threshold=0.0, engine=emu_engine)
    with pytest.raises(ValueError, match="erode_mm"):
        vs.vessel_analysis(x, lab, erode_mm=-1.0, engine=emu_engine)
    with pytest.raises(ValueError, match="needs labels"):
        vs.vessel_analysis(x, None, engine=emu_engine)
    with pytest.raises(ValueError, match="no voxel"):
        vs.vesselness(x, labels=np.zeros_like(lab), engine=emu_engine)
    with pytest.raises(ValueError, match="3-D"):
        vs.vesselness(x[0], engine=emu_engine)


def test_module_equals_definition(emu_engine):
    x, lab = scene()
    sig = (1.0, 2.0)
    V, scale = vs.vesselness(x, sig, spacing=SP, labels=lab, return_scale=True, engine=emu_engine)
    want, want_scale = oracle_vesselness(x, [[s / v for v in SP] for s in sig], sel=lab > 0)
    assert_same_bits(V, want)
    assert_same_bits(scale, want_scale)
    assert (V[lab > 0] > 0.5).sum() > 20  # the rods are found
    img = volume_io.Volume(x, SP[::-1], (1.0, 2.0, 3.0))  # brings its spacing (x, y, z)
    assert_same_bits(vs.vesselness(img, sig, labels=lab, engine=emu_engine), V)
    comp, eig = vs.hessian(img, 1.0, eigenvalues=True, engine=emu_engine)
    assert comp.shape == (6,) + SHAPE and eig.shape == (3,) + SHAPE and (np.abs(eig[0]) <= np.abs(eig[2])).all()
    # uint8 input is widened, as everywhere
    assert_same_bits(vs.vesselness((x + 1000).clip(0, 255).astype(np.uint8), sig, engine=emu_engine),
                     vs.vesselness((x + 1000).clip(0, 255).astype(np.int32), sig, engine=emu_engine))


def restated_analysis(x, lab, sig, threshold, erode_mm, sp, engine, names):
    V, scale = vs.vesselness(x, sig, spacing=sp, labels=lab, return_scale=True, engine=engine)
    eroded = engine.morph(lab, "erode", erode_mm, spacing=sp)[0]
    voxel_ml = None if sp is None else float(np.prod(sp)) / 1000.0
    hit = V >= np.float32(threshold)

    def entry(name, region):
        n = int(region.sum())
        if n == 0:
            return {"name": name, "voxels": 0, "vessel_voxels": None, "vessel_ml": None, "fraction": None, "by_scale": None}
        k = int((hit & region).sum())
        return {"name": name, "voxels": n, "vessel_voxels": k, "vessel_ml": None if voxel_ml is None else k * voxel_ml, "fraction": k / n,
                "by_scale": [int((hit & region & (scale == i + 1)).sum()) for i in range(len(sig))]}

    labels = {str(k): entry(names.get(k, f"label {k}"), eroded == k) for k in sorted(set(names) | set(np.unique(eroded[eroded > 0]).tolist()))}
    return V, scale, hit & (eroded > 0), labels, entry("lung", eroded > 0)


@pytest.mark.parametrize("sp", [SP, None])
def test_analysis_against_numpy(emu_engine, sp):
    x, lab = scene()
    lab[5, 20, 30] = 7  # a label without a name
    sig, names = (1.0, 1.5, 2.0), {1: "right lung", 2: "left lung", 3: "nothing"}
    a = vs.vessel_analysis(x, lab, sig, threshold=0.4, erode_mm=2.0, spacing=sp, names=names, engine=emu_engine)
    V, scale, mask, labels, lung = restated_analysis(x, lab, sig, 0.4, 2.0, sp, emu_engine, names)
    assert a["labels"] == labels and a["lung"] == lung
    assert a["sigmas_mm"] == [1.0, 1.5, 2.0] and a["threshold"] == 0.4 and a["erode_mm"] == 2.0
    assert a["spacing_mm"] == (None if sp is None else list(sp)) and (a["voxel_volume_ml"] is None) == (sp is None)
    assert a["lung"]["vessel_voxels"] > 20 and a["lung"]["voxels"] < int((lab > 0).sum())  # something is found; the erosion bites
    assert a["labels"]["3"]["voxels"] == 0 and a["labels"]["3"]["fraction"] is None and a["labels"]["3"]["by_scale"] is None
    assert sum(a["lung"]["by_scale"]) == a["lung"]["vessel_voxels"] == sum(e["vessel_voxels"] or 0 for e in a["labels"].values())
    assert json.loads(json.dumps(a)) == a  # JSON round trip
    r = vs.vessel_result(x, lab, sig, threshold=0.4, erode_mm=2.0, spacing=sp, names=names, engine=emu_engine)
    assert r.analysis == a and np.array_equal(r.mask, mask) and r.mask.dtype == bool
    assert_same_bits(r.vesselness, V)
    assert_same_bits(r.scale, scale)
    # without erosion the pleural voxels take part
    a0 = vs.vessel_analysis(x, lab, sig, threshold=0.4, erode_mm=0.0, spacing=sp, names=names, engine=emu_engine)
    assert a0["lung"]["voxels"] == int((lab > 0).sum())


def test_empty_labels(emu_engine):
    x, lab = scene()
    a = vs.vessel_analysis(x, np.zeros_like(lab), names={1: "right lung"}, spacing=SP, engine=emu_engine)
    assert a["lung"] == {"name": "lung", "voxels": 0, "vessel_voxels": None, "vessel_ml": None, "fraction": None, "by_scale": None}
    assert a["labels"] == {"1": dict(a["lung"], name="right lung")} and json.loads(json.dumps(a)) == a
    r = vs.vessel_result(x, np.zeros_like(lab), engine=emu_engine)
    assert not r.vesselness.any() and not r.scale.any() and not r.mask.any() and r.vesselness.dtype == np.float32
    assert r.analysis["lung"]["voxels"] == 0
    tiny = np.zeros(SHAPE, np.uint8)
    tiny[5, 20, 20] = 1  # the erosion removes everything: the label is empty, nothing fails
    a = vs.vessel_analysis(x, tiny, spacing=SP, engine=emu_engine)
    assert a["lung"]["voxels"] == 0 and a["lung"]["fraction"] is None


def test_apply_with_vessels_on_the_emulator(emu_engine, monkeypatch):
    """LMInferer.apply_with_vessels around fixed labels (test_mask_wrappers_emu's harness): the device branch, the host detour and
    the empty case, in the three input forms."""
    from tests.test_mask_wrappers_emu import IMAGE, LABELS, NAMES, NO_LABELS, SPACING, Harness, forms

    kw = dict(sigmas_mm=(0.6, 1.0), threshold=0.3, erode_mm=0.5)
    lung = Harness(emu_engine, LABELS)
    try:
        for detour in (False, True):
            if detour:
                monkeypatch.setattr(lung.inf, "_on_host", lambda arr: True)
            for name, (image, sp) in forms(IMAGE).items():
                labels, res = lung.inf.apply_with_vessels(image, spacing=sp, **kw)
                arr = image if isinstance(image, np.ndarray) else np.asarray(image.array)
                asp = sp if sp is not None else tuple(image.spacing[::-1])
                want = vs.vessel_result(arr, LABELS, spacing=asp, names=NAMES, engine=emu_engine, **kw)
                assert np.array_equal(labels, LABELS) and res.analysis == want.analysis and np.array_equal(res.mask, want.mask), name
                assert_same_bits(res.vesselness, want.vesselness)
                assert_same_bits(res.vesselness, vs.vesselness(arr, kw["sigmas_mm"], spacing=asp, labels=LABELS, engine=emu_engine))
                assert_same_bits(res.scale, want.scale)
        with pytest.raises(ValueError, match="limit is 32"):
            lung.inf.apply_with_vessels(IMAGE, sigmas_mm=(9.0,))
        with pytest.raises(ValueError, match="threshold"):
            lung.inf.apply_with_vessels(IMAGE, threshold=-1)
    finally:
        lung.inf.close()
    empty = Harness(emu_engine, NO_LABELS)
    try:
        labels, res = empty.inf.apply_with_vessels(IMAGE, spacing=SPACING, **kw)
        want = vs.vessel_result(IMAGE, NO_LABELS, spacing=SPACING, names=NAMES, engine=emu_engine, **kw)
        assert not labels.any() and not res.vesselness.any() and not res.mask.any() and res.analysis == want.analysis
        assert res.analysis["lung"]["voxels"] == 0 and res.analysis["labels"]["1"]["fraction"] is None
    finally:
        empty.inf.close()


def test_cli_vessels(emu_engine, tmp_path, monkeypatch):
    import lungmask_amd.__main__ as cli
    from lungmask_amd import filters as flt
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
    assert cli.main([str(ip), t("o.npy"), "--noprogress", "--vesselness", t("v.npy"), "--vessel-mask", t("m.nii.gz"), "--vessels", t("v.json")]) == 0
    want = vs.vessel_result(loaded, lab, names=names, engine=emu_engine)
    assert np.array_equal(np.load(t("o.npy")), lab)
    assert_same_bits(np.load(t("v.npy")), want.vesselness)
    m = volume_io.load_input_image(t("m.nii.gz"))
    assert np.array_equal(np.asarray(m.array) != 0, want.mask) and want.mask.any()
    np.testing.assert_allclose(m.spacing, loaded.spacing, atol=1e-6)
    assert json.load(open(t("v.json"))) == json.loads(json.dumps(want.analysis))
    # other scales and threshold, beside --stats (another apply_* method labels; the vessels come from its labels)
    assert cli.main([str(ip), t("o2.npy"), "--noprogress", "--stats", t("s.json"), "--vessels", t("v2.json"), "--vessel-sigmas", "1", "2.5",
                     "--vessel-threshold", "0.3"]) == 0
    want2 = vs.vessel_analysis(loaded, lab, (1.0, 2.5), threshold=0.3, names=names, engine=emu_engine)
    assert json.load(open(t("v2.json"))) == json.loads(json.dumps(want2))
    assert json.load(open(t("s.json"))) == json.loads(json.dumps(lmstats.label_statistics(loaded, lab, names=names, engine=emu_engine, n_labels=3)))
    # after --denoise the vessel filter reads the filtered image and the JSON names it
    assert cli.main([str(ip), t("o3.npy"), "--noprogress", "--denoise", "median", "--vessels", t("v3.json"), "--vesselness", t("v3.npy")]) == 0
    filtered = flt.median(loaded, 3, labels=lab, engine=emu_engine)
    want3 = vs.vessel_result(loaded.like(filtered), lab, names=names, engine=emu_engine)
    assert json.load(open(t("v3.json"))) == json.loads(json.dumps(dict(want3.analysis, denoise={"method": "median", "size": 3, "masked": True})))
    assert_same_bits(np.load(t("v3.npy")), want3.vesselness)
    # no labelled voxel
    FakeInferer.labels = np.zeros_like(lab)
    assert cli.main([str(ip), t("o4.npy"), "--noprogress", "--vesselness", t("v4.npy"), "--vessels", t("v4.json")]) == 0
    assert not np.load(t("v4.npy")).any() and json.load(open(t("v4.json")))["lung"]["voxels"] == 0
    for bad in (["--vessel-threshold", "0.4"], ["--vessel-sigmas", "1"], ["--vessels", "v.txt"], ["--vesselness", "v.txt"],
                ["--vessels", "v.json", "--vessel-sigmas", "-1"], ["--vessels", "v.json", "--vessel-threshold", "0"],
                ["--vessels", "v.json", "--vessel-sigmas"] + ["1"] * 9):
        with pytest.raises(SystemExit, match="--vessel"):  # refused before anything is loaded
            cli.main([str(ip), t("o5.npy")] + bad)
