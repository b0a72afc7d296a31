"""What the command line refuses, with which text, before anything is loaded; and which `apply_*` call a set of flags selects,
with which keyword arguments (that one call is what keeps a run at one upload of the volume).  No GPU, no engine."""
import numpy as np
import pytest

import lungmask_amd.__main__ as cli
from lungmask_amd import volume_io

VOLUME_EXT = "(use .nii, .nii.gz, .mha, .mhd or .npy)"
FIELD_EXT = "(use .npz, .nii or .nii.gz)"
NEED_CLUSTERS = "--cluster-threshold HU, --cluster-connectivity N and --cluster-ids PATH need --clusters PATH.json"
NEED_VESSELS = ("--vessel-sigmas MM and --vessel-threshold T need --vesselness PATH, --vessel-mask PATH, --vessels PATH.json, "
                "--vessel-skeleton PATH, --vessel-calibre PATH or --vessel-tree PATH.json")
NEED_RESAMPLED = ("--resample-spacing MM, --resample-like IMAGE, --resample-order N and --resample-label-mode MODE need --resampled PATH "
                  "or --resampled-labels PATH")
NEED_MOVING = "--registered PATH, --registration PATH.json and --register-transform KIND need --register-moving IMAGE"
NEED_PAIR = "--pair-roles, --pair-thresholds and --pair-range need --pair PATH.json, --pair-classes PATH or --pair-change PATH"
PAIR_NEEDS_MOVING = "--pair PATH.json, --pair-classes PATH and --pair-change PATH need --register-moving IMAGE"
GO_TOGETHER = "--compare-to MASK and --metrics PATH.json go together"
DENOISE = "--denoise: median, median:3, median:5 or gaussian:MM with MM > 0, got "
MOVING = ["--register-moving", "{IN}"]
DEFORM = MOVING + ["--register-deformable"]

# (extra argv, the exact text of the exit): one fault per row.  {IN} is the input file, {MISSING} a path that does not exist.
REFUSALS = [
    (["--denoise", "mean"], DENOISE + "'mean'"),
    (["--denoise", "median:4"], DENOISE + "'median:4'"),
    (["--denoise", "gaussian:-1"], DENOISE + "'gaussian:-1'"),
    (["--probabilities", "p.mha"], "--probabilities: unsupported file type 'p.mha' (use .npy, .nii or .nii.gz)"),
    (["--probabilities", "p.npy", "--modelname", "LTRCLobes_R231"],
     "--probabilities is not available with --modelname LTRCLobes_R231: the fused mode has labels only "
     "(run LTRCLobes and R231 on their own for their probabilities)"),
    (["--stats", "s.txt"], "--stats: unsupported file type 's.txt' (use .json)"),
    (["--texture-bin-width", "10"], "--texture-bin-width HU and --texture-range LO HI need --texture PATH.json"),
    (["--texture-range", "0", "100"], "--texture-bin-width HU and --texture-range LO HI need --texture PATH.json"),
    (["--texture", "t.txt"], "--texture: unsupported file type 't.txt' (use .json)"),
    (["--texture", "t.json", "--texture-bin-width", "0"],
     "--texture: need lo <= hi (int32) and bin_width >= 1, got hu_range (-1000, 199), bin_width 0"),
    (["--texture", "t.json", "--texture-range", "-1000", "1000"],
     "--texture: 81 grey levels: (hi - lo) // bin_width + 1 must not exceed 64"),
    (["--compare-to", "{IN}"], GO_TOGETHER),
    (["--metrics", "m.json"], GO_TOGETHER),
    (["--compare-to", "{IN}", "--metrics", "m.txt"], "--metrics: unsupported file type 'm.txt' (use .json)"),
    (["--compare-to", "{MISSING}", "--metrics", "m.json"], "File not found: {MISSING}"),
    (["--roi", "r.txt"], "--roi: unsupported file type 'r.txt' " + VOLUME_EXT),
    (["--roi-spacing", "1"], "--roi-spacing MM needs --roi PATH"),
    (["--roi", "r.npy", "--roi-spacing", "0"], "--roi-spacing: a positive spacing in mm, got 0.0"),
    (["--mesh", "m.vtk"], "--mesh: unsupported file type 'm.vtk' (use .stl, .ply or .obj)"),
    (["--mesh-smooth", "3"], "--mesh-smooth N needs --mesh PATH"),
    (["--mesh", "m.obj", "--mesh-smooth", "-1"], "--mesh-smooth: a number of iterations in 0..100000, got -1"),
    (["--close-mm", "5"], "--close-mm MM needs --closed PATH"),
    (["--closed", "c.npy", "--close-mm", "-1"], "--close-mm: a radius in mm >= 0, got -1.0"),
    (["--cluster-threshold", "-900"], NEED_CLUSTERS),
    (["--cluster-connectivity", "26"], NEED_CLUSTERS),
    (["--cluster-ids", "i.npy"], NEED_CLUSTERS),
    (["--denoised", "d.npy"], "--denoised PATH needs --denoise METHOD"),
    (["--denoise", "median", "--denoised", "d.txt"], "--denoised: unsupported file type 'd.txt' " + VOLUME_EXT),
    (["--laa-map", "l.txt"], "--laa-map: unsupported file type 'l.txt' " + VOLUME_EXT),
    (["--laa-sigma", "2"], "--laa-sigma MM needs --laa-map PATH"),
    (["--laa-map", "l.npy", "--laa-sigma", "0"], "--laa-sigma: a sigma in mm > 0, got 0.0"),
    (["--clusters", "c.txt"], "--clusters: unsupported file type 'c.txt' (use .json)"),
    (["--clusters", "c.json", "--cluster-ids", "i.dcm"],
     "--cluster-ids: unsupported file type 'i.dcm' (use .npy, .nii, .nii.gz, .mha or .mhd)"),
    (["--clusters", "c.json", "--cluster-threshold", "2147483648"],
     "--cluster-threshold: an HU value in the int32 range, got 2147483648"),
    (["--vessel-calibres", "5"], "--vessel-calibres MM2 needs --vessel-skeleton PATH, --vessel-calibre PATH or --vessel-tree PATH.json"),
    (["--vessel-skeleton", "k.txt"], "--vessel-skeleton: unsupported file type 'k.txt' " + VOLUME_EXT),
    (["--vessel-calibre", "c.json"], "--vessel-calibre: unsupported file type 'c.json' " + VOLUME_EXT),
    (["--vessel-tree", "t.txt"], "--vessel-tree: unsupported file type 't.txt' (use .json)"),
    (["--vessel-tree", "t.json", "--vessel-calibres", "10", "5"],
     "--vessel-calibres: calibres_mm2: 1 to 7 strictly ascending areas > 0 in mm^2, got (10.0, 5.0)"),
    (["--vessel-sigmas", "1"], NEED_VESSELS),
    (["--vessel-threshold", "0.4"], NEED_VESSELS),
    (["--vesselness", "v.txt"], "--vesselness: unsupported file type 'v.txt' " + VOLUME_EXT),
    (["--vessel-mask", "m.txt"], "--vessel-mask: unsupported file type 'm.txt' " + VOLUME_EXT),
    (["--vessels", "v.txt"], "--vessels: unsupported file type 'v.txt' (use .json)"),
    (["--vessels", "v.json", "--vessel-sigmas", "-1"],
     "--vessel-sigmas / --vessel-threshold: sigmas_mm: every sigma must be one value > 0 and finite, got -1.0"),
    (["--vessels", "v.json", "--vessel-threshold", "0"],
     "--vessel-sigmas / --vessel-threshold: threshold must be > 0 and finite, got 0.0"),
    (["--resample-spacing", "2"], NEED_RESAMPLED),
    (["--resample-like", "{IN}"], NEED_RESAMPLED),
    (["--resample-order", "1"], NEED_RESAMPLED),
    (["--resample-label-mode", "nearest"], NEED_RESAMPLED),
    (["--resampled", "r.txt"], "--resampled: unsupported file type 'r.txt' " + VOLUME_EXT),
    (["--resampled-labels", "r.txt"], "--resampled-labels: unsupported file type 'r.txt' " + VOLUME_EXT),
    (["--resampled", "r.npy", "--resample-spacing", "2", "--resample-like", "{IN}"],
     "--resample-spacing MM and --resample-like IMAGE exclude each other"),
    (["--resampled", "r.npy", "--resample-spacing", "1", "2"],
     "--resample-spacing: one positive spacing in mm or three (x y z), got [1.0, 2.0]"),
    (["--resampled", "r.npy", "--resample-spacing", "0"],
     "--resample-spacing: one positive spacing in mm or three (x y z), got [0.0]"),
    (["--resampled", "r.npy", "--resample-like", "{MISSING}"], "File not found: {MISSING}"),
    (["--compare-resample"], "--compare-resample needs --compare-to MASK"),
    (["--registered", "r.npy"], NEED_MOVING),
    (["--registration", "t.json"], NEED_MOVING),
    (["--register-transform", "affine"], NEED_MOVING),
    (MOVING + ["--deformation", "d.npz"], "--deformation PATH and --jacobian PATH need --register-deformable"),
    (MOVING + ["--jacobian", "j.npy"], "--deformation PATH and --jacobian PATH need --register-deformable"),
    (MOVING + ["--inverse-deformation", "i.npz"], "--inverse-deformation PATH and --labels-on-moving PATH need --register-deformable"),
    (MOVING + ["--labels-on-moving", "l.npy"], "--inverse-deformation PATH and --labels-on-moving PATH need --register-deformable"),
    (["--register-deformable"], "--register-deformable needs --register-moving IMAGE"),
    (MOVING + ["--registration", "t.json", "--pair-roles", "longitudinal"], NEED_PAIR),
    (MOVING + ["--registration", "t.json", "--pair-thresholds", "-950", "-856"], NEED_PAIR),
    (MOVING + ["--registration", "t.json", "--pair-range", "-1000", "-500"], NEED_PAIR),
    (["--pair", "p.json"], PAIR_NEEDS_MOVING),
    (["--pair-classes", "c.npy"], PAIR_NEEDS_MOVING),
    (["--pair-change", "c.npy"], PAIR_NEEDS_MOVING),
    (MOVING, "--register-moving IMAGE needs --registered PATH or --registration PATH.json"),
    (MOVING + ["--pair", "p.txt"], "--pair: unsupported file type 'p.txt' (use .json)"),
    (MOVING + ["--pair-classes", "c.txt"], "--pair-classes: unsupported file type 'c.txt' " + VOLUME_EXT),
    (MOVING + ["--pair-change", "c.txt"], "--pair-change: unsupported file type 'c.txt' " + VOLUME_EXT),
    (MOVING + ["--pair", "p.json", "--pair-range", "-500", "-1000"], "--pair: hu_range: finite lo <= hi, got (-500.0, -1000.0)"),
    (DEFORM + ["--inverse-deformation", "i.txt"], "--inverse-deformation: unsupported file type 'i.txt' " + FIELD_EXT),
    (DEFORM + ["--labels-on-moving", "l.txt"], "--labels-on-moving: unsupported file type 'l.txt' " + VOLUME_EXT),
    (DEFORM + ["--deformation", "d.txt"], "--deformation: unsupported file type 'd.txt' " + FIELD_EXT),
    (DEFORM + ["--jacobian", "j.txt"], "--jacobian: unsupported file type 'j.txt' " + VOLUME_EXT),
    (MOVING + ["--registered", "r.txt"], "--registered: unsupported file type 'r.txt' " + VOLUME_EXT),
    (MOVING + ["--registration", "t.txt"], "--registration: unsupported file type 't.txt' (use .json)"),
    (["--register-moving", "{MISSING}", "--registration", "t.json"], "File not found: {MISSING}"),
]

# these pass every check and go on to load the input
ACCEPTED = [
    ["--cluster-threshold", "-900", "--laa-map", "l.npy"],
    ["--roi", "r.npy"],
    MOVING + ["--registration", "t.json"],
]


class Loaded(Exception):
    """Raised by what stands in for the loader and for LMInferer: the checks have let the run through."""


@pytest.fixture
def paths(tmp_path, monkeypatch):
    src = tmp_path / "in.npy"
    np.save(src, np.zeros((1, 16, 16), np.int16))

    def loaded(*a, **kw):
        raise Loaded

    monkeypatch.setattr(cli, "LMInferer", loaded)
    monkeypatch.setattr(volume_io, "load_input_image", loaded)
    return dict(IN=str(src), MISSING=str(tmp_path / "missing.npy"))


@pytest.mark.parametrize("extra, text", REFUSALS, ids=lambda v: " ".join(v) if isinstance(v, list) else None)
def test_refused_before_anything_is_loaded(paths, extra, text):
    with pytest.raises(SystemExit) as e:
        cli.main([paths["IN"], "o.npy"] + [a.format(**paths) for a in extra])
    assert e.value.code == text.format(**paths)


def test_missing_input_is_refused(paths):
    with pytest.raises(SystemExit) as e:
        cli.main([paths["MISSING"], "o.npy"])
    assert e.value.code == f"File not found: {paths['MISSING']}"


@pytest.mark.parametrize("extra", ACCEPTED, ids=" ".join)
def test_accepted_reaches_the_loader(paths, extra):
    with pytest.raises(Loaded):
        cli.main([paths["IN"], "o.npy"] + [a.format(**paths) for a in extra])


class Called(Exception):
    """Carries (method name, positional arguments, keyword arguments) of the one apply* call out of main()."""


class Recorder:
    """Stands in for LMInferer: the constructor records its keyword arguments, every apply* method raises `Called`."""
    engine = None
    modelname = "R231"
    made = None

    def __init__(self, *a, **kw):
        assert not a
        Recorder.made = kw

    def __getattr__(self, name):
        if not name.startswith("apply"):
            raise AttributeError(name)

        def call(*a, **kw):
            raise Called(name, a, kw)

        return call


MADE = dict(modelname="R231", modelpath=None, force_cpu=False, batch_size=20, volume_postprocessing=True, tqdm_disable=False)
VESSEL_KW = dict(sigmas_mm=(1.0, 1.5, 2.0, 3.0), threshold=0.5)
PAIR_KW = dict(deformable=False, transform="rigid", roles=("inspiration", "expiration"), maps=("classes", "change"))

# (extra argv, the method that gets the volume, how many images it takes, its keyword arguments): the 15 rungs in their order,
# then the pairs whose order matters
LADDER = [
    (["--denoise", "gaussian:1.5"], "apply_denoised", 1, dict(method="gaussian", sigma_mm=1.5)),
    (["--probabilities", "p.npy"], "apply_probabilities", 1, {}),
    (["--stats", "s.json"], "apply_with_stats", 1, {}),
    (["--texture", "t.json", "--texture-bin-width", "50"], "apply_with_texture", 1, dict(hu_range=(-1000, 199), bin_width=50)),
    (["--roi", "r.npy", "--roi-spacing", "1.5"], "apply_roi", 1, dict(spacing_out=1.5)),
    (["--mesh", "m_{label}.ply", "--mesh-smooth", "2"], "apply_mesh", 1, dict(per_label=True, smooth=2)),
    (["--closed", "c.npy"], "apply_closed", 1, dict(radius_mm=10.0)),
    (["--clusters", "c.json", "--cluster-connectivity", "26"], "apply_with_clusters", 1, dict(threshold=-950, connectivity=26)),
    (["--vessel-tree", "t.json"], "apply_with_vessel_tree", 1, dict(calibres_mm2=(5.0, 10.0), **VESSEL_KW)),
    (["--vessels", "v.json", "--vessel-threshold", "0.4"], "apply_with_vessels", 1, dict(VESSEL_KW, threshold=0.4)),
    (["--resampled", "r.npy", "--resample-spacing", "1", "2", "3"], "apply_resampled", 1,
     dict(order=3, label_mode="linear", spacing_out=(3.0, 2.0, 1.0))),
    (MOVING + ["--pair", "p.json", "--pair-thresholds", "-940", "-850"], "apply_pair", 2,
     dict(PAIR_KW, fixed_threshold=-940.0, moving_threshold=-850.0)),
    (DEFORM + ["--deformation", "d.npz"], "apply_deformable", 2, dict(transform="rigid", inverse=False)),
    (MOVING + ["--registered", "r.npy", "--register-transform", "affine"], "apply_registered", 2, dict(transform="affine")),
    ([], "apply", 1, {}),
    (["--denoise", "median", "--probabilities", "p.npy"], "apply_probabilities", 1, {}),
    (["--denoise", "median:5", "--stats", "s.json"], "apply_denoised", 1, dict(method="median", size=5)),
    (["--probabilities", "p.npy", "--stats", "s.json"], "apply_probabilities", 1, {}),
    (["--stats", "s.json", "--texture", "t.json"], "apply_with_stats", 1, {}),
    (["--mesh", "m.stl", "--closed", "c.npy"], "apply_mesh", 1, dict(per_label=False, smooth=0)),
    (["--vessels", "v.json", "--vessel-skeleton", "k.npy"], "apply_with_vessel_tree", 1, dict(calibres_mm2=(5.0, 10.0), **VESSEL_KW)),
    (DEFORM + ["--pair", "p.json", "--pair-roles", "longitudinal"], "apply_pair", 2, dict(PAIR_KW, deformable=True, roles=None)),
    (DEFORM + ["--pair", "p.json", "--inverse-deformation", "i.npz"], "apply_deformable", 2, dict(transform="rigid", inverse=True)),
]


@pytest.fixture
def recorder(tmp_path, monkeypatch):
    src = tmp_path / "in.npy"
    np.save(src, np.zeros((1, 16, 16), np.int16))
    monkeypatch.setattr(cli, "LMInferer", Recorder)
    return str(src)


@pytest.mark.parametrize("extra, method, n_images, kwargs", LADDER, ids=lambda v: " ".join(v) if isinstance(v, list) else None)
def test_flags_select_one_apply_call(recorder, extra, method, n_images, kwargs):
    with pytest.raises(Called) as e:
        cli.main([recorder, "o.npy", "--noprogress"] + [a.format(IN=recorder, label="{label}") for a in extra])
    name, images, kw = e.value.args
    assert (name, kw) == (method, kwargs)
    assert len(images) == n_images and all(isinstance(v, volume_io.Volume) and v.array.shape == (1, 16, 16) for v in images)
    assert Recorder.made == dict(MADE, tqdm_disable=True)


def test_fused_model_is_two_models(recorder):
    with pytest.raises(Called) as e:
        cli.main([recorder, "o.npy", "--modelname", "LTRCLobes_R231", "--batchsize", "5", "--nopostprocess"])
    assert e.value.args[0] == "apply" and e.value.args[2] == {}
    assert Recorder.made == dict(modelname="LTRCLobes", force_cpu=False, fillmodel="R231", batch_size=5, volume_postprocessing=False,
                                 tqdm_disable=False)


def test_metrics_are_compared_after_the_mask_is_written(recorder, tmp_path, monkeypatch):
    """A --compare-to mask that cannot be compared leaves the mask on disk: the comparison comes after it is saved."""
    import json
    import os

    from lungmask_amd import metrics as lmmetrics

    class Engine:
        def n_classes(self, slot):
            return 3

    class Plain(Recorder):
        engine = Engine()

        def apply(self, image):
            return np.zeros(image.array.shape, np.uint8)

    out = str(tmp_path / "o.npy")

    def compare_labels(a, b, **kw):
        assert os.path.exists(out) and kw["n_labels"] == 3 and kw["resample_b"] is False
        return {"compared": True}

    monkeypatch.setattr(cli, "LMInferer", Plain)
    monkeypatch.setattr(lmmetrics, "compare_labels", compare_labels)
    assert cli.main([recorder, out, "--compare-to", recorder, "--metrics", str(tmp_path / "m.json")]) == 0
    assert json.load(open(tmp_path / "m.json")) == {"compared": True}


def test_nothing_labelled_refuses_registration_beside_another_product(recorder, monkeypatch):
    """The one refusal that needs the labels: registration beside another product, with no labelled voxel to register on."""

    class Engine:
        def n_classes(self, slot):
            return 3

    class Empty(Recorder):
        engine = Engine()

        def apply_with_stats(self, image):
            return np.zeros(image.array.shape, np.uint8), {}

    monkeypatch.setattr(cli, "LMInferer", Empty)
    with pytest.raises(SystemExit) as e:
        cli.main([recorder, "o.npy", "--stats", "s.json", "--register-moving", recorder, "--registration", "t.json"])
    assert e.value.code == "--register-moving: no voxel is labelled, nothing to register on"
