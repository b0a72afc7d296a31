"""LMInferer.apply_pair and the --pair flags on the emulator with the labelling replaced by a fixed volume (the pattern of
test_apply_deformable_on_the_emulator): the labels are apply's, the registration is apply_deformable's / apply_registered's, the
analysis equals pairs.pair_analysis on the downloaded pieces in the one-GPU branch and in the detour of the multi-GPU forms; the
command line writes what the API returns, and without the flags it writes no file more."""
import json
import os

import numpy as np
import pytest

from lungmask_amd import pairs
from lungmask_amd import volume_io
from tests.test_deform_emu import same_bits
from tests.test_mask_wrappers_emu import Harness
from tests.test_register_emu import REG_SPACING, RIGID_CASES, lung_classes, registration_case

RKW = dict(levels_mm=(8.0,), max_evaluations=20)
DKW = dict(levels_mm=(8.0, 6.0), iterations=(4, 3))
NAMES = {1: "right lung", 2: "left lung"}


def case():
    fixed, moving, _ = registration_case("rigid", RIGID_CASES["a"])
    labels = (lung_classes(fixed.array) == 1).astype(np.uint8)
    labels[:, :, 44:] *= 2  # two labels
    return fixed, moving, labels


def same_pair(a, b):
    return a.analysis == b.analysis and np.array_equal(a.table, b.table) and a.class_names == b.class_names and \
        all((x is None and y is None) or same_bits(x, y) for x, y in ((a.classes, b.classes), (a.change, b.change), (a.jacobian, b.jacobian)))


def test_apply_pair_on_the_emulator(emu_engine, monkeypatch):
    fixed, moving, labels = case()
    h = Harness(emu_engine, labels)
    try:
        kw = dict(margin_mm=6.0, moving_spacing=REG_SPACING, register_kw=RKW)
        for host in (False, True):
            if host:
                monkeypatch.setattr(h.inf, "_shard", object())
            h.reset()
            out, r, pair = h.inf.apply_pair(fixed, moving, deformable_kw=DKW, names=NAMES, **kw)
            assert np.array_equal(out, labels) and h.applied == (1 if host else 0)
            _, want_r = h.inf.apply_deformable(fixed, moving, **kw, **DKW)
            assert same_bits(r.field.array, want_r.field.array) and same_bits(r.image, want_r.image) and r.levels == want_r.levels
            assert r.field_dev is None and r.affine_registration.parameters == want_r.affine_registration.parameters
            want = pairs.pair_analysis(fixed, moving, labels, r, names=NAMES, moving_spacing=REG_SPACING, engine=emu_engine)
            assert same_pair(pair, want) and pair.analysis["transform"] == "deformable" and pair.analysis["n_labels"] == 3
            lung = pair.analysis["lung"]
            assert lung["voxels"] == int((labels > 0).sum()) and lung["analysed"] > 0.9 * lung["voxels"] and lung["classified"] > 0
            assert pair.analysis["labels"]["1"]["name"] == "right lung" and pair.classes.dtype == np.uint8 and pair.change.dtype == np.float32
            assert json.loads(json.dumps(pair.analysis)) == pair.analysis
            # the affine stage alone, a longitudinal pair, one map
            out, r, pair = h.inf.apply_pair(fixed, moving, deformable=False, roles=None, maps=("change",), hu_range=(-1000, -400),
                                            fixed_threshold=-900, n_labels=3, **kw)
            _, want_r = h.inf.apply_registered(fixed, moving, margin_mm=6.0, moving_spacing=REG_SPACING, **RKW)
            assert np.array_equal(out, labels) and r.parameters == want_r.parameters and same_bits(r.image, want_r.image)
            want = pairs.pair_analysis(fixed, moving, labels, r, roles=None, maps=("change",), hu_range=(-1000, -400), fixed_threshold=-900,
                                       n_labels=3, names=h.inf._model_labels(None)[1], moving_spacing=REG_SPACING, engine=emu_engine)
            assert same_pair(pair, want) and pair.classes is None and pair.jacobian is None and pair.analysis["transform"] == "affine"
            assert pair.class_names == ("neither", "fixed_only", "moving_only", "both") and pair.analysis["jac_scale"] == pairs.jac_scale(r.transform)
        with pytest.raises(ValueError, match="roles"):
            h.inf.apply_pair(fixed, moving, roles=("a", "b"))
        with pytest.raises(TypeError, match="unexpected"):
            h.inf.apply_pair(fixed, moving, moving_spacing=REG_SPACING, deformable_kw=dict(labels=labels))
        with pytest.raises(TypeError, match="deformable=True"):
            h.inf.apply_pair(fixed, moving, deformable=False, deformable_kw=DKW)
    finally:
        monkeypatch.undo()
        h.inf.close()
    e = Harness(emu_engine, np.zeros_like(labels))
    try:
        with pytest.raises(ValueError, match="no voxel is labelled"):
            e.inf.apply_pair(fixed, moving, moving_spacing=REG_SPACING)
    finally:
        e.inf.close()


def test_cli_pair_flags(emu_engine, monkeypatch, tmp_path):
    import lungmask_amd.__main__ as cli

    fixed, moving, labels = case()
    moving = volume_io.Volume(np.asarray(moving), REG_SPACING[::-1], (0.0, 0.0, 0.0))
    h = Harness(emu_engine, labels)
    try:
        # the command line has no flag for the registration's schedule: a short one for both sides of the comparison
        slow = h.inf.apply_pair
        quick = lambda *a, **kw: slow(*a, register_kw=RKW, deformable_kw=DKW if kw.get("deformable", True) else None, **kw)  # noqa: E731
        monkeypatch.setattr(h.inf, "apply_pair", quick)
        monkeypatch.setattr(h.inf, "apply_registered", lambda *a, **kw: Harness_registered(h, *a, **kw))
        monkeypatch.setattr(cli, "LMInferer", lambda **kw: h.inf)
        monkeypatch.setattr(h.inf, "close", lambda: None, raising=False)
        ip, mp = tmp_path / "in.nii.gz", tmp_path / "moving.nii.gz"
        volume_io.write_nifti(str(ip), fixed)
        volume_io.write_nifti(str(mp), moving)
        image, mv = volume_io.load_input_image(str(ip)), volume_io.load_input_image(str(mp))
        common = [str(ip), str(tmp_path / "out.npy"), "--noprogress", "--register-moving", str(mp)]
        jp, cp, dp = tmp_path / "pair.json", tmp_path / "classes.nii.gz", tmp_path / "change.npy"
        assert cli.main(common + ["--register-deformable", "--pair", str(jp), "--pair-classes", str(cp), "--pair-change", str(dp), "--pair-roles",
                                  "exp-insp", "--pair-thresholds", "-870", "-940", "--pair-range", "-1000", "-450"]) == 0
        _, _, want = quick(image, mv, deformable=True, roles=("expiration", "inspiration"), fixed_threshold=-870.0, moving_threshold=-940.0,
                           hu_range=(-1000.0, -450.0), maps=("classes", "change"))
        assert json.load(open(jp)) == want.analysis and want.analysis["class_names"] == ["normal", "fsad", "uncategorised", "emphysema"]
        back = volume_io.load_input_image(str(cp))
        assert back.array.dtype == np.uint8 and np.array_equal(back.array, want.classes) and same_bits(np.load(dp), want.change)
        assert np.array_equal(np.load(tmp_path / "out.npy"), labels) and want.analysis["lung"]["classified"] > 0
        # the affine stage alone, the default roles
        assert cli.main(common + ["--pair", str(jp)]) == 0
        _, _, want = quick(image, mv, deformable=False, maps=("classes", "change"))
        assert json.load(open(jp)) == want.analysis and want.analysis["transform"] == "affine" and want.analysis["roles"] == ["inspiration", "expiration"]
        # without the flags: the files a registration run wrote before, and no other
        for f in (jp, cp, dp):
            os.remove(f)
        before = sorted(os.listdir(tmp_path))
        assert cli.main(common + ["--registration", str(tmp_path / "t.json")]) == 0
        assert sorted(os.listdir(tmp_path)) == sorted(before + ["t.json"])
        for bad in (["--pair-roles", "longitudinal"], ["--pair-range", "-1000", "-500"]):
            with pytest.raises(SystemExit, match="need --pair"):
                cli.main(common + ["--registration", str(tmp_path / "t.json")] + bad)
        with pytest.raises(SystemExit, match="--register-moving"):
            cli.main([str(ip), str(tmp_path / "out.npy"), "--pair", str(jp)])
        with pytest.raises(SystemExit, match="outside hu_range"):
            cli.main(common + ["--pair", str(jp), "--pair-thresholds", "-300", "-856"])
        with pytest.raises(SystemExit, match="unsupported file type"):
            cli.main(common + ["--pair", str(tmp_path / "pair.txt")])
    finally:
        monkeypatch.undo()
        h.inf.close()


def Harness_registered(h, *a, **kw):
    """apply_registered with the short schedule (the run without the pair flags)."""
    return type(h.inf).apply_registered(h.inf, *a, **dict(RKW, **kw))
