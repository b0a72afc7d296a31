"""Texture matrices on the MI355X: lm_texture_dev against the numpy oracle of tests/test_texture_emu.py (every dtype, the emulation
shapes, a volume of many workgroups, a 4096-long run), LMInferer.apply_with_texture (R231, LTRCLobes) and the CLI's --texture."""
import json

import numpy as np
import pytest
import torch

from lungmask_amd import stats as st
from lungmask_amd import synthetic as syn
from lungmask_amd import texture as tx
from lungmask_amd import volume_io
from tests.test_texture_emu import assert_texture_equal, check, oracle_texture, random_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [np.int16, np.int32, np.int64, np.float32, np.float64])
def test_texture_dev_dtypes(gpu_engine, dtype):
    rng = np.random.default_rng(11)
    lab, vol = random_case(rng, (3, 21, 48), 3, dtype)
    if np.dtype(dtype).kind == "f":
        vol = vol + rng.choice([0.0, 0.25, 0.5, -0.5, 1.5], vol.shape).astype(dtype)
        vol.flat[::97] = np.nan
        vol.flat[1::101] = np.inf
        vol.flat[2::103] = -3e9
    check(gpu_engine, lab, vol, 3, what=dtype)


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 5, 7), (2, 3, 33), (4, 13, 50), (3, 11, 64), (5, 1, 16)])
def test_texture_dev_shapes(gpu_engine, shape):
    rng = np.random.default_rng(12)
    lab, vol = random_case(rng, shape, 3, extra=2)
    if shape == (1, 1, 1):
        lab[...], vol[...] = 1, -900
    one = shape == (1, 1, 1)
    check(gpu_engine, lab, vol, 3, pairs=() if one else None, runs=(1,) if one else None, what=shape)
    check(gpu_engine, lab, vol, 3, pairs=(), runs=(1,) if one else None, what=(shape, "distance 2, 64 levels"), distance=2, hi=599, nr=8)


def _blobs(rng, shape, n_labels, cell=8):
    coarse = rng.integers(0, n_labels, tuple((s + cell - 1) // cell for s in shape))
    for a in range(3):
        coarse = np.repeat(coarse, cell, axis=a)
    return coarse[:shape[0], :shape[1], :shape[2]].astype(np.uint8)


def test_texture_dev_many_workgroups(gpu_engine):
    """40 x 128 x 160 with 6 labels in blobs: many workgroups per direction, the slab reduction, runs across chunk borders."""
    rng = np.random.default_rng(13)
    shape = (40, 128, 160)
    _, vol = random_case(rng, shape, 6)
    lab = _blobs(rng, shape, 7)  # (label 6 >= n_labels takes no part)
    got = check(gpu_engine, lab, vol, 6, what="blobs")
    again = gpu_engine.texture(lab, vol, 6)  # two identical calls, identical results
    for f in got:
        assert np.array_equal(got[f], again[f]), f
    check(gpu_engine, lab, vol.astype(np.float32), 6, what="blobs f32, distance 3", distance=3)


def test_texture_dev_longest_run(gpu_engine):
    """One constant 4096-long row per label: longest_run, the clamped last column and texture_matrices' second call."""
    lab = np.ones((1, 2, 4096), np.uint8)
    lab[0, 1] = 2
    vol = np.full(lab.shape, -500, np.int16)
    got = check(gpu_engine, lab, vol, 3, pairs=(1, 2), what="row")
    assert list(got["longest_run"]) == [0, 4096, 4096] and got["glrlm"][1, 0, 20, 63] == 1
    raw = tx.texture_matrices(vol, lab, engine=gpu_engine)
    assert raw["glrlm"].shape == (3, 13, 48, 4096) and raw["glrlm"][2, 0, 20, 4095] == 1
    assert_texture_equal(raw, oracle_texture(lab, vol, 3), (1, 2), (1, 2), "row, unclamped")


def _oracle_dict(vol, labels, n_labels, names, **kw):
    return tx.finalize(oracle_texture(labels, vol, n_labels, **kw), oracle_texture((labels > 0).astype(np.uint8), vol, 2, **kw), names)


@pytest.mark.parametrize("model", ["R231", "LTRCLobes"])
def test_apply_with_texture_models(gpu_engine, model):
    from lungmask_amd.mask import LMInferer

    c = 3 if model == "R231" else 6
    inf = LMInferer(engine=gpu_engine, modelname=model, state_dict=syn.synthetic_state_dict(c, head="lunglike"))
    vol = syn.phantom(20, 512, 512)
    expect = inf.apply(vol).copy()
    labels, texture = inf.apply_with_texture(vol)
    assert np.array_equal(labels, expect)
    assert texture == _oracle_dict(vol, expect, c, st.label_names(model, c))
    assert json.loads(json.dumps(texture)) == texture
    lung = texture["lung"]
    assert lung["valid"] > 0 and lung["glcm"]["contrast"] is not None and lung["glrlm"]["run_percentage"] is not None
    assert sum(texture["labels"][str(k)]["voxels"] for k in range(1, c)) == lung["voxels"] == int((expect > 0).sum())
    assert any(texture["labels"][str(k)]["glcm"]["joint_entropy"] for k in range(1, c))


def test_cli_texture(gpu_engine, tmp_path):
    from lungmask_amd import LMInferer
    from lungmask_amd.__main__ import main

    sd = syn.synthetic_state_dict(3, head="lunglike")
    wp = tmp_path / "w.pth"
    torch.save(sd, wp)
    img = volume_io.Volume(syn.phantom(20, 512, 512), (0.7, 0.7, 2.0), (1.0, 2.0, 3.0))
    ip = tmp_path / "in.nii.gz"
    volume_io.write_nifti(str(ip), img)
    loaded = volume_io.load_input_image(str(ip))
    inf = LMInferer(modelpath=str(wp), engine=gpu_engine)
    ref_labels, ref = inf.apply_with_texture(loaded)
    ref = json.loads(json.dumps(ref))
    assert ref["lung"]["valid"] > 0
    base = [str(ip), str(tmp_path / "out.npy"), "--modelpath", str(wp), "--noprogress"]
    assert main(base + ["--texture", str(tmp_path / "t.json")]) == 0
    assert json.load(open(tmp_path / "t.json")) == ref
    assert np.array_equal(np.load(tmp_path / "out.npy"), ref_labels)
    assert main(base + ["--texture", str(tmp_path / "t2.json"), "--stats", str(tmp_path / "s.json")]) == 0
    assert json.load(open(tmp_path / "t2.json")) == ref
    assert json.load(open(tmp_path / "s.json"))["lung"]["voxels"] == ref["lung"]["voxels"]
    _, ref50 = inf.apply_with_texture(loaded, hu_range=(-1000, -200), bin_width=50)
    assert main(base + ["--texture", str(tmp_path / "t3.json"), "--texture-bin-width", "50", "--texture-range", "-1000", "-200"]) == 0
    assert json.load(open(tmp_path / "t3.json")) == json.loads(json.dumps(ref50)) and ref50["levels"] == 17
