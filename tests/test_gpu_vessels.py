"""The vessel filter on the MI355X: the emulator suite's cases bit for bit against the numpy oracle, the device form against the host
form, LMInferer.apply_with_vessels in the single-GPU, fused and several-engines modes, and the command line."""
import json

import numpy as np
import pytest
import torch

from lungmask_amd import stats as lmstats
from lungmask_amd import synthetic as syn
from lungmask_amd import vessels as vs
from lungmask_amd import volume_io
from tests.test_filters_emu import SHAPES, assert_same_bits, lung_labels
from tests.test_vessels_emu import (run_counts, run_filter_equality, run_hessian_cases, run_masked_property, run_meaning, run_nonfinite,
                                    run_state_rule, run_vesselness_cases, volume)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", SHAPES)
def test_hessian(gpu_engine, shape):
    run_hessian_cases(gpu_engine, shape)


@pytest.mark.parametrize("shape", SHAPES)
def test_vesselness(gpu_engine, shape):
    run_vesselness_cases(gpu_engine, shape)


def test_properties(gpu_engine):
    run_filter_equality(gpu_engine)
    run_masked_property(gpu_engine)
    run_nonfinite(gpu_engine)
    run_counts(gpu_engine)


def test_meaning(gpu_engine):
    run_meaning(gpu_engine)


def test_state_rule(gpu_engine):
    run_state_rule(gpu_engine)


def test_device_form_equals_host_form(gpu_engine):
    shape = (5, 33, 70)
    vol, lab = volume(shape, np.float32, 3), lung_labels(shape, 3)
    sigmas = [(0.5, 0.5, 0.5), (1.0, 1.75, 1.0)]
    vd, ld = gpu_engine.to_device(vol), gpu_engine.to_device(lab)
    V, scale = gpu_engine.vesselness_dev(vd, sigmas, lab=ld, keep=(1, 2), return_scale=True)
    gpu_engine.sync()
    hv, hs = gpu_engine.vesselness(vol, sigmas, lab, keep=(1, 2), return_scale=True)
    assert_same_bits(V.download(), hv)
    assert_same_bits(scale.download(), hs)
    again, none = gpu_engine.vesselness_dev(vd, sigmas, bright=False, out=V)  # a caller's output array; the workspace is reused
    gpu_engine.sync()
    assert again is V and none is None
    assert_same_bits(again.download(), gpu_engine.vesselness(vol, sigmas, bright=False))
    comp, eig = gpu_engine.hessian_dev(vd, sigmas[1], lab=ld, eigenvalues=True)
    gpu_engine.sync()
    hc, he = gpu_engine.hessian(vol, sigmas[1], lab, eigenvalues=True)
    assert_same_bits(comp.download(), hc)
    assert_same_bits(eig.download(), he)
    comp2, none = gpu_engine.hessian_dev(vd, sigmas[0], out=comp)
    gpu_engine.sync()
    assert comp2 is comp and none is None
    assert_same_bits(comp.download(), gpu_engine.hessian(vol, sigmas[0]))
    assert np.array_equal(ld.download(), lab)
    assert_same_bits(vd.download(), vol)  # the inputs are unchanged
    for d in (vd, ld, V, scale, comp, eig):
        d.free()


def _inferer_kw(model):
    fused = model == "LTRCLobes_R231"
    return dict(modelname="LTRCLobes" if fused else model, state_dict=syn.synthetic_state_dict(6 if fused else 3, head="lunglike"),
                fillmodel="R231" if fused else None, fill_state_dict=syn.synthetic_state_dict(3, head="lunglike") if fused else None)


def _check_result(result, vol, expect, sp, engine, names, **kw):
    V, scale = vs.vesselness(vol, labels=expect, spacing=sp, return_scale=True, engine=engine, **kw)
    assert_same_bits(result.vesselness, V)
    assert_same_bits(result.scale, scale)
    want = vs.vessel_result(vol, expect, spacing=sp, names=names, engine=engine, **kw)
    assert np.array_equal(result.mask, want.mask) and result.analysis == want.analysis
    assert not result.mask[expect == 0].any() and json.loads(json.dumps(result.analysis)) == result.analysis


@pytest.mark.parametrize("model", ["R231", "LTRCLobes_R231"])
def test_apply_with_vessels(gpu_engine, model):
    from lungmask_amd.mask import LMInferer

    inf = LMInferer(engine=gpu_engine, **_inferer_kw(model))
    vol = syn.phantom(24, 512, 512)
    expect = inf.apply(vol).copy()
    assert (expect > 0).sum() > 10 ** 4
    names = inf._model_labels()[1]
    labels, res = inf.apply_with_vessels(vol)
    assert np.array_equal(labels, expect)
    _check_result(res, vol, expect, None, gpu_engine, names)
    if model == "R231":
        sp = (2.0, 0.75, 0.75)
        labels, res = inf.apply_with_vessels(vol, sigmas_mm=(1.0, 2.0), spacing=sp)
        assert np.array_equal(labels, expect)
        _check_result(res, vol, expect, sp, gpu_engine, names, sigmas_mm=(1.0, 2.0))
        img = volume_io.Volume(vol, sp[::-1], (1.0, 2.0, 3.0))
        labels2, res2 = inf.apply_with_vessels(img, sigmas_mm=(1.0, 2.0))  # the image's own spacing
        assert np.array_equal(labels2, expect) and res2.analysis == res.analysis and np.array_equal(res2.mask, res.mask)
        assert_same_bits(res2.vesselness, res.vesselness)
        with pytest.raises(ValueError, match="spacing"):
            inf.apply_with_vessels(img, spacing=sp)
        with pytest.raises(ValueError, match="limit is 32"):
            inf.apply_with_vessels(vol, sigmas_mm=(9.0,))


def test_apply_with_vessels_several_engines(gpu_engine):
    from lungmask_amd.mask import LMInferer

    sd = syn.synthetic_state_dict(3, head="lunglike")
    vol = syn.phantom(24, 512, 512)
    one = LMInferer(state_dict=sd, engine=gpu_engine)
    lab1, r1 = one.apply_with_vessels(vol, sigmas_mm=(1.0, 2.0), spacing=(2.0, 0.8, 0.8))
    assert np.array_equal(lab1, one.apply(vol))
    inf = LMInferer(state_dict=sd, device_ids=[0, 0])
    try:
        lab2, r2 = inf.apply_with_vessels(vol, sigmas_mm=(1.0, 2.0), spacing=(2.0, 0.8, 0.8))
    finally:
        inf.close()
    assert np.array_equal(lab2, lab1) and np.array_equal(r2.mask, r1.mask) and r2.analysis == r1.analysis
    assert_same_bits(r2.vesselness, r1.vesselness)
    assert_same_bits(r2.scale, r1.scale)
    assert_same_bits(r1.vesselness, vs.vesselness(vol, (1.0, 2.0), spacing=(2.0, 0.8, 0.8), labels=lab1, engine=gpu_engine))


def test_cli_vessels(gpu_engine, tmp_path):
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
    ref_labels, res = inf.apply_with_vessels(loaded, sigmas_mm=(1.0, 2.0), threshold=0.4)
    ref_labels = ref_labels.copy()
    base = [str(ip), str(tmp_path / "out.npy"), "--modelpath", str(wp), "--noprogress"]
    assert main(base + ["--vesselness", str(tmp_path / "v.npy"), "--vessel-mask", str(tmp_path / "m.npy"), "--vessels", str(tmp_path / "v.json"),
                        "--vessel-sigmas", "1", "2", "--vessel-threshold", "0.4"]) == 0
    assert np.array_equal(np.load(tmp_path / "out.npy"), ref_labels)
    assert_same_bits(np.load(tmp_path / "v.npy"), res.vesselness)
    m = np.load(tmp_path / "m.npy")
    assert m.dtype == np.uint8 and np.array_equal(m.astype(bool), res.mask)
    assert json.load(open(tmp_path / "v.json")) == json.loads(json.dumps(res.analysis))
    # after --denoise the vessel filter reads the filtered image, and the JSON names it; combined with --stats
    _, filtered = inf.apply_denoised(loaded, method="gaussian", sigma_mm=1.0)
    names = lmstats.label_names(inf.modelname, 3)
    want = vs.vessel_result(loaded.like(filtered), ref_labels, names=names, engine=gpu_engine)
    assert main(base + ["--denoise", "gaussian:1", "--vessels", str(tmp_path / "d.json"), "--vesselness", str(tmp_path / "dv.nii.gz"),
                        "--stats", str(tmp_path / "s.json")]) == 0
    assert np.array_equal(np.load(tmp_path / "out.npy"), ref_labels)
    got = json.load(open(tmp_path / "d.json"))
    assert got.pop("denoise") == {"method": "gaussian", "sigma_mm": 1.0, "masked": True} and got == json.loads(json.dumps(want.analysis))
    assert_same_bits(np.asarray(volume_io.load_input_image(str(tmp_path / "dv.nii.gz")).array, np.float32), want.vesselness)
    assert "denoise" in json.load(open(tmp_path / "s.json"))
    with pytest.raises(SystemExit):
        main(base + ["--vessel-threshold", "0.4"])
    with pytest.raises(SystemExit):
        main(base + ["--vessels", str(tmp_path / "v.txt")])
