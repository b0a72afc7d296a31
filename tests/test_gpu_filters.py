"""The image filters on the MI355X: the emulator suite's cases bit for bit against the numpy oracle, the device form against the host
form, LMInferer.apply_denoised in the single-GPU, fused and several-engines modes, and the command line."""
import json

import numpy as np
import pytest
import torch

from lungmask_amd import filters as flt
from lungmask_amd import stats as lmstats
from lungmask_amd import synthetic as syn
from lungmask_amd import volume_io
from tests.test_filters_emu import (SHAPES, assert_same_bits, lung_labels, random_taps, run_box_property, run_median_cases, run_median_special,
                                    run_separable_cases, run_separable_special, volume)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", SHAPES)
def test_median(gpu_engine, shape):
    run_median_cases(gpu_engine, shape)


@pytest.mark.parametrize("shape", SHAPES)
def test_separable(gpu_engine, shape):
    run_separable_cases(gpu_engine, shape)


def test_special_cases_and_box(gpu_engine):
    run_median_special(gpu_engine)
    run_separable_special(gpu_engine)
    run_box_property(gpu_engine)


def test_device_form_equals_host_form(gpu_engine):
    shape = (5, 33, 70)
    vol, lab = volume(shape, np.float32, 3), lung_labels(shape, 3)
    taps = [random_taps(r, r, True) for r in (1, 7, 32)]
    vd, ld = gpu_engine.to_device(vol), gpu_engine.to_device(lab)
    outs = []
    for kw in (dict(kind="median", size=5, keep=(1,), fill=-3.0), dict(kind="separable", taps=taps, indicator=(None, -951), fill=0.0),
               dict(kind="separable", taps=taps)):
        out = gpu_engine.filter_dev(vd, ld, **kw)
        gpu_engine.sync()
        assert_same_bits(out.download(), gpu_engine.filter(vol, lab, **kw))
        outs.append(out)
    again = gpu_engine.filter_dev(vd, None, kind="median", out=outs[0])  # a caller's output array; the workspace is reused
    gpu_engine.sync()
    assert again is outs[0]
    assert_same_bits(again.download(), gpu_engine.filter(vol, None, kind="median"))
    assert np.array_equal(ld.download(), lab)
    assert_same_bits(vd.download(), vol)  # the inputs are unchanged
    for d in [vd, ld] + outs:
        d.free()


def _inferer_kw(model):
    fused = model == "LTRCLobes_R231"
    return dict(modelname="LTRCLobes" if fused else model, state_dict=syn.synthetic_state_dict(6 if fused else 3, head="lunglike"),
                fillmodel="R231" if fused else None, fill_state_dict=syn.synthetic_state_dict(3, head="lunglike") if fused else None)


@pytest.mark.parametrize("model", ["R231", "LTRCLobes_R231"])
def test_apply_denoised(gpu_engine, model):
    from lungmask_amd.mask import LMInferer

    inf = LMInferer(engine=gpu_engine, **_inferer_kw(model))
    vol = syn.phantom(24, 512, 512)
    expect = inf.apply(vol).copy()
    assert (expect > 0).sum() > 10 ** 4
    sp = (2.0, 0.75, 0.75)
    labels, med = inf.apply_denoised(vol)
    assert np.array_equal(labels, expect) and med.dtype == vol.dtype
    assert np.array_equal(med, flt.median(vol, 3, labels=expect, engine=gpu_engine)) and np.array_equal(med[expect == 0], vol[expect == 0])
    labels, g = inf.apply_denoised(vol, method="gaussian", sigma_mm=1.5, spacing=sp)
    assert np.array_equal(labels, expect)
    assert_same_bits(g, flt.gaussian(vol, 1.5, spacing=sp, labels=expect, engine=gpu_engine))
    img = volume_io.Volume(vol, sp[::-1], (1.0, 2.0, 3.0))
    labels2, g2 = inf.apply_denoised(img, method="gaussian", sigma_mm=1.5)  # the image's own spacing
    assert np.array_equal(labels2, expect)
    assert_same_bits(g2, g)
    _, plain = inf.apply_denoised(vol, size=5, masked=False)
    assert np.array_equal(plain, flt.median(vol, 5, engine=gpu_engine))
    with pytest.raises(ValueError, match="spacing"):
        inf.apply_denoised(img, spacing=sp)
    with pytest.raises(ValueError, match="sigma_mm"):
        inf.apply_denoised(vol, method="gaussian")


def test_apply_denoised_several_engines(gpu_engine):
    from lungmask_amd.mask import LMInferer

    sd = syn.synthetic_state_dict(3, head="lunglike")
    vol = syn.phantom(24, 512, 512)
    one = LMInferer(state_dict=sd, engine=gpu_engine)
    lab1, m1 = one.apply_denoised(vol)
    _, g1 = one.apply_denoised(vol, method="gaussian", sigma_mm=2.0, spacing=(2.0, 0.8, 0.8))
    inf = LMInferer(state_dict=sd, device_ids=[0, 0])
    try:
        lab2, m2 = inf.apply_denoised(vol)
        lab3, g2 = inf.apply_denoised(vol, method="gaussian", sigma_mm=2.0, spacing=(2.0, 0.8, 0.8))
    finally:
        inf.close()
    assert np.array_equal(lab2, lab1) and np.array_equal(lab3, lab1) and np.array_equal(m2, m1)
    assert_same_bits(g2, g1)


def test_cli_denoise(gpu_engine, tmp_path):
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
    ref_labels, filtered = inf.apply_denoised(loaded, method="gaussian", sigma_mm=1.0)
    ref_labels = ref_labels.copy()
    assert main([str(ip), str(tmp_path / "out.npy"), "--modelpath", str(wp), "--noprogress", "--denoise", "gaussian:1", "--denoised",
                 str(tmp_path / "d.npy"), "--stats", str(tmp_path / "s.json"), "--laa-map", str(tmp_path / "l.npy"), "--laa-sigma", "3"]) == 0
    assert np.array_equal(np.load(tmp_path / "out.npy"), ref_labels)
    assert_same_bits(np.load(tmp_path / "d.npy"), filtered)
    names = lmstats.label_names(inf.modelname, 3)
    want = lmstats.label_statistics(loaded.like(filtered), ref_labels, names=names, engine=gpu_engine, n_labels=3)
    want["denoise"] = {"method": "gaussian", "sigma_mm": 1.0, "masked": True}
    assert json.load(open(tmp_path / "s.json")) == json.loads(json.dumps(want))
    assert_same_bits(np.load(tmp_path / "l.npy"), flt.low_attenuation_map(loaded, ref_labels, sigma_mm=3.0, engine=gpu_engine))
