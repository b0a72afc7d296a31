"""The skeleton, the point list and the calibre classes on the MI355X: the emulator suite's cases bit for bit against the numpy oracle,
the device form against the host form, repeated runs of the in-place thinning, LMInferer.apply_with_vessel_tree in the single-GPU,
fused and several-engines modes, and the command line."""
import json

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

from lungmask_amd import skeleton as sk
from lungmask_amd import synthetic as syn
from lungmask_amd import volume_io
from tests.test_filters_emu import assert_same_bits
from tests.test_skeleton_emu import (CALIBRE_SPACINGS, CASES, calibre_volume, case, run_calibre, run_idempotent, run_points, run_state_rule,
                                     run_thinning_case, topology)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(CASES))
def test_thinning(gpu_engine, name):
    run_thinning_case(gpu_engine, name)


@pytest.mark.parametrize("name", ["torus", "random_0.5", "block_x"])
def test_second_call_is_identity(gpu_engine, name):
    run_idempotent(gpu_engine, name)


def test_points(gpu_engine):
    run_points(gpu_engine)


@pytest.mark.parametrize("spacing", CALIBRE_SPACINGS)
def test_calibre(gpu_engine, spacing):
    run_calibre(gpu_engine, spacing)


def test_state_rule(gpu_engine):
    run_state_rule(gpu_engine)


def test_device_form_equals_host_form(gpu_engine):
    sel, keep, want, info = case("keep_two")
    csel, clab = calibre_volume()
    sd, cd, ld = gpu_engine.to_device(sel), gpu_engine.to_device(csel), gpu_engine.to_device(clab)
    out, got_info = gpu_engine.skeleton_dev(sd, keep)
    assert np.array_equal(out.download(), want) and got_info == info
    again, _ = gpu_engine.skeleton_dev(sd, keep, out=out)  # a caller's output array; the workspace is reused
    assert again is out and np.array_equal(out.download(), want)
    kd, _ = gpu_engine.skeleton_dev(cd)
    cls, counts, d2 = gpu_engine.calibre_dev(kd, cd, (1.0, 2.0), spacing=(2.5, 0.75, 1.25), lab=ld, return_distance=True)
    hc, hcounts, hd2 = gpu_engine.calibre(kd.download(), csel, (1.0, 2.0), lab=clab, spacing=(2.5, 0.75, 1.25), return_distance=True)
    assert np.array_equal(cls.download(), hc) and np.array_equal(counts, hcounts)
    assert_same_bits(d2.download(), hd2)
    idx, code, dist, total = gpu_engine.skeleton_points_dev(kd, d2)
    codes = kd.download()
    assert total == idx.size == int((codes != 0).sum()) and np.array_equal(idx, np.flatnonzero(codes.ravel()))
    assert_same_bits(dist, hd2.ravel()[idx])
    mask = gpu_engine.vessel_mask_dev(d2, ld, 2.0)
    assert np.array_equal(mask.download(), ((clab != 0) & (hd2 >= np.float32(2.0))).astype(np.uint8))
    assert np.array_equal(sd.download(), sel) and np.array_equal(cd.download(), csel) and np.array_equal(ld.download(), clab)  # inputs unchanged
    for d in (sd, cd, ld, out, kd, cls, d2, mask):
        d.free()


def test_three_runs_give_identical_bytes(gpu_engine):
    """(24, 96, 80), thousands of candidates per sub-step in many workgroups: the in-place deletion is free of races."""
    rng = np.random.default_rng(17)
    vol = (ndi.gaussian_filter(rng.normal(size=(24, 96, 80)), 1.5) > 0.05).astype(np.uint8)
    runs = [gpu_engine.skeleton(vol, return_info=True) for _ in range(3)]
    codes, info = runs[0]
    assert info["selected"] == int(vol.sum()) > 30000 and info["skeleton"] < info["selected"] // 4 and info["passes"] >= 3
    for other, other_info in runs[1:]:
        assert np.array_equal(other, codes) and other_info == info
    assert topology(codes != 0) == topology(vol != 0) and not (codes != 0)[vol == 0].any()
    count = ndi.convolve((codes != 0).astype(np.int32), np.ones((3, 3, 3), np.int32), mode="constant")
    assert np.array_equal(codes, np.where(codes != 0, count, 0))


def _inferer_kw(model):
    fused = model == "LTRCLobes_R231"
    return dict(modelname="LTRCLobes" if fused else model, state_dict=syn.synthetic_state_dict(6 if fused else 3, head="lunglike"),
                fillmodel="R231" if fused else None, fill_state_dict=syn.synthetic_state_dict(3, head="lunglike") if fused else None)


def _same(a, b):
    assert a.tree == b.tree and a.analysis == b.analysis and np.array_equal(a.mask, b.mask)
    assert np.array_equal(a.skeleton, b.skeleton) and np.array_equal(a.calibre, b.calibre)
    assert_same_bits(a.vesselness, b.vesselness)
    assert_same_bits(a.scale, b.scale)


@pytest.mark.parametrize("model", ["R231", "LTRCLobes_R231"])
def test_apply_with_vessel_tree(gpu_engine, model):
    from lungmask_amd.mask import LMInferer

    inf = LMInferer(engine=gpu_engine, **_inferer_kw(model))
    vol = syn.phantom(24, 512, 512)
    names = inf._model_labels()[1]
    sp = (2.0, 0.75, 0.75)
    kw = dict(sigmas_mm=(1.0, 2.0), threshold=0.2, c=2.0, calibres_mm2=(3.0, 8.0))  # (c: the phantom holds noise, no vessels)
    labels, res = inf.apply_with_vessel_tree(vol, spacing=sp, **kw)
    expect = labels.copy()
    assert np.array_equal(expect, inf.apply(vol)) and (expect > 0).sum() > 10 ** 4
    _same(res, sk.vessel_tree(vol, expect, spacing=sp, names=names, engine=gpu_engine, **kw))
    print(model, "vessel voxels", int(res.mask.sum()), "skeleton", res.tree["lung"]["skeleton_voxels"], "segments", res.tree["lung"]["segments"],
          "junctions", res.tree["lung"]["junctions"])
    assert res.mask.any() and res.skeleton.any() and not (res.skeleton != 0)[~res.mask].any() and not res.calibre[~res.mask].any()
    assert json.loads(json.dumps(res.tree)) == res.tree
    if model == "R231":
        img = volume_io.Volume(vol, sp[::-1], (1.0, 2.0, 3.0))
        labels2, res2 = inf.apply_with_vessel_tree(img, **kw)  # the image's own spacing
        assert np.array_equal(labels2, expect)
        _same(res2, res)
        with pytest.raises(ValueError, match="calibres_mm2"):
            inf.apply_with_vessel_tree(vol, calibres_mm2=(8.0, 3.0))


def test_apply_with_vessel_tree_several_engines(gpu_engine):
    from lungmask_amd.mask import LMInferer

    sd = syn.synthetic_state_dict(3, head="lunglike")
    vol = syn.phantom(24, 512, 512)
    kw = dict(sigmas_mm=(1.0, 2.0), threshold=0.2, c=2.0, spacing=(2.0, 0.8, 0.8))
    one = LMInferer(state_dict=sd, engine=gpu_engine)
    lab1, r1 = one.apply_with_vessel_tree(vol, **kw)
    lab1 = lab1.copy()
    inf = LMInferer(state_dict=sd, device_ids=[0, 0])
    try:
        lab2, r2 = inf.apply_with_vessel_tree(vol, **kw)
    finally:
        inf.close()
    assert np.array_equal(lab2, lab1) and r1.skeleton.any()
    _same(r2, r1)


def test_cli_vessel_tree(gpu_engine, tmp_path):
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
    # (the phantom holds noise, no vessels, and the command line has Frangi's default c: a threshold low enough for a mask of speckle)
    ref_labels, res = inf.apply_with_vessel_tree(loaded, sigmas_mm=(1.0, 2.0), threshold=0.0001, calibres_mm2=(3.0, 8.0))
    ref_labels = ref_labels.copy()
    base = [str(ip), str(tmp_path / "out.npy"), "--modelpath", str(wp), "--noprogress"]
    assert main(base + ["--vessel-skeleton", str(tmp_path / "k.npy"), "--vessel-calibre", str(tmp_path / "c.npy"), "--vessel-tree",
                        str(tmp_path / "t.json"), "--vessel-mask", str(tmp_path / "m.npy"), "--vessels", str(tmp_path / "v.json"),
                        "--vessel-sigmas", "1", "2", "--vessel-threshold", "0.0001", "--vessel-calibres", "3", "8"]) == 0
    assert np.array_equal(np.load(tmp_path / "out.npy"), ref_labels) and res.skeleton.any()
    assert np.array_equal(np.load(tmp_path / "k.npy"), res.skeleton) and np.array_equal(np.load(tmp_path / "c.npy"), res.calibre)
    assert np.array_equal(np.load(tmp_path / "m.npy").astype(bool), res.mask)
    assert json.load(open(tmp_path / "t.json")) == json.loads(json.dumps(res.tree))
    assert json.load(open(tmp_path / "v.json")) == json.loads(json.dumps(res.analysis))
    with pytest.raises(SystemExit):
        main(base + ["--vessel-calibres", "5"])
    with pytest.raises(SystemExit):
        main(base + ["--vessel-tree", str(tmp_path / "t.txt")])
