"""The minimax flood, the airway mask and the airway segmentation on the MI355X: the emulator suite's cases and the phantom bit for bit
against the numpy oracle, the device form against the host form, a caller's output array, repeated runs of the in-place relaxation on
a volume with many bricks active per round, LMInferer.apply_with_airways in the single-GPU, fused and several-engines modes, and the
command line."""
import json

import numpy as np
import pytest
import torch

from lungmask_amd import airways as aw
from lungmask_amd import synthetic as syn
from lungmask_amd import volume_io
from tests.test_airway_emu import (CASES, UNREACHED, check_cap_monotone, check_edge_contact, check_history_independent,
                                   check_mask_is_seed_component, check_phantom_quality, check_serpentine, cost_oracle, mask_oracle, noise,
                                   run_cost_case, run_mask_case)
from tests.test_airway_host import same_result

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(CASES))
def test_cost_matches_oracle(gpu_engine, name):
    run_cost_case(gpu_engine, name)


def test_serpentine_needs_rounds_and_max_rounds_stops(gpu_engine):
    check_serpentine(gpu_engine)


def test_no_diagonal_passage_over_brick_edges(gpu_engine):
    check_edge_contact(gpu_engine)


def test_properties(gpu_engine):
    check_cap_monotone(gpu_engine)
    check_mask_is_seed_component(gpu_engine)
    check_history_independent(gpu_engine)


@pytest.mark.parametrize("name", ["odd_17_9_33", "flat_1_6_8", "impassable_seed", "float32"])
def test_mask_and_counts(gpu_engine, name):
    run_mask_case(gpu_engine, name)


def test_phantom_quality(gpu_engine):
    check_phantom_quality(gpu_engine)


def test_device_form_equals_host_form_and_inputs_stay(gpu_engine):
    vol, seeds, cap = CASES["odd_17_9_33"]
    want, want_curve, reached, _ = cost_oracle(vol, seeds, cap)
    lab = np.random.default_rng(3).integers(0, 5, vol.shape).astype(np.uint8)
    vd, ld = gpu_engine.to_device(vol), gpu_engine.to_device(lab)
    cost, curve, info = gpu_engine.seed_cost_dev(vd, seeds, cap)
    host_cost, host_curve, host_info = gpu_engine.seed_cost(vol, seeds, cap)
    assert np.array_equal(cost.download(), want) and np.array_equal(host_cost, want) and info == host_info and info["reached"] == reached
    assert np.array_equal(curve, want_curve) and np.array_equal(host_curve, want_curve)
    out = gpu_engine.empty(vol.shape, np.int16)
    again, _, _ = gpu_engine.seed_cost_dev(vd, seeds, cap, out=out)  # a caller's output array; the workspace is reused
    assert again is out and np.array_equal(out.download(), want)
    mask_out = gpu_engine.empty(vol.shape, np.uint8)
    mask, counts = gpu_engine.airway_mask_dev(cost, -700, lab=ld, out=mask_out)
    want_mask, want_counts = mask_oracle(want, -700, lab)
    assert mask is mask_out and np.array_equal(mask.download(), want_mask) and np.array_equal(counts, want_counts)
    assert np.array_equal(vd.download(), vol) and np.array_equal(ld.download(), lab) and np.array_equal(cost.download(), want)  # inputs unchanged
    for d in (vd, ld, cost, out, mask_out):
        d.free()


def test_three_runs_give_identical_bytes(gpu_engine):
    """(24, 96, 80), 3 x 12 x 3 bricks, most of them active in most rounds: the in-place update is free of races."""
    vol = noise((24, 96, 80), -1100, -300, 31)
    seeds = [(12, 48, 40), (0, 0, 0), (23, 95, 79)]
    runs = [gpu_engine.seed_cost(vol, seeds, cap_hu=-600) for _ in range(3)]
    cost, curve, info = runs[0]
    assert info["rounds"] >= 3 and info["reached"] > vol.size // 3
    for other, other_curve, other_info in runs[1:]:
        assert other.tobytes() == cost.tobytes() and other_curve.tobytes() == curve.tobytes() and other_info == info
    want, want_curve, _, _ = cost_oracle(vol, seeds, -600)
    assert np.array_equal(cost, want) and np.array_equal(curve, want_curve)


def chest(n=24):
    """The package's phantom with a trachea written into it: a tube of -990 HU down the middle of the body, closed by tissue."""
    vol = syn.phantom(n, 512, 512)
    y, x = np.mgrid[0:512, 0:512]
    vol[:, (y - 256) ** 2 + (x - 256) ** 2 <= 36] = -990
    return vol


def _inferer_kw(model):
    fused = model == "LTRCLobes_R231"
    return dict(modelname="LTRCLobes" if fused else model, state_dict=syn.synthetic_state_dict(6 if fused else 3, head="lunglike"),
                fillmodel="R231" if fused else None, fill_state_dict=syn.synthetic_state_dict(3, head="lunglike") if fused else None)


@pytest.mark.parametrize("model", ["R231", "LTRCLobes_R231"])
def test_apply_with_airways(gpu_engine, model):
    from lungmask_amd.mask import LMInferer

    inf = LMInferer(engine=gpu_engine, **_inferer_kw(model))
    vol = chest()
    names = inf._model_labels()[1]
    sp = (2.0, 0.75, 0.75)
    labels, res = inf.apply_with_airways(vol, spacing=sp)
    expect = labels.copy()
    assert np.array_equal(expect, inf.apply(vol)) and (expect > 0).sum() > 10 ** 4
    same_result(res, aw.segment_airways(vol, expect, spacing=sp, names=names, engine=gpu_engine))
    print(model, "seed", res.seed, "threshold", res.threshold, "voxels", res.analysis["voxels"], "rounds", res.analysis["rounds"],
          "segments", res.tree["totals"]["segments"])
    assert res.analysis["error"] is None and res.seed[0][0] == 0 and abs(res.seed[0][1] - 256) <= 6 and abs(res.seed[0][2] - 256) <= 6
    assert res.mask[:, 256, 256].all() and 24 * 100 <= res.mask.sum() <= 24 * 120 and res.tree["totals"]["segments"] >= 1
    assert json.loads(json.dumps(res.meta())) == res.meta()
    if model == "R231":
        img = volume_io.Volume(vol, sp[::-1], (1.0, 2.0, 3.0))
        labels2, res2 = inf.apply_with_airways(img, seed=(3, 256, 256), threshold=-900)  # the image's own spacing; no search, no rule
        assert np.array_equal(labels2, expect) and res2.threshold == -900 and res2.analysis["trachea"] is None
        same_result(res2, aw.segment_airways(vol, expect, seed=(3, 256, 256), threshold=-900, spacing=sp, names=names, engine=gpu_engine))
        labels3, res3 = inf.apply_with_airways(syn.phantom(24, 512, 512))  # no trachea: the labels and the reason
        assert np.array_equal(labels3, inf.apply(syn.phantom(24, 512, 512))) and "no candidate" in res3.analysis["error"] and not res3.mask.any()
        with pytest.raises(ValueError, match="cap_hu"):
            inf.apply_with_airways(vol, cap_hu=4000)


def test_apply_with_airways_several_engines(gpu_engine):
    from lungmask_amd.mask import LMInferer

    sd = syn.synthetic_state_dict(3, head="lunglike")
    vol = chest()
    kw = dict(spacing=(2.0, 0.8, 0.8))
    one = LMInferer(state_dict=sd, engine=gpu_engine)
    lab1, r1 = one.apply_with_airways(vol, **kw)
    lab1 = lab1.copy()
    inf = LMInferer(state_dict=sd, device_ids=[0, 0])
    try:
        lab2, r2 = inf.apply_with_airways(vol, **kw)
    finally:
        inf.close()
    assert np.array_equal(lab2, lab1) and r1.mask.any()
    same_result(r2, r1)


def test_cli_airways(gpu_engine, tmp_path):
    from lungmask_amd import LMInferer
    from lungmask_amd.__main__ import main

    sd = syn.synthetic_state_dict(3, head="lunglike")
    wp = tmp_path / "w.pth"
    torch.save(sd, wp)
    img = volume_io.Volume(chest(20), (0.7, 0.7, 2.0), (1.0, 2.0, 3.0))
    ip = tmp_path / "in.nii.gz"
    volume_io.write_nifti(str(ip), img)
    loaded = volume_io.load_input_image(str(ip))
    inf = LMInferer(modelpath=str(wp), engine=gpu_engine)
    ref_labels, res = inf.apply_with_airways(loaded)
    ref_labels = ref_labels.copy()
    base = [str(ip), str(tmp_path / "out.npy"), "--modelpath", str(wp), "--noprogress"]
    assert main(base + ["--airways", str(tmp_path / "a.npy"), "--airway-tree", str(tmp_path / "t.json"), "--airway-cost", str(tmp_path / "c.npy")]) == 0
    assert np.array_equal(np.load(tmp_path / "out.npy"), ref_labels) and res.mask.any()
    assert np.array_equal(np.load(tmp_path / "a.npy"), res.mask) and np.array_equal(np.load(tmp_path / "c.npy"), res.cost)
    assert np.load(tmp_path / "c.npy").dtype == np.int16 and (np.load(tmp_path / "c.npy")[res.mask == 0] > res.threshold).all()
    assert json.load(open(tmp_path / "t.json")) == json.loads(json.dumps(res.meta()))
    assert main(base + ["--airways", str(tmp_path / "b.npy"), "--stats", str(tmp_path / "s.json")]) == 0  # beside another product
    assert np.array_equal(np.load(tmp_path / "b.npy"), res.mask)
    with pytest.raises(SystemExit):
        main(base + ["--airway-threshold", "-900"])
    with pytest.raises(SystemExit):
        main(base + ["--airway-tree", str(tmp_path / "t.txt")])
    assert UNREACHED == aw.UNREACHED
