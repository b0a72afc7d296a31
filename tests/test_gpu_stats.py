"""Per-label statistics on the MI355X: lm_label_stats_dev against the numpy oracle of tests/test_stats_emu.py (every dtype, the
full 300 x 512 x 512 phantom with lung-like labels), LMInferer.apply_with_stats (R231, LTRCLobes, the fused mode, batch sizes, a
non-LPS Volume, several engines, repeat calls) and the CLI's --stats."""
import json

import numpy as np
import pytest
import torch

from lungmask_amd import stats as st
from lungmask_amd import synthetic as syn
from lungmask_amd import volume_io
from tests.test_stats_emu import assert_stats_equal, oracle_stats

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [np.int16, np.int32, np.int64, np.float32, np.float64])
def test_label_stats_dev_random_volumes(gpu_engine, dtype):
    rng = np.random.default_rng(11)
    for shape, n_labels in (((7, 64, 96), 3), ((5, 33, 70), 6), ((3, 40, 48), 16)):
        lab = rng.integers(0, n_labels + 1, shape).astype(np.uint8)
        vol = rng.integers(-1500, 3500, shape).astype(dtype)
        if np.dtype(dtype).kind == "f":
            vol = vol + rng.choice([0.0, 0.5, -0.5, 1.5], shape).astype(dtype)
            vol.flat[::97] = np.nan
            vol.flat[1::101] = np.inf
            vol.flat[2::103] = -3e9
        assert_stats_equal(gpu_engine.label_stats(lab, vol, n_labels), oracle_stats(lab, vol, n_labels), (dtype, shape))


def _lunglike_labels(gpu_engine, vol, classes=3):
    gpu_engine.load_state_dict(0, syn.synthetic_state_dict(classes, head="lunglike"))
    return gpu_engine.apply(0, vol)


def test_label_stats_dev_full_phantom(gpu_engine):
    """300 x 512 x 512 with the lung-like head: many workgroups per slab row, int64 sums."""
    vol = syn.phantom(300, 512, 512)
    lab = _lunglike_labels(gpu_engine, vol)
    assert (lab == 1).sum() > 10 ** 6 and (lab == 2).sum() > 10 ** 6
    want = oracle_stats(lab, vol, 3)
    got = gpu_engine.label_stats(lab, vol, 3)
    assert_stats_equal(got, want, "phantom")
    assert_stats_equal(gpu_engine.label_stats(lab, vol.astype(np.float32), 3), want, "phantom f32")
    lobes = (lab * 2 + (np.arange(300)[:, None, None] > 150)) * (lab > 0)  # five labels + background
    lobes = np.minimum(lobes, 5).astype(np.uint8)
    assert_stats_equal(gpu_engine.label_stats(lobes, vol, 6), oracle_stats(lobes, vol, 6), "phantom lobes")


def _oracle_dict(image, labels, n_labels, names, spacing=None):
    arr, sp, to_phys = st.geometry(image, spacing)
    return st.finalize(oracle_stats(labels, np.asarray(arr), n_labels), sp, (15,), (-950,), names, to_phys)


@pytest.mark.parametrize("model", ["R231", "LTRCLobes", "LTRCLobes_R231"])
def test_apply_with_stats_models(gpu_engine, model):
    from lungmask_amd.mask import LMInferer

    fused = model == "LTRCLobes_R231"
    c = 3 if model == "R231" else 6
    kw = dict(modelname="LTRCLobes" if fused else model, state_dict=syn.synthetic_state_dict(c, head="lunglike"),
              fillmodel="R231" if fused else None, fill_state_dict=syn.synthetic_state_dict(3, head="lunglike") if fused else None)
    inf = LMInferer(engine=gpu_engine, **kw)
    vol = syn.phantom(60, 512, 512)
    expect = inf.apply(vol).copy()
    labels, stats = inf.apply_with_stats(vol, spacing=(2.0, 0.75, 0.75))
    assert np.array_equal(labels, expect)
    names = st.label_names("LTRCLobes" if c == 6 else "R231", c)
    assert stats == _oracle_dict(vol, expect, c, names, spacing=(2.0, 0.75, 0.75))
    assert json.loads(json.dumps(stats)) == stats
    assert stats["lung"]["voxels"] == int((expect > 0).sum()) > 0
    labels2, stats2 = inf.apply_with_stats(vol, spacing=(2.0, 0.75, 0.75))  # two identical calls, identical results
    assert np.array_equal(labels2, labels) and stats2 == stats


def test_apply_with_stats_batch_size_invariance(gpu_engine):
    from lungmask_amd.mask import LMInferer

    sd = syn.synthetic_state_dict(3, head="lunglike")
    vol = syn.phantom(45, 512, 512)
    results = [LMInferer(state_dict=sd, engine=gpu_engine, batch_size=b).apply_with_stats(vol) for b in (1, 7, 20, 64)]
    for lab, s in results[1:]:
        assert np.array_equal(lab, results[0][0]) and s == results[0][1]


def test_apply_with_stats_non_lps_volume(gpu_engine):
    """Statistics of a non-LPS Volume are in the caller's index order and its physical space."""
    from lungmask_amd.mask import LMInferer

    inf = LMInferer(state_dict=syn.synthetic_state_dict(3, head="lunglike"), engine=gpu_engine)
    vol = syn.phantom(40, 512, 512)
    direction = (0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, -1.0, 0.0)  # permuted and flipped
    axes, flips = volume_io.lps_transform(direction)
    arr = np.ascontiguousarray(volume_io.apply_transform(vol, *volume_io.inverse_transform(axes, flips)))
    img = volume_io.Volume(arr, (0.7, 0.8, 2.5), (-12.0, 30.0, 4.5), direction)
    expect = inf.apply(img).copy()
    labels, stats = inf.apply_with_stats(img)
    assert np.array_equal(labels, expect)
    assert stats == _oracle_dict(img, expect, 3, st.label_names("R231", 3))
    s1 = stats["labels"]["1"]
    z, y, x = np.nonzero(expect == 1)
    assert s1["bbox"] == [int(z.min()), int(z.max()) + 1, int(y.min()), int(y.max()) + 1, int(x.min()), int(x.max()) + 1]
    c = [z.mean(), y.mean(), x.mean()]
    np.testing.assert_allclose(s1["centroid_index"], c, rtol=1e-12)
    np.testing.assert_allclose(s1["centroid_mm"], img.index_to_physical(c[::-1]), atol=1e-9)
    assert stats["spacing_mm"] == [2.5, 0.8, 0.7]


def test_apply_with_stats_several_engines(gpu_engine):
    from lungmask_amd.mask import LMInferer

    sd = syn.synthetic_state_dict(3, head="lunglike")
    vol = syn.phantom(25, 512, 512)
    single = LMInferer(state_dict=sd, engine=gpu_engine)
    lab1, s1 = single.apply_with_stats(vol)
    inf = LMInferer(state_dict=sd, device_ids=[0, 0, 0])
    try:
        lab3, s3 = inf.apply_with_stats(vol)
    finally:
        inf.close()
    assert np.array_equal(lab3, lab1) and s3 == s1


def test_cli_stats(gpu_engine, tmp_path):
    from lungmask_amd import LMInferer
    from lungmask_amd.__main__ import main

    sd = syn.synthetic_state_dict(3, head="lunglike")
    wp = tmp_path / "w.pth"
    torch.save(sd, wp)
    img = volume_io.Volume(syn.phantom(20, 512, 512), (0.7, 0.7, 2.0), (1.0, 2.0, 3.0))
    ip = tmp_path / "in.nii.gz"
    volume_io.write_nifti(str(ip), img)
    loaded = volume_io.load_input_image(str(ip))
    ref_labels, ref_stats = LMInferer(modelpath=str(wp), engine=gpu_engine).apply_with_stats(loaded)  # (names "label k")
    ref_stats = json.loads(json.dumps(ref_stats))
    assert main([str(ip), str(tmp_path / "out.npy"), "--modelpath", str(wp), "--noprogress", "--stats", str(tmp_path / "s.json")]) == 0
    assert json.load(open(tmp_path / "s.json")) == ref_stats
    assert np.array_equal(np.load(tmp_path / "out.npy"), ref_labels)
    assert main([str(ip), str(tmp_path / "out2.npy"), "--modelpath", str(wp), "--noprogress", "--stats", str(tmp_path / "s2.json"),
                 "--probabilities", str(tmp_path / "p.npy")]) == 0
    assert json.load(open(tmp_path / "s2.json")) == ref_stats
    assert np.array_equal(np.load(tmp_path / "out2.npy"), ref_labels)
