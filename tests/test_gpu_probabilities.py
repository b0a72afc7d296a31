"""Per-class probability maps at the input's geometry on the GPU: lm_apply_probs_dev / Engine.apply_probs /
LMInferer.apply_probabilities / the CLI's --probabilities, against the oracle recipe (oracle U-Net log-probabilities, np.exp,
scipy.ndimage.zoom(order=1) into the boxes of the oracle pre-processing, background fill: tests/test_probabilities_emu.py)."""
import numpy as np
import pytest
import torch

from oracle import prepost_oracle as po
from oracle import unet_oracle as uo
from tests.test_probabilities_emu import oracle_probs

pytestmark = pytest.mark.gpu
TOL = 1e-3  # the engine's log-probabilities are held to 1e-3 of the reference's (split-f16 today: <= 4.1e-4)


def oracle_maps(sd, vol):
    xs, boxes = po.preprocess(vol, [256, 256])
    x = po.normalise(xs)[:, None]
    with torch.inference_mode():
        logp = uo.forward(sd, torch.from_numpy(x)).numpy()
    return oracle_probs(logp, np.asarray(boxes, np.int32), vol.shape[1], vol.shape[2])


def check_maps(probs, ref, shape, ncls):
    assert probs.shape == (ncls,) + tuple(shape) and probs.dtype == np.float32
    err = float(np.abs(probs - ref).max())
    assert err <= TOL, err
    assert float(np.abs(probs.astype(np.float64).sum(axis=0) - 1.0).max()) <= 1e-5
    return err


def inferer(gpu_engine, sd, **kw):
    from lungmask_amd import LMInferer

    return LMInferer(state_dict=sd, engine=gpu_engine, **kw)


def test_r231_phantom_labels_and_maps(gpu_engine):
    sd = uo.synthetic_state_dict(3)
    vol = po.phantom(24, 512, 512, seed=61)
    ref = oracle_maps(sd, vol)
    for vp in (True, False):
        inf = inferer(gpu_engine, sd, volume_postprocessing=vp)
        labels, probs = inf.apply_probabilities(vol)
        assert np.array_equal(labels, inf.apply(vol)), vp
        err = check_maps(probs, ref, vol.shape, 3)
        print(f"R231 24 x 512^2, post-processing {vp}: max |dp| vs oracle {err:.2e}")
        _, p16 = inf.apply_probabilities(vol, dtype=np.float16)
        assert p16.dtype == np.float16 and np.array_equal(p16.view(np.uint16), probs.astype(np.float16).view(np.uint16))
        inf.close()


@pytest.mark.parametrize("dtype", [np.int32, np.float32])
def test_ltrclobes_odd_geometry(gpu_engine, dtype):
    sd = uo.synthetic_state_dict(6)
    vol = po.phantom(37, 300, 277, seed=62).astype(dtype)
    ref = oracle_maps(sd, vol)
    for vp in (True, False):
        inf = inferer(gpu_engine, sd, modelname="LTRCLobes", volume_postprocessing=vp)
        labels, probs = inf.apply_probabilities(vol)
        assert np.array_equal(labels, inf.apply(vol)), vp
        err = check_maps(probs, ref, vol.shape, 6)
        print(f"LTRCLobes 37 x 300 x 277 {np.dtype(dtype)}, post-processing {vp}: max |dp| vs oracle {err:.2e}")
        inf.close()
    gpu_engine.load_state_dict(0, uo.synthetic_state_dict(3))


def test_maps_independent_of_batch_size_and_lanes(gpu_engine):
    sd = uo.synthetic_state_dict(3)
    vol = po.phantom(23, 512, 512, seed=63)
    gpu_engine.load_state_dict(0, sd)
    lab0, ref = gpu_engine.apply_probs(0, vol, batch_size=20)
    for bs in (1, 7, 20):
        for lanes in (1, 2):
            gpu_engine.set_streams(lanes)
            try:
                lab, p = gpu_engine.apply_probs(0, vol, batch_size=bs)
            finally:
                gpu_engine.set_streams(2)
            assert np.array_equal(lab, lab0), (bs, lanes)
            assert np.array_equal(p.view(np.uint32), ref.view(np.uint32)), (bs, lanes, int((p != ref).sum()))


def test_seam_forward_then_uncrop_equals_pipeline(gpu_engine):
    """lm_forward_dev(..., logp) on the engine's own pre-processed slices, then lm_uncrop_probs_dev == apply_probabilities."""
    sd = uo.synthetic_state_dict(3)
    vol = po.phantom(9, 512, 488, seed=64)
    inf = inferer(gpu_engine, sd)
    _, probs = inf.apply_probabilities(vol)
    _, xf, bbox, _ = gpu_engine.preprocess(vol)
    _, logp = gpu_engine.forward(0, xf)
    for dt in (np.float32, np.float16):
        seam = gpu_engine.uncrop_probs(logp, bbox, vol.shape[1:], dt)
        want = probs if dt == np.float32 else probs.astype(np.float16)
        assert np.array_equal(seam, want), (dt, int((seam != want).sum()))
    inf.close()


def test_range_guard_rerun_regenerates_the_maps(gpu_engine, monkeypatch):
    """A model whose activations leave the f16 range at run time (loaded without the probe, as in test_gpu_forward.py): the guard
    re-runs the volume on the exact-fp32 kernels, and the maps must come from that re-run -- bit-identical to an f32 inferer's."""
    from tests.test_forward_emu import out_of_f16_range_state_dict

    sd = out_of_f16_range_state_dict(3)
    vol = po.phantom(7, 512, 512, seed=65)
    try:
        monkeypatch.setenv("LM_ACC_GUARD", "0")
        inf = inferer(gpu_engine, sd, batch_size=2)
        assert gpu_engine.model_precision(0) == "split_f16"
        labels, probs = inf.apply_probabilities(vol)
        assert gpu_engine.model_precision(0) == "f32"  # the guard tripped and re-ran the volume
        monkeypatch.delenv("LM_ACC_GUARD")
        ref_inf = inferer(gpu_engine, sd, batch_size=2, precision="f32")
        ref_labels, ref_probs = ref_inf.apply_probabilities(vol)
        assert np.array_equal(labels, ref_labels)
        assert np.array_equal(probs.view(np.uint32), ref_probs.view(np.uint32)), int((probs != ref_probs).sum())
        assert float(np.abs(probs.astype(np.float64).sum(axis=0) - 1.0).max()) <= 1e-5
    finally:
        gpu_engine.set_precision("split_f16")
        gpu_engine.load_state_dict(0, uo.synthetic_state_dict(3))


def test_non_lps_volume(gpu_engine):
    from lungmask_amd import volume_io as vio

    sd = uo.synthetic_state_dict(3)
    lps = po.phantom(6, 512, 512, seed=66)
    d = np.zeros((3, 3))
    d[0, 0], d[2, 1], d[1, 2] = 1, -1, 1  # index x -> L, index y -> I, index z -> P
    img = vio.Volume(lps.transpose(1, 0, 2)[:, ::-1, :].copy(), (0.7, 1.5, 0.7), (0, 0, 0), d)
    assert vio.orientation_code(img.direction) == "LIP"
    inf = inferer(gpu_engine, sd)
    lab_lps, p_lps = inf.apply_probabilities(lps)
    labels, probs = inf.apply_probabilities(img)
    assert np.array_equal(labels, inf.apply(img))
    axes, flips = vio.lps_transform(img.direction)
    inv = vio.inverse_transform(axes, flips)
    assert probs.shape == (3,) + img.array.shape
    for c in range(3):
        assert np.array_equal(probs[c], vio.apply_transform(p_lps[c], *inv)), c
    assert np.array_equal(labels, vio.apply_transform(lab_lps, *inv))
    _, p16 = inf.apply_probabilities(img, dtype=np.float16)  # (2-byte elements through lm_reorient_dev)
    assert np.array_equal(p16.view(np.uint16), probs.astype(np.float16).view(np.uint16))
    inf.close()


def test_refusals_leave_the_engine_usable(gpu_engine):
    from lungmask_amd import LMInferer

    sd3, sd6 = uo.synthetic_state_dict(3), uo.synthetic_state_dict(6)
    vol = po.phantom(4, 512, 512, seed=67)
    fused = LMInferer(modelname="LTRCLobes", fillmodel="R231", state_dict=sd6, fill_state_dict=sd3, engine=gpu_engine)
    with pytest.raises(ValueError, match="fused mode"):
        fused.apply_probabilities(vol)
    fused.close()
    multi = LMInferer(state_dict=sd3, device_ids=[0, 0])
    try:
        with pytest.raises(NotImplementedError, match="single device_id"):
            multi.apply_probabilities(vol)
    finally:
        multi.close()
    # the C ABI: a bad output dtype, an empty slot; the fused mode has no entry point here (no fill slot in the signature)
    eng = gpu_engine
    eng.load_state_dict(0, sd3)
    vd = eng.to_device(vol)
    pd = eng.empty((3,) + vol.shape, np.float32)
    try:
        assert eng.L.lib.lm_apply_probs_dev(eng.h, 0, vd.ptr, 0, *vol.shape, 20, 1, None, 3, pd.ptr) == -1  # LM_F64 maps
        assert b"prob_dtype" in eng.L.lib.lm_last_error()
        assert eng.L.lib.lm_apply_probs_dev(eng.h, 3, vd.ptr, 0, *vol.shape, 20, 1, None, 2, pd.ptr) == -3  # empty slot
    finally:
        vd.free()
        pd.free()
    # after the refusals: apply is still what the engine computes on its own, and the maps are still right
    ref = LMInferer(state_dict=sd3, engine=gpu_engine)
    got = ref.apply(vol).copy()
    assert np.array_equal(got, gpu_engine.apply(0, vol))
    labels, probs = ref.apply_probabilities(vol)
    assert np.array_equal(labels, got)
    check_maps(probs, oracle_maps(sd3, vol), vol.shape, 3)
    ref.close()


def test_cli_probabilities(gpu_engine, tmp_path):
    import gzip
    import struct

    from lungmask_amd import LMInferer
    from lungmask_amd.__main__ import main

    sd = uo.synthetic_state_dict(3)
    wp, ip = tmp_path / "w.pth", tmp_path / "in.npy"
    torch.save(sd, wp)
    vol = po.phantom(5, 512, 512, seed=68)
    np.save(ip, vol)
    assert main([str(ip), str(tmp_path / "plain.npy"), "--modelpath", str(wp), "--noprogress"]) == 0
    plain = np.load(tmp_path / "plain.npy")
    ref_labels, ref_probs = LMInferer(state_dict=sd, engine=gpu_engine).apply_probabilities(vol)
    for name in ("p.nii.gz", "p.npy"):
        op = tmp_path / ("out_" + name.split(".", 1)[1].replace(".", "_") + ".npy")
        assert main([str(ip), str(op), "--modelpath", str(wp), "--noprogress", "--probabilities", str(tmp_path / name)]) == 0
        assert np.array_equal(np.load(op), plain)
        assert np.array_equal(plain, ref_labels)
        if name.endswith(".npy"):
            got = np.load(tmp_path / name)
            assert got.dtype == np.float32
        else:
            buf = gzip.open(tmp_path / name).read()
            dim = struct.unpack_from("<8h", buf, 40)
            assert dim == (4, 512, 512, 5, 3, 1, 1, 1) and struct.unpack_from("<h", buf, 70)[0] == 16
            got = np.frombuffer(buf, "<f4", offset=int(struct.unpack_from("<f", buf, 108)[0])).reshape(3, 5, 512, 512)
        assert np.array_equal(got, ref_probs)
    with pytest.raises(SystemExit, match="LTRCLobes_R231"):
        main([str(ip), str(tmp_path / "x.npy"), "--modelname", "LTRCLobes_R231", "--probabilities", str(tmp_path / "q.npy")])
    assert not (tmp_path / "x.npy").exists()
