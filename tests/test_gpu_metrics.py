"""Label agreement metrics on the MI355X: lm_edt_dev and lm_label_agreement_dev against the numpy oracles of
tests/test_metrics_emu.py at sizes that exercise the tiling, the full 300 x 512 x 512 pair against numpy (integers, exact) and scipy
(distances, 1e-6 relative), compare_labels on an LMInferer.apply result, distance_transform, the device form and the CLI."""
import json

import numpy as np
import pytest
import torch

from lungmask_amd import metrics as lm
from lungmask_amd import synthetic as syn
from lungmask_amd import volume_io
from tests.test_metrics_emu import (SPACINGS, WORD_SPACINGS, assert_agreement_equal, bits, blobs, oracle_agreement, oracle_edt, surface,
                                    word_boundary_rows)

pytestmark = pytest.mark.gpu
ndi = pytest.importorskip("scipy.ndimage")


@pytest.mark.parametrize("spacing", SPACINGS)
def test_edt_against_oracle(gpu_engine, spacing):
    rng = np.random.default_rng(40)
    for shape in ((40, 200, 264), (1, 300, 70), (33, 1, 130), (70, 45, 33)):
        feat = (rng.random(shape) < 0.0005).astype(np.uint8)
        feat[shape[0] // 2, shape[1] // 3, 5] = 3
        got = gpu_engine.edt(feat, spacing)
        assert np.array_equal(bits(got), bits(oracle_edt(feat, spacing))), (shape, spacing)
    assert np.all(np.isposinf(gpu_engine.edt(np.zeros((3, 40, 70), np.uint8), spacing)))


@pytest.mark.parametrize("spacing", WORD_SPACINGS)
def test_edt_word_boundaries(gpu_engine, spacing):
    feat = word_boundary_rows()
    assert np.array_equal(bits(gpu_engine.edt(feat, spacing)), bits(oracle_edt(feat, spacing))), spacing


def test_distance_transform(gpu_engine):
    rng = np.random.default_rng(41)
    feat = rng.random((20, 90, 130)) < 0.001
    sp = SPACINGS[1]
    d2 = lm.distance_transform(feat, sp, squared=True, engine=gpu_engine)
    want = oracle_edt(feat, sp)
    assert d2.dtype == np.float32 and np.array_equal(bits(d2), bits(want))
    d = lm.distance_transform(feat, sp, engine=gpu_engine)
    assert d.dtype == np.float32 and np.all(np.abs(d.view(np.int32) - np.sqrt(want).view(np.int32)) <= 1)
    ref = ndi.distance_transform_edt(~feat, sampling=sp)
    print("max relative deviation from scipy:", float(np.max(np.abs(d - ref) / np.maximum(ref, 1e-30))))
    assert np.allclose(d, ref, rtol=1e-6, atol=0)


@pytest.mark.parametrize("n_labels", [3, 6, 16])
def test_agreement_against_oracle(gpu_engine, n_labels):
    rng = np.random.default_rng(42 + n_labels)
    shape = (40, 200, 264) if n_labels == 3 else (24, 90, 136)
    a = blobs(rng, shape, n_labels, extra=1, fill=0.3)
    b = np.roll(a, (1, 2, 3), (0, 1, 2))
    b[rng.random(shape) < 0.02] = 0
    qs = (0, 50, 95, 100)
    got = gpu_engine.label_agreement(a, b, n_labels, SPACINGS[1], qs)
    assert_agreement_equal(got, oracle_agreement(a, b, n_labels, SPACINGS[1], qs), n_labels)
    odd = (7, 33, 70)  # w not a multiple of 16: the scalar path
    a, b = blobs(rng, odd, n_labels), blobs(rng, odd, n_labels)
    assert_agreement_equal(gpu_engine.label_agreement(a, b, n_labels, None, qs), oracle_agreement(a, b, n_labels, None, qs), "odd")


def test_agreement_dev_equals_host_form(gpu_engine):
    rng = np.random.default_rng(50)
    a, b = blobs(rng, (20, 64, 96), 3), blobs(rng, (20, 64, 96), 3)
    ad, bd = gpu_engine.to_device(a), gpu_engine.to_device(b)
    dev = gpu_engine.label_agreement_dev(ad, bd, 3, SPACINGS[2], (95,))
    host = gpu_engine.label_agreement(a, b, 3, SPACINGS[2], (95,))
    assert_agreement_equal(dev, host, "dev")
    assert np.array_equal(dev["sum_d_ab"], host["sum_d_ab"])  # the same schedule: the same sums
    ad.free()
    bd.free()


def _lunglike_labels(gpu_engine, vol, classes=3):
    gpu_engine.load_state_dict(0, syn.synthetic_state_dict(classes, head="lunglike"))
    return gpu_engine.apply(0, vol)


def test_agreement_full_phantom(gpu_engine):
    """300 x 512 x 512: a = lung-like lobes, b = a shifted by (1, 2, 3) voxels with one lobe eroded."""
    vol = syn.phantom(300, 512, 512)
    lab = _lunglike_labels(gpu_engine, vol)
    assert (lab == 1).sum() > 10 ** 6 and (lab == 2).sum() > 10 ** 6
    a = (lab * 2 + (np.arange(300)[:, None, None] > 150)) * (lab > 0)  # five labels + background
    a = np.minimum(a, 5).astype(np.uint8)
    b = np.zeros_like(a)
    b[1:, 2:, 3:] = a[:-1, :-2, :-3]
    b[(b == 4) & ~ndi.binary_erosion(b == 4, iterations=2)] = 0
    sp = SPACINGS[1]
    qs = (50, 95)
    got = gpu_engine.label_agreement(a, b, 6, sp, qs)
    for k in range(6):
        A, B = (a >= 1, b >= 1) if k == 0 else (a == k, b == k)
        if not (A | B).any():  # (label 1 of this construction: lab * 2 starts at 2)
            assert (got["voxels_a"][k], got["voxels_b"][k], got["surface_a"][k], got["surface_b"][k]) == (0, 0, 0, 0), k
            assert got["bbox"][k].tolist() == [-1] * 6 and got["max_d2_ab"][k] == -1, k
            continue
        z, y, x = np.nonzero(A | B)
        box = (slice(z.min(), z.max() + 1), slice(y.min(), y.max() + 1), slice(x.min(), x.max() + 1))
        sa, sb = surface(A)[box], surface(B)[box]  # (surfaces of the whole volume: its border counts, the crop's does not)
        A, B = A[box], B[box]
        assert (got["voxels_a"][k], got["voxels_b"][k], got["intersection"][k]) == (A.sum(), B.sum(), (A & B).sum()), k
        assert (got["surface_a"][k], got["surface_b"][k]) == (sa.sum(), sb.sum()), k
        assert got["bbox"][k].tolist() == [z.min(), z.max() + 1, y.min(), y.max() + 1, x.min(), x.max() + 1], k
        dab = ndi.distance_transform_edt(~sb, sampling=sp)[sa]
        dba = ndi.distance_transform_edt(~sa, sampling=sp)[sb]
        rel = []
        for name, g, w in (("max ab", np.sqrt(float(got["max_d2_ab"][k])), dab.max()), ("max ba", np.sqrt(float(got["max_d2_ba"][k])), dba.max()),
                           ("sum ab", got["sum_d_ab"][k], dab.sum()), ("sum ba", got["sum_d_ba"][k], dba.sum())):
            rel.append((name, abs(g - w) / w))
        for i, q in enumerate(qs):
            for f, lst in (("order_ab", dab), ("order_ba", dba), ("order_pooled", np.concatenate([dab, dba]))):
                s = np.sort(lst)
                pos = (q / 100.0) * (s.size - 1)
                for j, r in enumerate((int(np.floor(pos)), int(np.ceil(pos)))):
                    w = s[min(r, s.size - 1)]
                    rel.append((f"{f} {q} {j}", abs(np.sqrt(float(got[f][k, i, j])) - w) / max(w, 1e-30) if w > 0 else float(got[f][k, i, j])))
        print(f"row {k}: surfaces {sa.sum()} / {sb.sum()}, largest relative deviation from scipy {max(r for _, r in rel):.3g}")
        assert all(r <= 1e-6 for _, r in rel), (k, [x for x in rel if x[1] > 1e-6])
    assert got["other_a"] == 0 and got["other_b"] == 0
    assert sum(int(got["surface_a"][k] > 0 and got["surface_b"][k] > 0) for k in range(6)) >= 5  # four lobes and the lung


def test_compare_labels_on_apply_result(gpu_engine):
    from lungmask_amd.mask import LMInferer

    inf = LMInferer(state_dict=syn.synthetic_state_dict(3, head="lunglike"), engine=gpu_engine)
    img = volume_io.Volume(syn.phantom(40, 512, 512), (0.7, 0.8, 2.5))
    x = img.like(inf.apply(img))
    out = lm.compare_labels(x, x, names={1: "right lung", 2: "left lung"}, engine=gpu_engine)
    assert out["unit"] == "mm" and out["spacing_mm"] == [2.5, 0.8, 0.7] and set(out["labels"]) == {"1", "2"}
    for row in (out["lung"], out["labels"]["1"], out["labels"]["2"]):
        assert row["voxels_a"] > 0 and row["dice"] == 1.0 and row["jaccard"] == 1.0 and row["hausdorff"] == 0.0 and row["assd"] == 0.0
        assert row["percentiles"]["95"] == {"a_to_b": 0.0, "b_to_a": 0.0, "pooled": 0.0}
    assert out["lung"]["voxels_a"] == int((x.array > 0).sum()) and out["labels"]["1"]["name"] == "right lung"
    assert json.loads(json.dumps(out)) == out
    y = np.roll(x.array, 2, 2)
    moved = lm.compare_labels(x.array, y, spacing=(2.5, 0.8, 0.7), engine=gpu_engine)  # two voxels along x
    assert 0 < moved["lung"]["dice"] < 1 and 0 < moved["lung"]["hausdorff"] <= 2 * 0.7 + 1e-6


def test_cli_metrics(gpu_engine, tmp_path):
    from lungmask_amd import LMInferer
    from lungmask_amd.__main__ import main

    sd = syn.synthetic_state_dict(3, head="lunglike")
    wp = tmp_path / "w.pth"
    torch.save(sd, wp)
    img = volume_io.Volume(syn.phantom(20, 512, 512), (0.7, 0.7, 2.0), (1.0, 2.0, 3.0))
    ip = tmp_path / "in.nii.gz"
    volume_io.write_nifti(str(ip), img)
    loaded = volume_io.load_input_image(str(ip))
    ref_labels = LMInferer(modelpath=str(wp), engine=gpu_engine).apply(loaded)
    truth = np.roll(ref_labels, 1, 1)
    mp = tmp_path / "truth.nii.gz"
    volume_io.write_nifti(str(mp), loaded.like(truth))
    np.save(tmp_path / "truth.npy", truth)
    want = json.loads(json.dumps(lm.compare_labels(loaded.like(ref_labels), loaded.like(truth), n_labels=3, engine=gpu_engine)))
    assert 0 < want["lung"]["dice"] < 1 and want["lung"]["hausdorff"] > 0
    assert main([str(ip), str(tmp_path / "out.npy"), "--modelpath", str(wp), "--noprogress", "--compare-to", str(mp), "--metrics",
                 str(tmp_path / "m.json")]) == 0
    assert json.load(open(tmp_path / "m.json")) == want
    assert np.array_equal(np.load(tmp_path / "out.npy"), ref_labels)
    assert main([str(ip), str(tmp_path / "out2.npy"), "--modelpath", str(wp), "--noprogress", "--compare-to", str(tmp_path / "truth.npy"),
                 "--metrics", str(tmp_path / "m2.json"), "--stats", str(tmp_path / "s.json"), "--probabilities", str(tmp_path / "p.npy")]) == 0
    assert json.load(open(tmp_path / "m2.json")) == want
    assert json.load(open(tmp_path / "s.json"))["lung"]["voxels"] == want["lung"]["voxels_a"]
