"""Connected components, their table and the cluster analysis on the MI355X: the emulator suite's cases bit for bit against the numpy
oracle, the device forms against the host forms, LMInferer.apply_with_clusters and the command line."""
import json

import numpy as np
import pytest
import torch

from lungmask_amd import _native as nat
from lungmask_amd import components as cp
from lungmask_amd import synthetic as syn
from lungmask_amd import volume_io
from tests.test_components_emu import (INT_MAX, INT_MIN, SHAPES, assert_rows_equal, check_components, checkerboard, oracle_table, random_case,
                                       raw_table, serpentine)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", SHAPES)
def test_random_labels(gpu_engine, shape):
    labels, image = random_case(shape, sum(shape))
    for hu_range in ((-950, -200), (None, -951), (-300, None), None):
        assert check_components(gpu_engine, image, labels, hu_range=hu_range)[1] > 0
    check_components(gpu_engine, None, labels)
    check_components(gpu_engine, None, labels, connectivity=26)
    check_components(gpu_engine, image, labels, hu_range=(-700, None), connectivity=26, per_label=False)
    check_components(gpu_engine, image, labels, hu_range=(-700, None), per_label=False)


def test_checkerboard_and_cap(gpu_engine):
    shape = (5, 33, 70)
    labels = checkerboard(shape)
    image = random_case(shape, 1)[1]
    ids, T, rows = check_components(gpu_engine, image, labels)
    assert T == labels.sum() and (rows["voxels"] == 1).all()
    want = oracle_table(ids, labels, image)
    for cap in (100, T, 100000, 0):
        got, total = raw_table(gpu_engine, ids, labels, image, cap)
        k = min(cap, T)
        assert total == T
        assert_rows_equal(got[:k], want[:k])
        assert (got[k:].view(np.uint8) == 0x5A).all()
    assert check_components(gpu_engine, None, labels, connectivity=26)[1] == 1


def test_large_components(gpu_engine):
    shape = SHAPES[4]
    labels = np.full(shape, 3, np.uint8)
    _, T, rows = check_components(gpu_engine, random_case(shape, 2)[1], labels)
    groups, per = gpu_engine.component_table_launch(labels.size)
    assert T == 1 and rows["voxels"][0] == labels.size and groups >= 2 and per < labels.size
    assert check_components(gpu_engine, None, serpentine((5, 33, 70)))[1] == 1
    small = np.ones((5, 33, 70), np.uint8)
    image = np.full(small.shape, INT_MAX, np.int32)
    image[3:] = INT_MIN
    _, _, rows = check_components(gpu_engine, image, small)
    assert rows["hu_min"][0] == INT_MIN and rows["hu_max"][0] == INT_MAX
    assert check_components(gpu_engine, np.full(small.shape, INT_MAX, np.int32), small)[2]["hu_sum"][0] == small.size * INT_MAX


def test_borders_corners_keep_empty(gpu_engine):
    labels = np.zeros((3, 7, 600), np.uint8)
    labels[1, 2:5, 10:300] = 1
    labels[1, 2:5, 300:590] = 2
    assert check_components(gpu_engine, None, labels, per_label=True)[1] == 2
    assert check_components(gpu_engine, None, labels, per_label=False)[1] == 1
    corner = np.zeros((5, 33, 70), np.uint8)
    corner[1, 4, 63] = corner[2, 5, 64] = 1
    assert check_components(gpu_engine, None, corner, connectivity=6)[1] == 2
    assert check_components(gpu_engine, None, corner, connectivity=26)[1] == 1
    labels, image = random_case((5, 33, 70), 4)
    check_components(gpu_engine, image, labels, keep=(2, 5), hu_range=(None, -300))
    ids, T, rows = check_components(gpu_engine, image, labels, hu_range=(5000, None))
    assert T == 0 and not ids.any() and rows.shape == (0,)


def test_float_image(gpu_engine):
    shape = (5, 33, 70)
    rng = np.random.default_rng(9)
    labels = rng.integers(0, 3, shape).astype(np.uint8)
    image = (rng.integers(-2000, 400, shape) / 2).astype(np.float32)
    flat = image.ravel()
    flat[rng.choice(flat.size, 300, replace=False)] = np.nan
    flat[rng.choice(flat.size, 100, replace=False)] = np.inf
    flat[rng.choice(flat.size, 100, replace=False)] = -np.inf
    for hu_range in ((-950, -200), (None, -500), None):
        check_components(gpu_engine, image, labels, hu_range=hu_range)
    check_components(gpu_engine, image.astype(np.float64), labels, hu_range=(-950, -200))


def test_device_forms_and_relabel(gpu_engine):
    labels, image = random_case((5, 33, 70), 8)
    kw = dict(hu_range=(None, -600))
    ids, T, counts, rows = gpu_engine.components(labels, image, **kw)
    ld, vd = gpu_engine.to_device(labels), gpu_engine.to_device(image)
    d_ids, total, d_counts = gpu_engine.components_dev(ld, vd, **kw)
    d_rows, d_total = gpu_engine.component_table_dev(d_ids, ld, vd)
    assert total == d_total == T and np.array_equal(d_ids.download(), ids) and np.array_equal(d_counts, counts)
    assert_rows_equal(d_rows, rows)
    assert np.array_equal(ld.download(), labels) and np.array_equal(vd.download(), image)  # the inputs are unchanged
    lut = np.concatenate([[0], np.random.default_rng(0).permutation(T) + 1]).astype(np.int32)
    out = gpu_engine.relabel_dev(d_ids, lut)
    assert np.array_equal(out.download(), lut[ids]) and np.array_equal(d_ids.download(), ids)
    assert gpu_engine.relabel_dev(d_ids, lut, out=d_ids) is d_ids and np.array_equal(d_ids.download(), lut[ids])
    d_ids.upload(ids)
    with pytest.raises(nat.LMError, match="outside the table"):  # an error code, not an out-of-bounds read
        gpu_engine.relabel_dev(d_ids, lut[:T], out=d_ids)
    assert np.array_equal(d_ids.download(), np.where(ids < T, lut[np.minimum(ids, T - 1)], 0))
    got = cp.find_components(image, labels, order="size", min_voxels=2, engine=gpu_engine, **kw)
    assert (np.diff(got.table["voxels"]) <= 0).all() and got.table["voxels"].min() >= 2 and got.count == (rows["voxels"] >= 2).sum()
    for d in (ld, vd, d_ids, out):
        d.free()


@pytest.mark.parametrize("model", ["R231", "LTRCLobes_R231"])
def test_apply_with_clusters(gpu_engine, model):
    from lungmask_amd.mask import LMInferer

    fused = model == "LTRCLobes_R231"
    kw = dict(modelname="LTRCLobes" if fused else model, state_dict=syn.synthetic_state_dict(6 if fused else 3, head="lunglike"),
              fillmodel="R231" if fused else None, fill_state_dict=syn.synthetic_state_dict(3, head="lunglike") if fused else None)
    inf = LMInferer(engine=gpu_engine, **kw)
    vol = syn.phantom(24, 512, 512)
    expect = inf.apply(vol).copy()
    assert (expect > 0).sum() > 10 ** 4
    sp = (2.0, 0.75, 0.75)
    labels, clusters = inf.apply_with_clusters(vol, spacing=sp)
    assert np.array_equal(labels, expect)
    from lungmask_amd import stats as st

    names = st.label_names(inf.modelname, max(1, min(gpu_engine.n_classes(0), st.MAX_LABELS)))
    assert clusters == cp.cluster_analysis(vol, expect, spacing=sp, names=names, engine=gpu_engine)
    assert sum(e["selected"] for e in clusters["labels"].values()) == ((vol < -950) & (expect > 0)).sum() == clusters["lung"]["selected"]
    assert json.loads(json.dumps(clusters)) == clusters
    img = volume_io.Volume(vol, sp[::-1], (1.0, 2.0, 3.0))
    labels2, clusters2 = inf.apply_with_clusters(img, threshold=-900, connectivity=26)  # the image's own spacing
    assert np.array_equal(labels2, expect)
    assert clusters2 == cp.cluster_analysis(img, expect, threshold=-900, connectivity=26, names=names, engine=gpu_engine)
    with pytest.raises(ValueError, match="spacing"):
        inf.apply_with_clusters(img, spacing=sp)


def test_cli_clusters(gpu_engine, tmp_path):
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
    ref_labels, ref = inf.apply_with_clusters(loaded)
    ref_labels = ref_labels.copy()
    assert main([str(ip), str(tmp_path / "out.npy"), "--modelpath", str(wp), "--noprogress", "--clusters", str(tmp_path / "c.json"),
                 "--cluster-ids", str(tmp_path / "ids.npy"), "--stats", str(tmp_path / "s.json")]) == 0
    assert np.array_equal(np.load(tmp_path / "out.npy"), ref_labels) and (tmp_path / "s.json").exists()
    assert json.load(open(tmp_path / "c.json")) == json.loads(json.dumps(ref))
    ids = np.load(tmp_path / "ids.npy")
    want = cp.find_components(loaded, ref_labels, hu_range=(None, -951), per_label=False, order="size", engine=gpu_engine)
    assert ids.dtype == np.int32 and np.array_equal(ids, want.ids) and ids.max() == ref["lung"]["clusters"]
