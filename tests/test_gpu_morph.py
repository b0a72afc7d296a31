"""Label morphology on the MI355X: lm_nearest_label_dev and lm_morph_dev bit for bit against the numpy oracle of
tests/test_morph_emu.py (its tie inputs included) on the smallest shapes that reach each code path, the device forms against the host
forms, LMInferer.apply_closed (R231, the fused mode, several engines) and the CLI's --closed / --close-mm round trip."""
import numpy as np
import pytest
import torch

from lungmask_amd import morphology as morph
from lungmask_amd import synthetic as syn
from lungmask_amd import volume_io
from tests.test_metrics_emu import WORD_SPACINGS, bits, word_boundary_rows
from tests.test_morph_emu import OPS, check_nearest, check_op, oracle_morph, oracle_nearest, random_labels, table, tie_volume

pytestmark = pytest.mark.gpu

ANISO = (2.5, 0.7421875, 0.7421875)
# six labels and an anisotropic spacing; several ballot words; a line so long that a tile holds fewer than 32 columns; skipped axes;
# odd widths
SHAPES = [(24, 90, 136), (6, 40, 264), (1, 600, 40), (33, 1, 130), (1, 1, 70), (7, 33, 70)]


@pytest.mark.parametrize("shape", SHAPES)
def test_nearest_label(gpu_engine, shape):
    rng = np.random.default_rng(sum(shape))
    lab = random_labels(rng, shape, n_labels=7)
    check_nearest(gpu_engine, lab, None, ANISO, "random")
    check_nearest(gpu_engine, lab, [2, 5], (0.625, 0.71, 0.83), "labels outside keep")
    ties, want = tie_volume(shape)
    for spacing in (None, ANISO):
        near = check_nearest(gpu_engine, ties, None, spacing, "ties")
        for v, k in want:
            if spacing is None or oracle_nearest(ties, None, spacing)[1][v] == k:  # unit spacing: every tie is exact
                assert near[v] == k, (v, near[v], k)


@pytest.mark.parametrize("spacing", WORD_SPACINGS)
def test_nearest_label_word_boundaries(gpu_engine, spacing):
    check_nearest(gpu_engine, word_boundary_rows((5, 2, 7, 3)), None, spacing, "word boundaries")


@pytest.mark.parametrize("shape", SHAPES)
def test_operators(gpu_engine, shape):
    rng = np.random.default_rng(50 + sum(shape))
    lab = random_labels(rng, shape, n_labels=7)
    ties, _ = tie_volume(shape)
    for op in OPS:
        check_op(gpu_engine, lab, op, 2.3, ANISO, None, (0,), "random")
        check_op(gpu_engine, lab, op, np.sqrt(5.0), None, [2, 5], (0, 1, 3), "keep subset, into may overwrite 1 and 3")
        check_op(gpu_engine, ties, op, 3.0, None, None, (0,), "ties")
    got, changed = gpu_engine.morph(lab, "dilate", np.inf, spacing=ANISO, keep=[1, 2], into=(0, 3))
    want, wchanged = oracle_morph(lab, "dilate", np.inf, ANISO, [1, 2], (0, 3))
    assert np.array_equal(got, want) and changed == wchanged
    m = np.isin(lab, (0, 3))
    assert np.array_equal(got[m], oracle_nearest(lab, [1, 2], ANISO)[1][m])


def test_device_forms_equal_host_forms(gpu_engine):
    rng = np.random.default_rng(3)
    lab = random_labels(rng, (7, 33, 70), n_labels=7)
    ld = gpu_engine.to_device(lab)
    near, d2 = gpu_engine.nearest_label_dev(ld, ANISO, [1, 4], return_distance=True)
    gpu_engine.sync()
    hn, hd = gpu_engine.nearest_label(lab, ANISO, [1, 4], return_distance=True)
    assert np.array_equal(near.download(), hn) and np.array_equal(bits(d2.download()), bits(hd))
    assert np.array_equal(bits(hd), bits(gpu_engine.edt(table([1, 4])[lab].astype(np.uint8), ANISO)))
    for op in OPS:
        out, changed = gpu_engine.morph_dev(ld, op, 2.0, spacing=ANISO)
        gpu_engine.sync()
        host, hchanged = gpu_engine.morph(lab, op, 2.0, spacing=ANISO)  # (in place on its own copy)
        assert out is not ld and np.array_equal(out.download(), host) and changed == hchanged, op
        assert np.array_equal(ld.download(), lab)
        assert np.array_equal(getattr(morph, "open_" if op == "open" else op)(lab, 2.0, spacing=ANISO, engine=gpu_engine), host)
        out.free()
    assert np.array_equal(morph.propagate(lab, engine=gpu_engine), gpu_engine.morph(lab, "dilate", np.inf)[0])
    for d in (ld, near, d2):
        d.free()


@pytest.mark.parametrize("model", ["R231", "LTRCLobes_R231"])
def test_apply_closed(gpu_engine, model):
    from lungmask_amd.mask import LMInferer

    fused = model == "LTRCLobes_R231"
    kw = dict(modelname="LTRCLobes" if fused else model, state_dict=syn.synthetic_state_dict(6 if fused else 3, head="lunglike"),
              fillmodel="R231" if fused else None, fill_state_dict=syn.synthetic_state_dict(3, head="lunglike") if fused else None)
    inf = LMInferer(engine=gpu_engine, **kw)
    vol = syn.phantom(24, 512, 512)
    expect = inf.apply(vol).copy()
    assert (expect > 0).sum() > 10 ** 4
    sp = (2.0, 0.75, 0.75)
    labels, closed = inf.apply_closed(vol, radius_mm=6.0, spacing=sp)
    assert np.array_equal(labels, expect)
    assert np.array_equal(closed, morph.close(expect, 6.0, spacing=sp, engine=gpu_engine))
    assert np.array_equal(closed[expect > 0], expect[expect > 0])  # extensive
    img = volume_io.Volume(vol, sp[::-1], (1.0, 2.0, 3.0))
    labels2, closed2 = inf.apply_closed(img, radius_mm=6.0)  # the image's own spacing
    assert np.array_equal(labels2, expect) and np.array_equal(closed2, closed)
    with pytest.raises(ValueError, match="spacing"):
        inf.apply_closed(img, spacing=sp)


def test_apply_closed_several_engines(gpu_engine):
    from lungmask_amd.mask import LMInferer

    sd = syn.synthetic_state_dict(3, head="lunglike")
    vol = syn.phantom(24, 512, 512)
    lab1, c1 = LMInferer(state_dict=sd, engine=gpu_engine).apply_closed(vol, radius_mm=4.0, spacing=(2.0, 0.8, 0.8))
    inf = LMInferer(state_dict=sd, device_ids=[0, 0])
    try:
        lab2, c2 = inf.apply_closed(vol, radius_mm=4.0, spacing=(2.0, 0.8, 0.8))
    finally:
        inf.close()
    assert np.array_equal(lab2, lab1) and np.array_equal(c2, c1)


def test_cli_closed(gpu_engine, tmp_path):
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
    ref_labels, ref_closed = inf.apply_closed(loaded)
    ref_labels = ref_labels.copy()
    cp = tmp_path / "closed.nii.gz"
    assert main([str(ip), str(tmp_path / "out.npy"), "--modelpath", str(wp), "--noprogress", "--closed", str(cp)]) == 0
    assert np.array_equal(np.load(tmp_path / "out.npy"), ref_labels)
    back = volume_io.load_input_image(str(cp))
    assert np.array_equal(np.asarray(back.array), ref_closed)
    np.testing.assert_allclose(back.spacing, loaded.spacing, atol=1e-6)
    assert np.array_equal(ref_closed, morph.close(loaded.like(ref_labels), 10.0, engine=gpu_engine))
    # another radius, beside --stats, into another container
    assert main([str(ip), str(tmp_path / "out2.npy"), "--modelpath", str(wp), "--noprogress", "--closed", str(tmp_path / "c.npy"),
                 "--close-mm", "4", "--stats", str(tmp_path / "s.json")]) == 0
    assert np.array_equal(np.load(tmp_path / "out2.npy"), ref_labels) and (tmp_path / "s.json").exists()
    assert np.array_equal(np.load(tmp_path / "c.npy"), morph.close(loaded.like(ref_labels), 4.0, engine=gpu_engine))
