"""The command line of the inverse transform on the MI355X: --inverse-deformation and --labels-on-moving write what
LMInferer.apply_deformable(..., inverse=True) returns, and a run without them writes what it wrote before them."""
import json

import numpy as np
import pytest
import torch

from lungmask_amd import deformable as dfm
from lungmask_amd import resample as rs
from lungmask_amd import synthetic as syn
from lungmask_amd import volume_io
from tests.test_deform_emu import same_bits

pytestmark = pytest.mark.gpu


def test_cli_inverse_round_trip(gpu_engine, tmp_path):
    from lungmask_amd import LMInferer
    from lungmask_amd.__main__ import main

    sd = syn.synthetic_state_dict(3, head="lunglike")
    wp = tmp_path / "w.pth"
    torch.save(sd, wp)
    img = volume_io.Volume(syn.phantom(20, 512, 512), (0.75, 0.75, 2.0), (1.0, 2.0, 3.0))
    grid = rs.Grid.of(img)
    moving = grid.like(rs.resample_image(img, grid, rs.Affine.translation((-2.0, 3.0, 0.0)), order=1, dtype=np.int16, engine=gpu_engine).array)
    ip, mp = tmp_path / "in.nii.gz", tmp_path / "moving.nii.gz"
    volume_io.write_nifti(str(ip), img)
    volume_io.write_nifti(str(mp), moving)
    loaded, loaded_moving = volume_io.load_input_image(str(ip)), volume_io.load_input_image(str(mp))
    inf = LMInferer(modelpath=str(wp), engine=gpu_engine)
    ref_labels, ref = inf.apply_deformable(loaded, loaded_moving, transform="translation", inverse=True)
    common = [str(ip), str(tmp_path / "out.npy"), "--modelpath", str(wp), "--noprogress", "--register-moving", str(mp), "--register-transform",
              "translation", "--register-deformable"]
    vp, lp, fp, tp = tmp_path / "inv.npz", tmp_path / "lm.nii.gz", tmp_path / "f.npz", tmp_path / "t.json"
    assert main(common + ["--inverse-deformation", str(vp), "--labels-on-moving", str(lp), "--deformation", str(fp), "--registration", str(tp)]) == 0
    assert np.array_equal(np.load(tmp_path / "out.npy"), ref_labels)
    inv = dfm.load(str(vp))
    assert same_bits(inv.array, ref.inverse_field.array) and inv.grid.same_as(rs.Grid.of(loaded_moving))
    assert np.array_equal(inv.affine.matrix, ref.affine.inverse().matrix)
    assert np.array_equal(inv.affine.translation_vector, ref.affine.inverse().translation_vector)
    back = volume_io.load_input_image(str(lp))
    assert back.array.dtype == np.uint8 and np.array_equal(back.array, ref.labels_on_moving) and rs.Grid.of(back).same_as(rs.Grid.of(loaded_moving))
    assert (ref.labels_on_moving > 0).sum() > 10 ** 4
    meta = json.load(open(tp))
    assert meta == json.loads(json.dumps(ref.meta())) and meta["inverse"]["converged"] is True
    assert same_bits(dfm.load(str(fp)).array, ref.field.array)
    # one flag alone, the other file types; beside --stats: from the labels it returned
    assert main(common[:1] + [str(tmp_path / "out2.npy")] + common[2:] + ["--labels-on-moving", str(tmp_path / "lm.npy"), "--inverse-deformation",
                                                                          str(tmp_path / "inv.nii.gz"), "--stats", str(tmp_path / "s.json")]) == 0
    assert np.array_equal(np.load(tmp_path / "lm.npy"), ref.labels_on_moving)
    assert same_bits(dfm.load(str(tmp_path / "inv.nii.gz")).array, ref.inverse_field.array)
    # without the new flags every output is what it was
    old_labels, old = inf.apply_deformable(loaded, loaded_moving, transform="translation")
    assert main(common[:1] + [str(tmp_path / "out3.npy")] + common[2:] + ["--deformation", str(tmp_path / "f3.npz"), "--registration",
                                                                          str(tmp_path / "t3.json")]) == 0
    assert np.array_equal(np.load(tmp_path / "out3.npy"), old_labels) and same_bits(dfm.load(str(tmp_path / "f3.npz")).array, old.field.array)
    plain = json.load(open(tmp_path / "t3.json"))
    assert "inverse" not in plain and plain == json.loads(json.dumps(old.meta())) and same_bits(old.field.array, ref.field.array)
    assert {k: v for k, v in meta.items() if k != "inverse"} == plain
