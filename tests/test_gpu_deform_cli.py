"""The command line of the deformable registration on the MI355X: --register-deformable --deformation --jacobian write what the
Python calls return, and a run without the new flags writes what it wrote before them."""
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


def test_cli_deformable_round_trip(gpu_engine, tmp_path):
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
    ref_labels, ref = inf.apply_deformable(loaded, loaded_moving, transform="translation")
    det, info = ref.jacobian(engine=gpu_engine)
    common = [str(ip), str(tmp_path / "out.npy"), "--modelpath", str(wp), "--noprogress", "--register-moving", str(mp), "--register-transform",
              "translation"]
    fp, jp, rp, tp = tmp_path / "f.npz", tmp_path / "j.npy", tmp_path / "r.npy", tmp_path / "t.json"
    assert main(common + ["--register-deformable", "--deformation", str(fp), "--jacobian", str(jp), "--registered", str(rp),
                          "--registration", str(tp)]) == 0
    assert np.array_equal(np.load(tmp_path / "out.npy"), ref_labels)
    field = dfm.load(str(fp))
    assert same_bits(field.array, ref.field.array) and field.grid.same_as(rs.Grid.of(loaded))
    assert np.array_equal(field.affine.matrix, ref.affine.matrix) and np.array_equal(field.affine.translation_vector, ref.affine.translation_vector)
    assert same_bits(np.load(jp), det) and same_bits(np.load(rp), ref.image)
    meta = json.load(open(tp))
    assert meta == json.loads(json.dumps(ref.meta())) and meta["folding"]["folded"] == info["folded"] and len(meta["levels"]) == 3
    # the other file types; beside --stats: from the labels it returned
    assert main(common[:1] + [str(tmp_path / "out2.npy")] + common[2:] + ["--register-deformable", "--deformation", str(tmp_path / "f.nii.gz"),
                                                                          "--jacobian", str(tmp_path / "j.nii.gz"), "--stats", str(tmp_path / "s.json")]) == 0
    assert same_bits(dfm.load(str(tmp_path / "f.nii.gz")).array, ref.field.array)
    back = volume_io.load_input_image(str(tmp_path / "j.nii.gz"))
    assert back.array.dtype == np.float32 and same_bits(np.ascontiguousarray(back.array), det)
    # without the new flags every output is what it was: apply_registered's
    old_labels, old = inf.apply_registered(loaded, loaded_moving, transform="translation")
    assert main(common[:1] + [str(tmp_path / "out3.npy")] + common[2:] + ["--registered", str(tmp_path / "r3.npy"), "--registration",
                                                                          str(tmp_path / "t3.json")]) == 0
    assert np.array_equal(np.load(tmp_path / "out3.npy"), old_labels) and np.array_equal(np.load(tmp_path / "r3.npy"), old.image)
    assert json.load(open(tmp_path / "t3.json")) == json.loads(json.dumps(old.meta()))
