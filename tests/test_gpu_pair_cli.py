"""The command line of the paired analysis on the MI355X: --pair, --pair-classes and --pair-change with --pair-roles,
--pair-thresholds and --pair-range write what LMInferer.apply_pair returns."""
import json

import numpy as np
import pytest
import torch

from lungmask_amd import resample as rs
from lungmask_amd import synthetic as syn
from lungmask_amd import volume_io
from tests.test_deform_emu import same_bits

pytestmark = pytest.mark.gpu


def test_cli_pair(gpu_engine, tmp_path):
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
    ref_labels, _, ref = inf.apply_pair(loaded, loaded_moving, deformable=False, transform="translation", roles=None, fixed_threshold=-900.0,
                                        moving_threshold=-910.0, hu_range=(-1000.0, -300.0), maps=("classes", "change"))
    jp, cp, dp = tmp_path / "pair.json", tmp_path / "classes.nii.gz", tmp_path / "change.npy"
    assert main([str(ip), str(tmp_path / "out.npy"), "--modelpath", str(wp), "--noprogress", "--register-moving", str(mp), "--register-transform",
                 "translation", "--pair", str(jp), "--pair-classes", str(cp), "--pair-change", str(dp), "--pair-roles", "longitudinal",
                 "--pair-thresholds", "-900", "-910", "--pair-range", "-1000", "-300"]) == 0
    assert np.array_equal(np.load(tmp_path / "out.npy"), ref_labels) and (ref_labels > 0).sum() > 10 ** 4
    assert json.load(open(jp)) == ref.analysis and ref.analysis["lung"]["classified"] > 0 and ref.analysis["transform"] == "affine"
    back = volume_io.load_input_image(str(cp))
    assert back.array.dtype == np.uint8 and np.array_equal(back.array, ref.classes) and rs.Grid.of(back).same_as(grid)
    assert same_bits(np.load(dp), ref.change)
