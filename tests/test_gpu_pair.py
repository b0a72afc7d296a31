"""The paired analysis on the MI355X: lm_pair_map_dev bit for bit against the numpy restatement of tests/test_pair_emu.py (its
`run_*` cases, plus (9, 130, 301) for many workgroups, twice, into dirty outputs), and LMInferer.apply_pair on the synthetic
lung-like volume and a deformed copy of it: the labels are apply's, and the analysis -- an integer table and maps defined in float64
-- equals, bit for bit, what the emulation library computes from the same volume, labels and field."""
import numpy as np
import pytest

from lungmask_amd import deformable as dfm
from lungmask_amd import pairs
from lungmask_amd import resample as rs
from lungmask_amd import synthetic as syn
from tests import test_pair_emu as cases
from tests.test_deform_emu import DEMONS_DTYPES, FIELDS, SHAPES, SPACING, make_field, rot_scale, same_bits
from tests.test_gpu_field import DEF_KW, REG_KW, SP, known_field

pytestmark = pytest.mark.gpu


def test_pair_cases(gpu_engine):
    for shapes in SHAPES:
        for kind in FIELDS:
            cases.run_pair_cases(gpu_engine, shapes, kind)
    for fdtype in DEMONS_DTYPES:
        for mdtype in DEMONS_DTYPES:
            cases.run_pair_dtypes(gpu_engine, fdtype, mdtype)
    cases.run_label_patterns(gpu_engine)
    cases.run_folded(gpu_engine)
    cases.run_large_sum(gpu_engine)
    cases.run_bounds(gpu_engine)


def test_properties_and_the_mass_pair(gpu_engine):
    cases.run_properties(gpu_engine)
    cases.run_mass_pair(gpu_engine)


def test_many_workgroups_and_dirty_outputs(gpu_engine):
    eng = gpu_engine
    shape = (9, 130, 301)  # 352170 voxels: 172 workgroups of 2048 voxels and a partial one
    assert shape[0] * shape[1] * shape[2] >= 2 * 2048 + 1
    A, b = rot_scale()
    fixed, moving = cases.lungish(shape, np.int16, 60), cases.lungish(shape, np.float32, 61)
    labels = np.random.default_rng(62).integers(0, 18, shape).astype(np.uint8)
    labels[4:, 40:90, 100:200] = 3  # a block of one label: whole waves share it
    field = make_field("special", shape, 63, SPACING)
    kw = dict(spacing=SPACING, jac_scale=abs(float(np.linalg.det(A))), keep=range(0, 256))
    first = cases.check_pair(eng, fixed, labels, moving, field, A, b, 16, **kw)  # (check_pair's outputs start dirty)
    eng.debug_fill_workspaces(0xA5)  # (the call keeps no workspace: nothing changes)
    again = cases.check_pair(eng, fixed, labels, moving, field, A, b, 16, **kw)
    assert first[0] == again[0] and all(same_bits(first[1][k], again[1][k]) for k in cases.MAPS)
    assert all(row[0] > 0 for row in first[0]) and sum(row[2] for row in first[0]) > 0 and sum(row[3] for row in first[0]) > 0


def test_apply_pair(gpu_engine, emu_engine):
    from lungmask_amd.mask import LMInferer

    inf = LMInferer(state_dict=syn.synthetic_state_dict(3, head="lunglike"), engine=gpu_engine)
    vol = syn.phantom(20, 512, 512)
    grid = rs.Grid.of(vol, SP)
    moving = dfm.warp_image(vol, dfm.DisplacementField(known_field(grid), grid), 1, dtype=np.int16, engine=gpu_engine, spacing=SP)
    moving = moving.array if hasattr(moving, "array") else moving
    labels, r, pair = inf.apply_pair(vol, moving, spacing=SP, moving_spacing=SP, register_kw=REG_KW, deformable_kw=DEF_KW, roles=None,
                                     hu_range=(-1000, -300))
    assert (labels > 0).sum() > 10 ** 4 and np.array_equal(labels, inf.apply(vol))
    assert r.field.array.shape == (3,) + vol.shape and r.field_dev is None and r.image.shape == vol.shape
    n_labels, names = inf._model_labels(None)
    kw = dict(roles=None, hu_range=(-1000, -300), n_labels=n_labels, names=names, spacing=SP, moving_spacing=SP)
    same = lambda a, b: a.analysis == b.analysis and np.array_equal(a.table, b.table) and same_bits(a.classes, b.classes) and \
        same_bits(a.change, b.change) and same_bits(a.jacobian, b.jacobian)  # noqa: E731
    assert same(pair, pairs.pair_analysis(vol, moving, labels, r, engine=gpu_engine, **kw))
    assert same(pair, pairs.pair_analysis(vol, moving, labels, r, engine=emu_engine, **kw))
    lung = pair.analysis["lung"]
    print(f"apply_pair: {lung['voxels']} lung voxels, {lung['analysed']} analysed, {lung['outside']} outside, {lung['folded']} folded; mean Jacobian "
          f"{lung['mean_jacobian']:.4f}, mean change {lung['mean_change_hu']:.2f} HU, rms {lung['rms_change_hu']:.2f} HU; classes "
          f"{ {k: v['voxels'] for k, v in lung['classes'].items()} }")
    assert lung["voxels"] == int((labels > 0).sum()) and lung["analysed"] > 0.9 * lung["voxels"] and lung["classified"] > 0
    assert pair.analysis["transform"] == "deformable" and pair.class_names == ("neither", "fixed_only", "moving_only", "both")
    # the affine stage alone
    labels2, r2, pair2 = inf.apply_pair(vol, moving, deformable=False, spacing=SP, moving_spacing=SP, register_kw=REG_KW, maps=("classes",))
    assert np.array_equal(labels2, labels) and pair2.change is None and pair2.analysis["transform"] == "affine"
    want = pairs.pair_analysis(vol, moving, labels, r2, maps=("classes",), n_labels=n_labels, names=names, spacing=SP, moving_spacing=SP,
                               engine=emu_engine)
    assert pair2.analysis == want.analysis and same_bits(pair2.classes, want.classes)
