"""CPU suite: results do not depend on what an engine did before, nor on where the caller's buffers lie (tests/state_cases.py), on
the emulator.  Everything is compared with the first call of a new engine, byte for byte.  The network entry points run at one tiny
shape here (an emulated forward takes ten seconds and more); the GPU module runs all of them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import state_cases as sc
from lungmask_amd import _native as nat

NAMES = sc.names(gpu=False)
SLOW = {"forward_split_f16_logp"}
PARAMS = [pytest.param(n, marks=pytest.mark.slow) if n in SLOW else n for n in NAMES]


@pytest.fixture(scope="module")
def base(emu_engine):
    return sc.Baselines(emu_engine.L, gpu=False)


def test_seam_refuses_an_open_slab_exchange_and_bad_bytes(emu_engine):
    lib = emu_engine.L
    eng = nat.Engine(0, lib)
    try:
        assert eng.debug_fill_workspaces(0) == 0  # nothing allocated yet
        for byte in (-1, 256):
            with pytest.raises(nat.LMError):
                eng.debug_fill_workspaces(byte)
        d = eng.to_device(sc.blob_labels((4, 16, 16)))
        eng.L.check(lib.lib.lm_slab_begin(eng.h, d.ptr, 4, 16, 16, 0, 1, 0, 4, (C.c_int * 1)(0), 0, 3), "lm_slab_begin")
        with pytest.raises(nat.LMError, match="slab exchange is open"):
            eng.debug_fill_workspaces(0x5A)
    finally:
        eng.close()


def test_guard_bands_notice_a_stray_write(emu_engine):
    """The arena's own check: a byte written behind an output view, and a changed input, are both reported."""
    eng = nat.Engine(0, emu_engine.L)
    try:
        for victim in ("guard", "input"):
            mem = sc.ArenaMem(eng, 0, 1 << 20)
            a = mem.inp(sc.blob_labels((2, 8, 8)))
            o = mem.out((2, 8, 8), "uint8")
            where = o.ptr + o.nbytes if victim == "guard" else a.ptr + 5
            eng.L.check(eng.L.lib.lm_copy_h2d(eng.h, where, (C.c_uint8 * 1)(7), 1), "lm_copy_h2d")
            with pytest.raises(AssertionError, match="outside the outputs changed"):
                mem.finish()
            mem.close()
    finally:
        eng.close()


@pytest.mark.parametrize("name", PARAMS)
def test_dirty_workspace(base, name):
    sc.check_dirty_workspace(base, name)


def test_call_order(base):
    sc.check_call_order(base, [n for n in NAMES if n not in SLOW])


def test_deferred_by_one(base):
    """The emulator's streams are synchronous: this run checks the harness of the deferred collection (every case enqueued, the next
    one's dirtying shape enqueued, only then collected), not the ordering on a device -- tests/test_gpu_state.py does that."""
    sc.check_deferred(base, [n for n in NAMES if n not in SLOW])


def test_enqueue_only_table_names_cases():
    assert set(sc.ENQUEUE_ONLY) <= set(sc.BY_NAME) and all(len(v) == 2 and all(v) for v in sc.ENQUEUE_ONLY.values())
    assert {"forward_f32_logp", "forward_batches_f32", "apply_f32", "reshape_mask", "uncrop_probs", "reorient", "edt", "filter_whole",
            "nearest_label", "fuse_spare", "spline_prefilter", "resample_linear", "resample_cubic", "resample_labels", "joint_hist", "warp",
            "demons_step", "jacobian", "lcc", "field_combine", "pair_map", "hessian", "vesselness"} <= set(sc.ENQUEUE_ONLY)
    # (each ends in, or is interleaved with, a call that reads counts back)
    assert not {"vesselness_masked", "skeleton", "airway"} & set(sc.ENQUEUE_ONLY)


# The declared entry points that are not the subject of a case: name -> where they are covered instead.  The `_dev` forms need a reason
# to be here; the others are listed so that the sentence "one case per device entry point" says what it leaves out.
NOT_A_CASE = {
    "lm_slab_begin": "the slab_protocol case drives the whole exchange through pipeline.postprocess_slabs_in_process (its device buffers are the protocol's own)",
    "lm_slab_pending": "as lm_slab_begin",
    "lm_slab_pending_uniform": "as lm_slab_begin",
    "lm_slab_emit": "as lm_slab_begin",
    "lm_slab_step": "as lm_slab_begin",
    "lm_pipe_upload": "host buffers in, host buffers out, resident volumes that ARE state between calls: tests/test_gpu_apply.py (ordering on the device included)",
    "lm_pipe_apply": "as lm_pipe_upload",
    "lm_pipe_download": "as lm_pipe_upload",
    "lm_pipe_wait": "as lm_pipe_upload",
    "lm_pipe_query": "as lm_pipe_upload",
    "lm_component_table_launch": "host arithmetic only (the launch plan of lm_component_table_dev): tests/test_components_emu.py",
    "lm_seed_cost_bricks": "host arithmetic only (the tiling of lm_seed_cost_dev): tests/test_airway_emu.py",
}


def declared_entry_points():
    """Every function name declared in include/lungmask_hip.h (comments stripped: they quote calls)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "lungmask_hip.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return set(re.findall(r"\b(lm_\w+)\s*\(", text))


def test_every_device_entry_point_has_a_case():
    declared = declared_entry_points()
    assert len(declared) > 60 and "lm_forward_dev" in declared and "lm_airway_mask_dev" in declared  # (the parse itself)
    named = {e for c in sc.CASES for e in c.entries}
    unknown = sorted((named | set(NOT_A_CASE)) - declared)
    assert not unknown, f"not declared in include/lungmask_hip.h: {unknown}"
    assert all(c.entries for c in sc.CASES if c.name != "slab_protocol"), "a case without entries"
    assert not named & set(NOT_A_CASE) and all(NOT_A_CASE.values())
    missing = sorted(e for e in declared if e.endswith("_dev") and e not in named and e not in NOT_A_CASE)
    assert not missing, f"device entry points without a case in tests/state_cases.py (or a reason in NOT_A_CASE): {missing}"


def test_optional_outputs_of_the_wrappers(emu_engine):
    """eig_out / scale_out / d2_out / index_out, code_out, d2_out: the caller's arrays receive what the wrapper otherwise allocates,
    bit for bit, and get the checks of `out=`."""
    eng, shape, sig = emu_engine, (3, 9, 20), (0.5, 0.5, 0.5)
    with eng.scope() as dev:
        vol = dev.upload(sc._vessel_volume(shape, np.int16, 1))
        sel = dev.upload(sc._skeleton_volume(shape, 2))
        comp, eig = dev.add(*eng.hessian_dev(vol, sig, eigenvalues=True))
        mine = dev.empty((3,) + shape, np.float32)
        assert eng.hessian_dev(vol, sig, out=comp, eig_out=mine)[1] is mine and mine.download().tobytes() == eig.download().tobytes()
        v, scale = dev.add(*eng.vesselness_dev(vol, [sig], return_scale=True))
        mine = dev.empty(shape, np.uint8)
        assert eng.vesselness_dev(vol, [sig], out=v, scale_out=mine)[1] is mine and np.array_equal(mine.download(), scale.download())
        skel = dev.add(eng.skeleton_dev(sel)[0])
        cls, counts, d2 = eng.calibre_dev(skel, sel, (1.0,), return_distance=True)
        dev.add(cls, d2)
        mine = dev.empty(shape, np.float32)
        assert eng.calibre_dev(skel, sel, (1.0,), out=cls, d2_out=mine)[2] is mine and mine.download().tobytes() == d2.download().tobytes()
        idx, code, pd2, total = eng.skeleton_points_dev(skel, d2)
        assert total == idx.size > 2
        outs = dev.empty((total,), np.int32), dev.empty((total,), np.uint8), dev.empty((total,), np.float32)
        got = eng.skeleton_points_dev(skel, d2, index_out=outs[0], code_out=outs[1], d2_out=outs[2])
        assert got[3] == total and all(np.array_equal(a, b) and np.array_equal(o.download(), b) for a, b, o in zip(got[:3], (idx, code, pd2), outs))
        assert np.array_equal(eng.skeleton_points_dev(skel, cap=2, index_out=outs[0], code_out=outs[1])[0], idx[:2])
        for call in (lambda: eng.hessian_dev(vol, sig, eig_out=dev.empty((6,) + shape, np.float32)),
                     lambda: eng.hessian_dev(vol, sig, eig_out=dev.empty((3,) + shape, np.float64)),
                     lambda: eng.vesselness_dev(vol, [sig], scale_out=dev.empty(shape, np.float32)),
                     lambda: eng.vesselness_dev(vol, [sig], scale_out=dev.empty((1,) + shape, np.uint8)),
                     lambda: eng.calibre_dev(skel, sel, (1.0,), d2_out=dev.empty(shape, np.uint8)),
                     lambda: eng.calibre_dev(skel, sel, (1.0,), d2_out=dev.empty(shape[1:], np.float32)),
                     lambda: eng.skeleton_points_dev(skel, index_out=outs[0]),
                     lambda: eng.skeleton_points_dev(skel, index_out=outs[0], code_out=outs[1], d2_out=outs[2]),  # (d2_out without d2)
                     lambda: eng.skeleton_points_dev(skel, d2, index_out=outs[0], code_out=outs[1]),
                     lambda: eng.skeleton_points_dev(skel, index_out=outs[0], code_out=dev.empty((total + 1,), np.uint8)),
                     lambda: eng.skeleton_points_dev(skel, index_out=outs[0], code_out=dev.empty((total,), np.int32)),
                     lambda: eng.skeleton_points_dev(skel, cap=total + 1, index_out=outs[0], code_out=outs[1])):
            with pytest.raises(nat.LMError, match="eig_out|scale_out|d2_out|index_out"):
                call()


def test_new_cases_reach_their_edges(base):
    """What the cases of the sampling and registration families are there for, read off the baselines: samples outside the moving
    volume, non-finite values, a folding field, thinning that deletes, a flood that crosses brick faces."""
    for i, shape in enumerate(sc.BY_NAME["joint_hist"].shapes("small", gpu=False)):
        counts = base("joint_hist")[i][0][-4:]
        assert counts[0] == counts[1:].sum() and counts[1] > 0 and counts[2] > 0, (shape, counts)  # sampled = contributed + outside + nan
        c = base("demons_step")[i][1]
        assert c[0] == c[1] + c[2] + c[3] and c[1] > 0 and c[2] > 0, (shape, c)
        c = base("lcc")[i][2]
        assert c[0] == c[1] + c[2] + c[3] and c[1] > 0 and c[2] > 0 and c[3] > 0, (shape, c)
        det, c = base("jacobian")[i]
        assert 0 < c[0] < det.size, (shape, c)  # folded somewhere, not everywhere
        assert base("field_combine")[i][1][0] > 0, shape  # sampled outside `src`
        table = base("pair_map")[i][0]
        assert (table[1:, 0] > 0).all() and table[:, 1].sum() > 0 and table[:, 2].sum() > 0, (shape, table)
        for name in ("resample_linear", "resample_cubic", "resample_labels"):
            out = base(name)[i][0]
            assert (out[:, 0] == 3).all() and not (out == 3).all(), (name, shape)  # the first row is the fill, the rest is not
        kd, info = base("skeleton")[i][:2]
        assert 0 < info["skeleton"] < info["selected"] and info["passes"] > 1 and base("skeleton")[i][8] == info["skeleton"], (shape, info)
        info = base("airway")[i][2]
        assert info["converged"] and info["seeds_passable"] == 2 and 2 * info["reached"] > np.prod(shape), (shape, info)
        v, s, counts, mask = base("vesselness_masked")[i]
        assert counts.sum() == mask.sum() > 0, shape


@pytest.mark.parametrize("name", PARAMS)
def test_red_zones(base, name):
    sc.check_red_zones(base, name)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("name", [p for p in PARAMS if sc.BY_NAME[p if isinstance(p, str) else p.values[0]].emu_shapes["vec"]])
def test_misaligned_bases(base, name, k):
    sc.check_red_zones(base, name, k)
