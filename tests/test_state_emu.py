"""CPU suite: results do not depend on what an engine did before, nor on where the caller's buffers lie (tests/state_cases.py), on
the emulator.  Everything is compared with the first call of a new engine, byte for byte.  The network entry points run at one tiny
shape here (an emulated forward takes ten seconds and more); the GPU module runs all of them."""
import ctypes as C

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
            "nearest_label", "fuse_spare"} <= set(sc.ENQUEUE_ONLY)


@pytest.mark.parametrize("name", PARAMS)
def test_red_zones(base, name):
    sc.check_red_zones(base, name)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("name", [p for p in PARAMS if sc.BY_NAME[p if isinstance(p, str) else p.values[0]].emu_shapes["vec"]])
def test_misaligned_bases(base, name, k):
    sc.check_red_zones(base, name, k)
