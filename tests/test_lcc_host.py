"""The host side of the local-correlation metric: the refusals of lm_local_moments_dev, lm_lcc_step_dev and of the Python layers
above them, the sequence of engine calls of `register_deformable` -- `metric="ssd"` is the sequence from before the metric
argument existed, `metric="lcc"` one warp, the window sums and one step per iteration --, and the command line's two flags."""
import numpy as np
import pytest

import lungmask_amd.__main__ as cli
from lungmask_amd import _native as nat
from lungmask_amd import deformable as dfm
from tests.test_cli_refusals import DEFORM, MOVING, PAIR_KW, Called, Recorder


# ------------------------------------------------------------------------------------------------ argument refusals
def test_entry_point_refusals(emu_engine):
    eng = emu_engine
    lib = eng.L.lib
    I, z = np.eye(3), np.zeros(3)
    shape = (2, 3, 4)
    with eng.scope() as dev:
        f, m = dev.upload(np.zeros(shape, np.float32)), dev.upload(np.ones(shape, np.float32))
        S, u, v, counts = dev.empty((6,) + shape, np.float64), dev.upload(np.zeros((3,) + shape, np.float32)), dev.empty((3,) + shape, np.float32), dev.empty((6,), np.int64)
        # the window
        for bad in (9, (1, 2, 9), -1):
            with pytest.raises(ValueError, match=r"0 \.\. 8"):
                eng.local_moments_dev(f, m, bad)
        with pytest.raises(ValueError, match="whole number"):
            eng.local_moments_dev(f, m, 1.5)
        with pytest.raises(ValueError, match="whole number"):
            eng.local_moments_dev(f, m, (1, 2))
        r = (nat.C.c_int32 * 3)(1, 9, 1)
        assert lib.lm_local_moments_dev(eng.h, f.ptr, m.ptr, 2, 3, 4, r, S.ptr) < 0 and b"radius[1] = 9 must lie in 0 .. 8" in lib.lm_last_error()
        r = (nat.C.c_int32 * 3)(1, 1, 1)
        # NULL pointers, dimension limits (no pointer is followed), aliasing
        assert lib.lm_local_moments_dev(eng.h, f.ptr, None, 2, 3, 4, r, S.ptr) < 0 and b"not NULL" in lib.lm_last_error()
        assert lib.lm_local_moments_dev(eng.h, f.ptr, m.ptr, 2, 3, 4, None, S.ptr) < 0 and b"not NULL" in lib.lm_last_error()
        assert lib.lm_local_moments_dev(eng.h, 8, 8, 1, 1, 4097, r, 16) < 0 and b"4096" in lib.lm_last_error()
        assert lib.lm_local_moments_dev(eng.h, 8, 8, 2048, 1024, 1024, r, 16) < 0
        assert lib.lm_local_moments_dev(eng.h, S.ptr + 64, m.ptr, 2, 3, 4, r, S.ptr) < 0 and b"overlap" in lib.lm_last_error()
        # dtypes and shapes
        with pytest.raises(nat.LMError, match="float32"):
            eng.local_moments_dev(dev.upload(np.zeros(shape, np.int16)), m, 1)
        with pytest.raises(nat.LMError, match="one grid"):
            eng.local_moments_dev(f, dev.upload(np.zeros((2, 3, 5), np.float32)), 1)
        with pytest.raises(nat.LMError, match="float64"):
            eng.local_moments_dev(f, m, 1, out=dev.empty((6,) + shape, np.float32))
        # the step
        with pytest.raises(nat.LMError, match="in-place"):
            eng.lcc_step_dev(f, m, S, u, u, counts, I, z, shape)
        with pytest.raises(nat.LMError, match="moments must be"):
            eng.lcc_step_dev(f, m, dev.empty((5,) + shape, np.float64), u, v, counts, I, z, shape)
        with pytest.raises(nat.LMError, match="six values"):
            eng.lcc_step_dev(f, m, S, u, v, dev.empty((5,), np.int64), I, z, shape)
        with pytest.raises(nat.LMError, match="field must be"):
            eng.lcc_step_dev(f, m, S, dev.upload(np.zeros((3, 2, 3, 5), np.float32)), v, counts, I, z, shape)
        with pytest.raises(nat.LMError, match="labels"):
            eng.lcc_step_dev(f, m, S, u, v, counts, I, z, shape, labels=dev.upload(np.zeros((2, 3, 5), np.uint8)))
        for kw in (dict(inv_k2=-1.0), dict(den_min=float("nan")), dict(var_eps=-1.0), dict(a_max=0.0), dict(a_max=float("inf")), dict(spacing=(1.0, 0.0, 1.0))):
            with pytest.raises((nat.LMError, ValueError), match="finite|spacing"):
                eng.lcc_step_dev(f, m, S, u, v, counts, I, z, shape, **kw)
        with pytest.raises(nat.LMError, match="4096"):
            eng.lcc_step_dev(f, m, S, u, v, counts, I, z, (1, 1, 4097))
        p = nat.LccParams()
        p.moving_dims[:] = [2, 3, 4]
        p.a_max = 4.0
        p.field_scale[:] = [1.0] * 3
        assert lib.lm_lcc_step_dev(eng.h, f.ptr, m.ptr, S.ptr, None, 2, 3, 4, u.ptr, p, u.ptr, counts.ptr) < 0 and b"in-place" in lib.lm_last_error()
        assert lib.lm_lcc_step_dev(eng.h, f.ptr, m.ptr, S.ptr, None, 2, 3, 4, u.ptr, p, S.ptr, counts.ptr) < 0 and b"overlap" in lib.lm_last_error()
        assert lib.lm_lcc_step_dev(eng.h, f.ptr, m.ptr, S.ptr, None, 2, 3, 4, u.ptr, p, None, counts.ptr) < 0 and b"not NULL" in lib.lm_last_error()
        assert lib.lm_lcc_step_dev(eng.h, f.ptr, m.ptr, S.ptr, None, 2, 3, 4, u.ptr, None, v.ptr, counts.ptr) < 0 and b"not NULL" in lib.lm_last_error()
        assert lib.lm_lcc_step_dev(eng.h, f.ptr, m.ptr, S.ptr, None, 2, 3, 4, u.ptr, p, v.ptr, counts.ptr) == 0
        eng.sync()


def test_register_deformable_refusals():
    vol = np.zeros((3, 4, 5), np.int16)
    with pytest.raises(ValueError, match="metric: one of"):
        dfm.register_deformable(vol, vol, metric="ncc")
    with pytest.raises(ValueError, match="window_mm"):
        dfm.register_deformable(vol, vol, metric="lcc", window_mm=0.0)
    with pytest.raises(ValueError, match="window_mm"):
        dfm.register_deformable(vol, vol, metric="lcc", window_mm=(1.0, 2.0))
    with pytest.raises(ValueError, match="var_eps"):
        dfm.register_deformable(vol, vol, metric="lcc", var_eps=-1.0)
    with pytest.raises(ValueError, match="a_max"):
        dfm.register_deformable(vol, vol, a_max=0.0)
    assert dfm.METRICS == ("ssd", "lcc") and (dfm.WINDOW_LEVEL_VOXELS, dfm.VAR_EPS, dfm.A_MAX) == (4, 25.0, 4.0)


def test_a_window_above_the_limit_is_refused_before_anything_runs(emu_engine):
    vol = np.zeros((6, 8, 10), np.int16)
    log = Log(emu_engine)
    with pytest.raises(ValueError, match="limit is 8 voxels"):
        dfm.register_deformable(vol, vol, metric="lcc", window_mm=9.0, levels_mm=(2.0, 1.0), iterations=(1, 1), engine=log)  # 9 voxels at 1 mm
    assert log.calls == []


# ------------------------------------------------------------------------------------------------ the sequence of engine calls
COMPUTE = ("filter_dev", "resample_dev", "warp_dev", "demons_step_dev", "local_moments_dev", "lcc_step_dev", "jacobian_dev")


class Log:
    """An engine that records the names of the compute calls it passes on."""

    def __init__(self, eng):
        self._eng, self.calls = eng, []

    def __getattr__(self, name):
        attr = getattr(self._eng, name)
        if name in COMPUTE:
            def call(*a, **kw):
                self.calls.append(name)
                return attr(*a, **kw)
            return call
        return attr


def expected_calls(step, iterations):
    """The calls of a two-level registration whose levels run `iterations` without an early stop; `step`: the calls of one step."""
    to_level = ["filter_dev", "resample_dev"] * 2
    iteration = step + ["filter_dev"] * 3
    return (to_level + iteration * iterations[0]                                          # the first level, from zeros
            + to_level + ["resample_dev"] * 3 + step + iteration * iterations[1] + step   # the last one, between its two metrics
            + ["resample_dev"] * 3 + ["jacobian_dev"])                                    # onto the fixed grid


def test_call_sequences(emu_engine):
    rng = np.random.default_rng(3)
    fixed = rng.normal(-600.0, 200.0, (8, 10, 12)).astype(np.int16)
    moving = rng.normal(-600.0, 200.0, (8, 10, 12)).astype(np.int16)
    kw = dict(levels_mm=(4.0, 2.0), iterations=(2, 3), patience=10)
    ssd = expected_calls(["demons_step_dev"], kw["iterations"])
    runs = {}
    for name, extra in (("default", {}), ("ssd", dict(metric="ssd")), ("ssd_with_lcc_arguments", dict(metric="ssd", window_mm=3.0, var_eps=1.0, a_max=2.0)),
                        ("lcc", dict(metric="lcc"))):
        log = Log(emu_engine)
        runs[name] = (dfm.register_deformable(fixed, moving, engine=log, **kw, **extra), log.calls)
    for name in ("default", "ssd", "ssd_with_lcc_arguments"):
        reg, calls = runs[name]
        assert calls == ssd, name
        assert np.array_equal(reg.field.array.view(np.uint32), runs["default"][0].field.array.view(np.uint32)) and reg.levels == runs["default"][0].levels
        meta = reg.meta()
        assert meta["metric"] == "ssd" and not {"window_voxels", "initial_local_correlation", "final_local_correlation"} & set(meta)
        assert all(len(it) == 2 for lv in reg.levels for it in lv["metric"]) and all("window_voxels" not in lv for lv in reg.levels)
    reg, calls = runs["lcc"]
    assert calls == expected_calls(["warp_dev", "local_moments_dev", "lcc_step_dev"], kw["iterations"])
    meta = reg.meta()
    assert meta["metric"] == "lcc" and meta["window_voxels"] == [[4, 4, 4], [4, 4, 4]]
    assert 0.0 <= meta["initial_local_correlation"] <= 1.0 and 0.0 <= meta["final_local_correlation"] <= 1.0
    assert meta["final_local_correlation"] == reg.final_metric[2] / (2.0 ** 20 * reg.final_metric[1])
    import json

    assert json.loads(json.dumps(meta))["window_voxels"] == meta["window_voxels"]


# ------------------------------------------------------------------------------------------------ the command line
NEED_DEFORMABLE = "--register-metric NAME and --register-window MM need --register-deformable"

CLI_REFUSALS = [
    (["--register-metric", "lcc"], NEED_DEFORMABLE),
    (["--register-window", "10"], NEED_DEFORMABLE),
    (MOVING + ["--registration", "t.json", "--register-metric", "lcc"], NEED_DEFORMABLE),
    (MOVING + ["--registered", "r.npy", "--register-metric", "ssd"], NEED_DEFORMABLE),
    (MOVING + ["--pair", "p.json", "--register-window", "10"], NEED_DEFORMABLE),
    (DEFORM + ["--deformation", "d.npz", "--register-window", "10"], "--register-window MM needs --register-metric lcc"),
    (DEFORM + ["--deformation", "d.npz", "--register-metric", "ssd", "--register-window", "10"], "--register-window MM needs --register-metric lcc"),
    (DEFORM + ["--deformation", "d.npz", "--register-metric", "lcc", "--register-window", "0"], "--register-window: a length in mm > 0, got 0.0"),
    (DEFORM + ["--deformation", "d.npz", "--register-metric", "lcc", "--register-window", "inf"], "--register-window: a length in mm > 0, got inf"),
]


@pytest.fixture
def source(tmp_path, monkeypatch):
    from lungmask_amd import volume_io

    src = tmp_path / "in.npy"
    np.save(src, np.zeros((1, 16, 16), np.int16))
    return str(src), monkeypatch, volume_io


@pytest.mark.parametrize("extra, text", CLI_REFUSALS, ids=lambda v: " ".join(v) if isinstance(v, list) else None)
def test_cli_refusals(source, extra, text):
    src, monkeypatch, volume_io = source
    monkeypatch.setattr(volume_io, "load_input_image", lambda *a, **kw: pytest.fail("refused before anything is loaded"))
    monkeypatch.setattr(cli, "LMInferer", lambda *a, **kw: pytest.fail("refused before anything is loaded"))
    with pytest.raises(SystemExit) as e:
        cli.main([src, "o.npy"] + [a.format(IN=src) for a in extra])
    assert e.value.code == text


def test_cli_refuses_an_unknown_metric(source, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main([source[0], "o.npy"] + [a.format(IN=source[0]) for a in DEFORM] + ["--deformation", "d.npz", "--register-metric", "ncc"])
    assert e.value.code == 2 and "--register-metric" in capsys.readouterr().err


CLI_CALLS = [
    (DEFORM + ["--deformation", "d.npz", "--register-metric", "lcc"], "apply_deformable", dict(transform="rigid", inverse=False, metric="lcc")),
    (DEFORM + ["--deformation", "d.npz", "--register-metric", "lcc", "--register-window", "7.5"], "apply_deformable",
     dict(transform="rigid", inverse=False, metric="lcc", window_mm=7.5)),
    (DEFORM + ["--deformation", "d.npz", "--register-metric", "ssd"], "apply_deformable", dict(transform="rigid", inverse=False, metric="ssd")),
    (DEFORM + ["--deformation", "d.npz"], "apply_deformable", dict(transform="rigid", inverse=False)),
    (DEFORM + ["--pair", "p.json", "--register-metric", "lcc", "--register-window", "6"], "apply_pair",
     dict(PAIR_KW, deformable=True, deformable_kw=dict(metric="lcc", window_mm=6.0))),
    (DEFORM + ["--pair", "p.json"], "apply_pair", dict(PAIR_KW, deformable=True)),
]


@pytest.mark.parametrize("extra, method, kwargs", CLI_CALLS, ids=lambda v: " ".join(v) if isinstance(v, list) else None)
def test_cli_flags_reach_the_apply_call(source, extra, method, kwargs):
    src, monkeypatch, _ = source
    monkeypatch.setattr(cli, "LMInferer", Recorder)
    with pytest.raises(Called) as e:
        cli.main([src, "o.npy", "--noprogress"] + [a.format(IN=src) for a in extra])
    name, images, kw = e.value.args
    assert (name, kw) == (method, kwargs) and len(images) == 2


def test_cli_flags_reach_the_registration_beside_another_product(source):
    """Beside --stats the registration is the stand-alone function's: it gets the two arguments too."""
    src, monkeypatch, _ = source
    from lungmask_amd import morphology, registration

    seen = {}

    class Engine:
        def n_classes(self, slot):
            return 3

    class WithStats(Recorder):
        engine = Engine()

        def apply_with_stats(self, image):
            return np.ones(image.array.shape, np.uint8), {}

    def register_deformable(image, moving, **kw):
        seen.update(kw)
        raise Called("register_deformable")

    monkeypatch.setattr(cli, "LMInferer", WithStats)
    monkeypatch.setattr(morphology, "dilate", lambda labels, mm, engine=None: labels)
    monkeypatch.setattr(registration, "register", lambda *a, **kw: "first")
    monkeypatch.setattr(dfm, "register_deformable", register_deformable)
    with pytest.raises(Called):
        cli.main([src, "o.npy", "--stats", "s.json"] + [a.format(IN=src) for a in DEFORM] + ["--deformation", "d.npz", "--register-metric", "lcc",
                                                                                                "--register-window", "5"])
    assert seen["metric"] == "lcc" and seen["window_mm"] == 5.0 and seen["initial"] == "first"


def test_inferer_keywords():
    from lungmask_amd.mask import LMInferer

    assert {"metric", "window_mm", "var_eps", "a_max"} <= LMInferer._DEFORMABLE_KW
