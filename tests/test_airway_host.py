"""CPU suite of lungmask_amd.airways: the explosion rule on hand-made curves, find_trachea's rule on hand-made volumes, the tree on
masks whose topology is known (through the emulator engine), the argument checks, the command line's refusals and
LMInferer.apply_with_airways through the wrappers' harness (tests/test_mask_wrappers_emu.py)."""
import json

import numpy as np
import pytest

import lungmask_amd.__main__ as cli
from lungmask_amd import airways as aw
from lungmask_amd import volume_io
from tests.test_airway_emu import UNREACHED, cost_oracle
from tests.test_cli_refusals import MADE, VOLUME_EXT, Called, Loaded, Recorder, paths, recorder  # noqa: F401 (fixtures)
from tests.test_mask_wrappers_emu import Harness, alive, nothing_left  # noqa: F401 (fixtures)

CAP = -800
ML = 1e-3  # 1 mm voxels: leak_ml = 10 is 10 000 voxels, max_ml = 400 is 400 000


def curve_of(steps, cap=CAP):
    """A curve from {hu: voxels that join at that hu}."""
    c = np.zeros(cap + 1025, np.int64)
    for hu, n in steps.items():
        c[hu + 1024] = n
    return c


# ---- choose_threshold -------------------------------------------------------------------------------------------------------------------
def test_no_leak_gives_the_cap():
    r = aw.choose_threshold(curve_of({-1000: 900, -940: 200, -870: 300, -805: 50}), ML)
    assert r["threshold"] == CAP and r["first_leaking"] is None and r["voxels"] == 1450 and r["volume_ml"] == pytest.approx(1.45)
    assert r["curve"][0] == [-950, 900] and r["curve"][-1] == [CAP, 1450] and r["cap_hu"] == CAP


def test_single_step_jump_and_give_back_of_the_window():
    # 30 000 voxels join at -863: the first tested threshold that sees them is -860; the whole window -869 .. -860 is given back
    r = aw.choose_threshold(curve_of({-1000: 2000, -868: 7, -863: 30000, -861: 5}), ML)
    assert r["first_leaking"] == -860 and r["threshold"] == -870 and r["voxels"] == 2000
    r = aw.choose_threshold(curve_of({-1000: 2000, -870: 7, -869: 30000}), ML)  # -870 itself is still clean
    assert r["first_leaking"] == -860 and r["threshold"] == -870 and r["voxels"] == 2007


def test_jump_spread_over_less_than_a_step():
    steps = {-1000: 2000}
    steps.update({hu: 3000 for hu in range(-888, -882)})  # 18 000 voxels over six thresholds inside one window
    r = aw.choose_threshold(curve_of(steps), ML)
    assert r["first_leaking"] == -880 and r["threshold"] == -890 and r["voxels"] == 2000
    spread = {-1000: 2000}
    spread.update({hu: 900 for hu in range(-930, -830)})  # 9 000 per window: below leak_ml, never a leak
    assert aw.choose_threshold(curve_of(spread), ML)["threshold"] == CAP


def test_jump_below_leak_ml_or_below_the_ratio_is_ignored():
    r = aw.choose_threshold(curve_of({-1000: 2000, -900: 9999}), ML)  # a factor of six, but under 10 ml
    assert r["threshold"] == CAP and r["first_leaking"] is None
    r = aw.choose_threshold(curve_of({-1000: 100000, -900: 40000}), ML)  # 40 ml, but only a factor 1.4
    assert r["threshold"] == CAP
    assert aw.choose_threshold(curve_of({-1000: 2000, -900: 10001}), ML)["first_leaking"] == -900
    assert aw.choose_threshold(curve_of({-1000: 2000, -900: 9999}), ML, leak_ml=5.0)["first_leaking"] == -900


def test_max_ml():
    slow = {-1000: 300000}
    slow.update({hu: 8000 for hu in range(-940, -800, 10)})  # never a jump; V[-820] = 300 000 + 13 x 8 000 is the first over 400 ml
    r = aw.choose_threshold(curve_of(slow), ML)
    assert r["first_leaking"] == -820 and r["threshold"] == -830 and r["voxels"] == 300000 + 12 * 8000
    assert aw.choose_threshold(curve_of(slow), ML, max_ml=1000.0)["threshold"] == CAP


def test_empty_curve_and_leak_at_once_give_none():
    r = aw.choose_threshold(curve_of({}), ML)
    assert r["threshold"] is None and r["voxels"] == 0 and r["first_leaking"] is None
    r = aw.choose_threshold(curve_of({-945: 50000}), ML)  # open to outside air: the first step leaks, nothing below it
    assert r["threshold"] is None and r["first_leaking"] == -940 and r["voxels"] == 0
    r = aw.choose_threshold(curve_of({-1000: 500, -945: 50000}), ML)  # ... with a trachea below start_hu: it is kept
    assert r["threshold"] == -950 and r["voxels"] == 500


def test_thresholds_below_start_are_never_tested_and_steps_stop_at_the_cap():
    r = aw.choose_threshold(curve_of({-1020: 10, -990: 50000}), ML)
    assert r["threshold"] == CAP and r["first_leaking"] is None
    r = aw.choose_threshold(curve_of({-1000: 2000, -803: 50000}, cap=-803), ML)  # -800 is beyond the cap: the last tested t is -810
    assert r["threshold"] == -803 and r["first_leaking"] is None and r["voxels"] == 52000


def test_choose_threshold_arguments():
    c = curve_of({-1000: 5})
    for kw, text in ((dict(voxel_ml=0), "voxel_ml"), (dict(start_hu=-700), "start_hu"), (dict(step_hu=0), "step_hu"),
                     (dict(leak_ratio=0.5), "leak_ratio"), (dict(leak_ml=-1), "leak_ml"), (dict(max_ml=float("nan")), "max_ml")):
        with pytest.raises(ValueError, match=text):
            aw.choose_threshold(c, **dict(dict(voxel_ml=ML), **kw))
    with pytest.raises(ValueError, match="curve"):
        aw.choose_threshold(np.zeros((3, 3), np.int64), ML)
    with pytest.raises(ValueError, match="curve"):
        aw.choose_threshold(c.astype(np.float64), ML)


# ---- find_trachea -----------------------------------------------------------------------------------------------------------------------
def body(shape=(30, 24, 28)):
    """Tissue with outside air on the y and x borders."""
    vol = np.full(shape, 40, np.int16)
    vol[:, :2, :] = vol[:, -2:, :] = -1000
    vol[:, :, :2] = vol[:, :, -2:] = -1000
    return vol


def test_outside_air_and_blobs_are_excluded(emu_engine):
    vol = body()
    vol[0:24, 10:13, 12:15] = -990      # the trachea: 24 slices, 9 voxels across
    vol[20:28, 5:15, 18:25] = -980      # a bubble: 8 slices only
    vol[2:26, 14:21, 4:10] = -1000      # 24 slices but 42 voxels across: over 40 mm^2 below
    r = aw.find_trachea(vol, engine=emu_engine, max_area_mm2=40.0)
    assert r["index"] == (0, 10, 12) and len(r["candidates"]) == 1 and r["components"] == 4
    assert r["rejected"] == {"touches_border": 1, "too_short": 1, "too_wide": 1, "outside_lung_box": 0}
    c = r["candidates"][0]
    assert c["voxels"] == 24 * 9 and c["length_mm"] == 24.0 and c["mean_area_mm2"] == 9.0 and c["bbox"] == [0, 24, 10, 13, 12, 15]
    wide = aw.find_trachea(vol, engine=emu_engine)  # the default 600 mm^2 lets the wide one in: same length, more voxels, so it wins
    assert wide["index"] == (2, 14, 4) and [k["voxels"] for k in wide["candidates"]] == [24 * 42, 24 * 9]
    spaced = aw.find_trachea(vol, spacing=(0.5, 1.0, 1.0), engine=emu_engine, max_area_mm2=40.0, min_length_mm=12.0)
    assert spaced["index"] == (0, 10, 12) and spaced["candidates"][0]["length_mm"] == 12.0
    with pytest.raises(aw.NoTrachea, match="1 touch the y or x border, 3 shorter than 20.0 mm"):
        aw.find_trachea(vol, spacing=(0.5, 1.0, 1.0), engine=emu_engine)


def test_tie_order_and_labels(emu_engine):
    vol = body()
    vol[3:27, 6:8, 6:8] = -990       # A: 24 slices, 96 voxels
    vol[0:24, 6:8, 20:22] = -990     # B: 24 slices, 96 voxels, the smaller id (first voxel in slice 0)
    vol[5:29, 16:18, 12:15] = -990   # C: 24 slices, 144 voxels
    r = aw.find_trachea(vol, engine=emu_engine)
    assert [c["voxels"] for c in r["candidates"]] == [144, 96, 96] and r["index"] == (5, 16, 12)
    assert r["candidates"][1]["index"] == [0, 6, 20] and r["candidates"][1]["component"] < r["candidates"][2]["component"]
    lab = np.zeros(vol.shape, np.uint8)
    lab[4:20, 4:12, 4:24] = 1        # the lungs' in-plane box: y 4 .. 11, x 4 .. 23; C's centroid (16.5, 13) lies outside
    lab[vol < 0] = 0
    r = aw.find_trachea(vol, lab, engine=emu_engine)
    assert r["index"] == (0, 6, 20) and r["rejected"]["outside_lung_box"] == 1 and len(r["candidates"]) == 2
    lab[5:29, 16:18, 12:15] = 2      # air inside a label is no candidate at all
    assert aw.find_trachea(vol, lab, engine=emu_engine)["components"] == r["components"] - 1
    assert aw.find_trachea(vol, np.zeros(vol.shape, np.uint8), engine=emu_engine)["index"] == (5, 16, 12)  # labels without a voxel


def test_no_candidate_says_what_was_found(emu_engine):
    with pytest.raises(aw.NoTrachea, match="no candidate among 1 air components .*1 touch the y or x border"):
        aw.find_trachea(body(), engine=emu_engine)
    with pytest.raises(ValueError, match="no candidate among 0 air components"):
        aw.find_trachea(np.full((4, 5, 6), 40, np.int16), engine=emu_engine)
    with pytest.raises(ValueError, match="seed_hu"):
        aw.find_trachea(body(), seed_hu=-950.5, engine=emu_engine)
    with pytest.raises(ValueError, match="min_length_mm"):
        aw.find_trachea(body(), min_length_mm=0, engine=emu_engine)


# ---- airway_tree ------------------------------------------------------------------------------------------------------------------------
def tube(mask, a, b, r):
    """A straight tube of radius r between the voxels a and b (axis-aligned or diagonal), drawn as balls along the line."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    z, y, x = np.meshgrid(*(np.arange(s) for s in mask.shape), indexing="ij")
    for t in np.linspace(0, 1, int(np.abs(b - a).max()) * 2 + 1):
        c = a + t * (b - a)
        mask |= (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= r * r
    return mask


def y_mask(spur=False):
    m = np.zeros((40, 21, 41), bool)
    tube(m, (0, 10, 20), (18, 10, 20), 2.0)
    tube(m, (18, 10, 20), (34, 10, 6), 1.5)
    tube(m, (18, 10, 20), (34, 10, 34), 1.5)
    if spur:
        m[8, 12, 22] = m[8, 13, 23] = True  # a diagonal bump of two voxels on the trunk's surface: a spur of 1.41 mm with radius 1
    return m


def summary(tree):
    return [g["segments"] for g in tree["generations"]], tree["totals"]


def test_y(emu_engine):
    tree = aw.airway_tree(y_mask(), (0, 10, 20), engine=emu_engine)
    per_gen, totals = summary(tree)
    assert per_gen == [1, 2] and totals["segments"] == 3 and totals["end_points"] == 2 and totals["deepest_generation"] == 1
    assert totals["cycles"] == 0 and totals["unreached_segments"] == 0
    root = tree["segments"][0]
    assert root["id"] == tree["root"] and root["generation"] == 0 and root["parent"] is None and len(root["children"]) == 2
    assert all(s["parent"] == root["id"] and s["children"] == [] for s in tree["segments"][1:])
    assert 12 <= root["length_mm"] <= 19 and 3.0 <= root["diameter_mm"] <= 5.0 and root["label"] == 0
    assert all(14 <= s["length_mm"] <= 23 and s["diameter_mm"] < root["diameter_mm"] for s in tree["segments"][1:])
    assert json.loads(json.dumps(tree)) == tree
    spaced = aw.airway_tree(y_mask(), (0, 10, 20), spacing=(2.0, 1.0, 1.0), engine=emu_engine)
    assert spaced["segments"][0]["length_mm"] > 1.5 * root["length_mm"] and summary(spaced)[0] == [1, 2]


def test_y_with_a_spur(emu_engine):
    kept = aw.airway_tree(y_mask(spur=True), (0, 10, 20), spur_factor=0.0, engine=emu_engine)
    pruned = aw.airway_tree(y_mask(spur=True), (0, 10, 20), engine=emu_engine)
    clean = aw.airway_tree(y_mask(), (0, 10, 20), engine=emu_engine)
    assert kept["totals"]["pruned_spurs"] == 0 and kept["totals"]["segments"] > 3  # the bump leaves an end point, and the thinning keeps it
    assert pruned["totals"]["pruned_spurs"] >= 1 and summary(pruned)[0] == [1, 2] and pruned["totals"]["segments"] == 3
    assert pruned["totals"]["end_points"] == clean["totals"]["end_points"] == 2


def test_three_level_binary_tree_with_labels(emu_engine):
    m = np.zeros((44, 25, 65), bool)
    tube(m, (0, 12, 32), (12, 12, 32), 2.0)
    forks = [((12, 12, 32), (24, 12, 16)), ((12, 12, 32), (24, 12, 48))]
    leaves = [((24, 12, 16), (38, 12, 6)), ((24, 12, 16), (38, 12, 24)), ((24, 12, 48), (38, 12, 40)), ((24, 12, 48), (38, 12, 58))]
    for a, b in forks:
        tube(m, a, b, 1.5)
    for a, b in leaves:
        tube(m, a, b, 1.0)
    lab = np.zeros(m.shape, np.uint8)
    lab[10:, :, :32] = 1
    lab[10:, :, 32:] = 2
    tree = aw.airway_tree(m, [(0, 12, 32)], labels=lab, engine=emu_engine)
    per_gen, totals = summary(tree)
    assert per_gen == [1, 2, 4] and totals["end_points"] == 4 and totals["deepest_generation"] == 2 and totals["cycles"] == 0
    by_id = {s["id"]: s for s in tree["segments"]}
    root = by_id[tree["root"]]
    assert root["label"] == 0 and sorted(by_id[k]["generation"] for k in root["children"]) == [1, 1]
    for k in root["children"]:
        assert by_id[k]["parent"] == root["id"] and len(by_id[k]["children"]) == 2
        for leaf in by_id[k]["children"]:
            assert by_id[leaf]["generation"] == 2 and by_id[leaf]["parent"] == k and by_id[leaf]["label"] == by_id[k]["label"]
    assert sorted(by_id[k]["label"] for k in root["children"]) == [1, 2]
    gens = tree["generations"]
    assert gens[0]["mean_diameter_mm"] > gens[1]["mean_diameter_mm"] > gens[2]["mean_diameter_mm"]
    assert gens[2]["length_mm"] == pytest.approx(sum(s["length_mm"] for s in tree["segments"] if s["generation"] == 2))


def test_ring_is_reported_not_broken_and_empty_mask(emu_engine):
    m = np.zeros((30, 9, 31), bool)
    tube(m, (0, 4, 15), (8, 4, 15), 1.0)
    tube(m, (8, 4, 15), (16, 4, 6), 1.0)
    tube(m, (8, 4, 15), (16, 4, 24), 1.0)
    tube(m, (16, 4, 6), (24, 4, 15), 1.0)
    tube(m, (16, 4, 24), (24, 4, 15), 1.0)
    tree = aw.airway_tree(m, (0, 4, 15), engine=emu_engine)
    assert tree["totals"]["cycles"] >= 1 and tree["segments"][0]["generation"] == 0
    empty = aw.airway_tree(np.zeros((4, 5, 6), bool), (0, 0, 0), engine=emu_engine)
    assert empty["segments"] == [] and empty["root"] is None and empty["totals"]["segments"] == 0
    with pytest.raises(ValueError, match="spur_factor"):
        aw.airway_tree(m, (0, 4, 15), spur_factor=-1, engine=emu_engine)
    with pytest.raises(ValueError, match="seed"):
        aw.airway_tree(m, (0, 4), engine=emu_engine)
    with pytest.raises(ValueError, match="same shape"):
        aw.airway_tree(m, (0, 4, 15), labels=np.zeros((2, 2, 2), np.uint8), engine=emu_engine)


# ---- segment_airways: arguments, results, JSON ----------------------------------------------------------------------------------------------
def small_chest():
    """(30, 24, 28): outside air, tissue, a trachea of 3 x 3 that forks into two bronchi ending in two air sacs."""
    vol = body()
    vol[0:22, 10:13, 12:15] = -990
    vol[20:23, 10:13, 5:22] = -960
    vol[22:28, 9:14, 4:8] = -900
    vol[22:28, 9:14, 19:23] = -880
    lab = np.zeros(vol.shape, np.uint8)
    lab[22:28, 9:14, 4:8] = 1
    lab[22:28, 9:14, 19:23] = 2
    return vol, lab


def test_segment_airways_on_a_small_chest(emu_engine):
    vol, lab = small_chest()
    res = aw.segment_airways(vol, lab, spacing=(1.0, 1.0, 1.0), names={1: "left", 2: "right"}, engine=emu_engine)
    cost = cost_oracle(vol, [(0, 10, 12)], -800)[0]
    assert res.seed == [[0, 10, 12]] and res.threshold == -800 and res.analysis["first_leaking"] is None
    assert np.array_equal(res.cost, cost) and np.array_equal(res.mask, (cost <= -800).astype(np.uint8)) and res.mask.dtype == np.uint8
    a = res.analysis
    assert a["by_label"]["1"] == {"name": "left", "voxels": 120, "volume_ml": pytest.approx(0.12)}
    assert a["by_label"]["2"]["voxels"] == 120 and a["by_label"]["0"]["name"] == "outside the labels"
    assert a["voxels"] == int(res.mask.sum()) == a["reached"] and a["trachea"]["index"] == [0, 10, 12] and a["error"] is None
    assert a["parameters"]["cap_hu"] == -800 and a["parameters"]["start_hu"] == -950 and a["rounds"] >= 1
    assert json.loads(json.dumps(res.meta())) == res.meta() and set(res.meta()) == {"analysis", "tree"}
    fixed = aw.segment_airways(vol, lab, seed=(5, 11, 13), threshold=-950, engine=emu_engine)  # the rule and the search are skipped
    assert fixed.threshold == -950 and fixed.analysis["trachea"] is None and fixed.analysis["volume_ml"] is None
    assert np.array_equal(fixed.mask, (cost_oracle(vol, [(5, 11, 13)], -800)[0] <= -950).astype(np.uint8)) and fixed.mask.sum() == 22 * 9 + 3 * 3 * 17 - 18 - 18  # (less what the two share and what the sacs overwrote)
    tissue = aw.segment_airways(vol, lab, seed=(5, 5, 5), engine=emu_engine)  # a seed in tissue: nothing, and the reason
    assert tissue.threshold is None and not tissue.mask.any() and "not air" in tissue.analysis["error"] and (tissue.cost == UNREACHED).all()
    leak = vol.copy()
    leak[10, 0:10, 13] = -945  # a channel to the outside air, as a scan with the mouth in it has
    open_ = aw.segment_airways(leak, lab, seed=(0, 10, 12), spacing=(4.0, 4.0, 4.0), leak_ml=1.0, engine=emu_engine)
    assert open_.threshold == -950 and open_.analysis["first_leaking"] == -940  # the trachea below start_hu is all that is kept
    with pytest.raises(aw.NoTrachea, match="no candidate"):
        aw.segment_airways(body(), engine=emu_engine)
    assert "no candidate" in aw.segment_or_empty(body(), engine=emu_engine).analysis["error"]


def test_segment_airways_arguments(emu_engine):
    vol, lab = small_chest()
    for kw, text in ((dict(cap_hu=-1024), "cap_hu"), (dict(cap_hu=-800.5), "cap_hu"), (dict(threshold=-700), "threshold"),
                     (dict(threshold=-900.5), "threshold"), (dict(seed=(1, 2)), "seed"), (dict(seed=(1.0, 2.0, 3.0)), "seed"),
                     (dict(step_hu=0), "step_hu"), (dict(start_hu=-700), "start_hu"), (dict(leak_ratio=0.9), "leak_ratio"),
                     (dict(spur_factor=-1), "spur_factor"), (dict(seed_hu=4000), "seed_hu"), (dict(spacing=(1, 0, 1)), "spacing")):
        with pytest.raises(ValueError, match=text):
            aw.segment_airways(vol, lab, engine=emu_engine, **kw)
    with pytest.raises(TypeError, match="unknown keyword"):
        aw.segment_airways(vol, lab, engine=emu_engine, leak=3)
    with pytest.raises(ValueError, match="outside the volume"):
        aw.segment_airways(vol, lab, seed=(30, 0, 0), engine=emu_engine)
    with pytest.raises(ValueError, match="same shape"):
        aw.segment_airways(vol, lab[1:], engine=emu_engine)
    cost, curve, info = aw.minimax_cost(vol, (0, 10, 12), engine=emu_engine)
    assert np.array_equal(cost, cost_oracle(vol, [(0, 10, 12)], -800)[0]) and curve.sum() == info["reached"]


# ---- the command line -------------------------------------------------------------------------------------------------------------------
NEED_AIRWAYS = "--airway-seed Z Y X, --airway-cap HU and --airway-threshold HU need --airways PATH, --airway-tree PATH.json or --airway-cost PATH"
AIRWAY_REFUSALS = [
    (["--airway-seed", "1", "2", "3"], NEED_AIRWAYS),
    (["--airway-cap", "-700"], NEED_AIRWAYS),
    (["--airway-threshold", "-900"], NEED_AIRWAYS),
    (["--airways", "a.txt"], "--airways: unsupported file type 'a.txt' " + VOLUME_EXT),
    (["--airway-cost", "c.json"], "--airway-cost: unsupported file type 'c.json' " + VOLUME_EXT),
    (["--airway-tree", "t.npy"], "--airway-tree: unsupported file type 't.npy' (use .json)"),
    (["--airways", "a.npy", "--airway-cap", "-1024"],
     "--airway-seed / --airway-cap / --airway-threshold: cap_hu: an integer in -1023 .. 3071, got -1024"),
    (["--airways", "a.npy", "--airway-threshold", "-700"],
     "--airway-seed / --airway-cap / --airway-threshold: threshold: None or an integer in -1024 .. cap_hu (-800), got -700"),
]


@pytest.mark.parametrize("extra, text", AIRWAY_REFUSALS, ids=lambda v: " ".join(v) if isinstance(v, list) else None)
def test_cli_refusals(paths, extra, text):  # noqa: F811
    with pytest.raises(SystemExit) as e:
        cli.main([paths["IN"], "o.npy"] + extra)
    assert e.value.code == text


def test_cli_accepts_and_selects_apply_with_airways(recorder):  # noqa: F811
    with pytest.raises(Called) as e:
        cli.main([recorder, "o.npy", "--airways", "a.nii.gz", "--airway-seed", "0", "7", "8", "--airway-cap", "-750", "--airway-threshold", "-900"])
    name, images, kw = e.value.args
    assert name == "apply_with_airways" and kw == dict(seed=(0, 7, 8), cap_hu=-750, threshold=-900) and len(images) == 1
    with pytest.raises(Called) as e:
        cli.main([recorder, "o.npy", "--airway-tree", "t.json"])
    assert e.value.args[0] == "apply_with_airways" and e.value.args[2] == dict(seed=None, cap_hu=-800, threshold=None)
    with pytest.raises(Called) as e:  # the earlier rungs keep the volume; the airways are then computed beside them
        cli.main([recorder, "o.npy", "--airway-cost", "c.npy", "--stats", "s.json"])
    assert e.value.args[0] == "apply_with_stats"
    with pytest.raises(Called) as e:
        cli.main([recorder, "o.npy", "--airways", "a.npy", "--resampled", "r.npy"])
    assert e.value.args[0] == "apply_with_airways"
    with pytest.raises(Called) as e:  # without the flags every call is what it was
        cli.main([recorder, "o.npy"])
    assert e.value.args[0] == "apply" and e.value.args[2] == {}


# ---- LMInferer.apply_with_airways ---------------------------------------------------------------------------------------------------------
def same_result(a, b):
    assert np.array_equal(a.mask, b.mask) and np.array_equal(a.cost, b.cost) and np.array_equal(a.curve, b.curve)
    assert a.threshold == b.threshold and a.seed == b.seed and a.analysis == b.analysis and a.tree == b.tree


def test_apply_with_airways_device_branch(emu_engine, alive):  # noqa: F811
    vol, lab = small_chest()
    h = Harness(emu_engine, lab)
    names = h.inf._model_labels()[1]
    try:
        sp = (1.0, 1.0, 1.0)
        with nothing_left(alive):
            labels, res = h.inf.apply_with_airways(vol, spacing=sp)
        assert np.array_equal(labels, lab) and len(h.calls) == 1 and h.applied == 0
        same_result(res, aw.segment_airways(vol, lab, spacing=sp, names=names, engine=emu_engine))
        assert res.mask.any() and res.analysis["by_label"]["1"]["name"] == names[1]
        with nothing_left(alive):
            labels, res = h.inf.apply_with_airways(volume_io.Volume(vol, sp, (1.0, 2.0, 3.0)), seed=(5, 11, 13), threshold=-950, cap_hu=-900)
        same_result(res, aw.segment_airways(vol, lab, seed=(5, 11, 13), threshold=-950, cap_hu=-900, spacing=sp, names=names, engine=emu_engine))
        with nothing_left(alive):  # no trachea: the labels and an empty result with the reason, no exception
            labels, res = h.inf.apply_with_airways(body())
        assert np.array_equal(labels, lab) and not res.mask.any() and res.threshold is None and "no candidate" in res.analysis["error"]
        assert json.loads(json.dumps(res.meta())) == res.meta()
        with nothing_left(alive), pytest.raises(ValueError, match="cap_hu"):
            h.inf.apply_with_airways(vol, cap_hu=5000)
        with nothing_left(alive), pytest.raises(ValueError, match="outside the volume"):
            h.inf.apply_with_airways(vol, seed=(99, 0, 0))
    finally:
        h.inf.close()


def test_apply_with_airways_host_detour(emu_engine):
    vol, lab = small_chest()
    h = Harness(emu_engine, lab)
    try:
        h.inf._shard = object()  # several engines: the labels come gathered from apply()
        labels, res = h.inf.apply_with_airways(vol, spacing=(1.0, 1.0, 1.0))
        assert h.applied == 1 and h.calls == [] and np.array_equal(labels, lab)
        same_result(res, aw.segment_airways(vol, lab, spacing=(1.0, 1.0, 1.0), names=h.inf._model_labels()[1], engine=emu_engine))
        labels, res = h.inf.apply_with_airways(body())
        assert "no candidate" in res.analysis["error"] and not res.mask.any()
    finally:
        h.inf._shard = None
        h.inf.close()
