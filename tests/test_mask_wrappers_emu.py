"""CPU suite: the one-GPU device branch of LMInferer's apply_* methods, on the emulator, without the network.

The scaffolding under those methods (input forms, orientation, host detours, result array, uploads, frees, download) needs device
labels in the caller's orientation and nothing else of the network, whose emulated forward takes 10-30 s.  So `_labels_dev` is
replaced on the instance by a stub that uploads a fixed label volume, records (axes, flips, free_input) and honours `free_input`, and
`apply` by a stub that returns a copy of the same labels.  Everything is compared exactly: the first result with the labels, the
second with the stand-alone function the method's docstring names, bit for bit for arrays and `==` for dicts.  Device allocations
are counted (every DeviceArray of the test's engine, uploads included): after each call, and after each call that raises, none
is left behind, and none was left to the garbage collector."""
import contextlib
import re
import weakref

import numpy as np
import pytest

from lungmask_amd import _native as nat
from lungmask_amd import components, filters, mesh, morphology, roi, stats, texture, volume_io
from lungmask_amd.mask import LMInferer
from oracle import unet_oracle as uo

SHAPE = (5, 12, 9)
SPACING = (1.5, 0.8, 0.7)  # array axis order; the Volumes carry it as (x, y, z)
ORIGIN = (-12.0, 30.0, 4.5)
DIRECTION = [[0, 1, 0], [1, 0, 0], [0, 0, -1]]  # permuted and flipped
IDENTITY = ((0, 1, 2), (False, False, False))
NAMES = stats.label_names("R231", 3)

IMAGE = np.random.default_rng(7).integers(-1100, 200, SHAPE).astype(np.int16)
LABELS = np.zeros(SHAPE, np.uint8)
LABELS[1:4, 2:6, 1:4] = 1
LABELS[1:4, 6:10, 5:8] = 2
NO_LABELS = np.zeros(SHAPE, np.uint8)


class Boom(Exception):
    pass


class Harness:
    """An LMInferer on the emulator whose labelling is the fixed volume `labels`."""

    def __init__(self, engine, labels):
        self.engine, self.labels = engine, labels
        self.calls, self.applied = [], 0
        self.inf = LMInferer(state_dict=uo.synthetic_state_dict(3), engine=engine)
        self.inf._labels_dev = self._labels_dev
        self.inf.apply = self._apply

    def _labels_dev(self, raw, axes, flips, free_input=False):
        self.calls.append((tuple(axes), tuple(bool(f) for f in flips), bool(free_input)))
        assert tuple(raw.shape) == self.labels.shape
        back = self.engine.to_device(self.labels)
        if free_input:
            raw.free()
        return back

    def _apply(self, image, out=None):
        self.applied += 1
        return self.labels.copy()

    def reset(self):
        self.calls, self.applied = [], 0


@pytest.fixture(scope="module")
def lung(emu_engine):
    h = Harness(emu_engine, LABELS)
    yield h
    h.inf.close()


@pytest.fixture(scope="module")
def empty(emu_engine):
    h = Harness(emu_engine, NO_LABELS)
    yield h
    h.inf.close()


class Allocations:
    """The live DeviceArrays of the test's engine: `ptrs`, the device pointers allocated and not yet freed by a call of `free()`, and
    `dropped`, the shapes of arrays that were garbage-collected without one (`DeviceArray.__del__` frees them, which would hide a
    missing `free()` from `ptrs`).  DeviceViews own nothing and are not counted."""

    def __init__(self):
        self.ptrs, self.dropped = set(), []


@pytest.fixture
def alive(emu_engine, monkeypatch):
    acc = Allocations()
    init, free = nat.DeviceArray.__init__, nat.DeviceArray.free

    def counted_init(self, eng, shape, dtype):
        init(self, eng, shape, dtype)
        if eng is emu_engine and self.ptr:
            acc.ptrs.add(self.ptr)

    def counted_free(self):
        if self.eng is emu_engine:
            acc.ptrs.discard(self.ptr)
        free(self)

    def counted_del(self):
        if self.ptr and self.eng is emu_engine and self.eng.h:
            acc.dropped.append(self.shape)
            counted_free(self)

    monkeypatch.setattr(nat.DeviceArray, "__init__", counted_init)
    monkeypatch.setattr(nat.DeviceArray, "free", counted_free)
    monkeypatch.setattr(nat.DeviceArray, "__del__", counted_del)
    return acc


@contextlib.contextmanager
def nothing_left(alive):
    before, dropped = set(alive.ptrs), len(alive.dropped)
    yield
    assert alive.ptrs == before, f"{len(alive.ptrs - before)} device array(s) left behind"
    assert alive.dropped[dropped:] == [], "device arrays left to the garbage collector"


def forms(arr):
    """name -> (image, spacing argument): the bare array, an LPS Volume, a permuted and flipped Volume."""
    return {"array": (arr, SPACING),
            "lps": (volume_io.Volume(arr, SPACING[::-1], ORIGIN), None),
            "permuted": (volume_io.Volume(arr, SPACING[::-1], ORIGIN, DIRECTION), None)}


def like(image, labels):
    return labels if isinstance(image, np.ndarray) else image.like(labels)


def present(labels):
    return [k for k in (1, 2) if (labels == k).any()]


class Case:
    def __init__(self, method, call, ref, boom, free_input=False, takes_spacing=True):
        self.method, self.call, self.ref, self.boom, self.free_input, self.takes_spacing = method, call, ref, boom, free_input, takes_spacing


CASES = {
    "stats": Case("apply_with_stats", lambda inf, img, sp: inf.apply_with_stats(img, spacing=sp),
                  lambda eng, img, sp, lab: stats.label_statistics(img, lab, spacing=sp, n_labels=3, names=NAMES, engine=eng),
                  "label_stats_dev"),
    "texture": Case("apply_with_texture", lambda inf, img, sp: inf.apply_with_texture(img),
                    lambda eng, img, sp, lab: texture.texture_features(img, lab, n_labels=3, names=NAMES, engine=eng),
                    "texture_dev", takes_spacing=False),
    "roi": Case("apply_roi", lambda inf, img, sp: inf.apply_roi(img, margin_mm=1.0, spacing=sp),
                lambda eng, img, sp, lab: roi.extract_roi(img, lab, spacing=sp, margin_mm=1.0, engine=eng),
                "roi_dev"),
    "mesh": Case("apply_mesh", lambda inf, img, sp: inf.apply_mesh(img, spacing=sp),
                 lambda eng, img, sp, lab: {k: mesh.extract_surface(like(img, lab), spacing=sp, label=k, engine=eng) for k in present(lab)},
                 "mesh_dev", free_input=True),
    "closed": Case("apply_closed", lambda inf, img, sp: inf.apply_closed(img, radius_mm=2.0, spacing=sp),
                   lambda eng, img, sp, lab: morphology.close(like(img, lab), 2.0, spacing=sp, engine=eng),
                   "morph_dev", free_input=True),
    "clusters": Case("apply_with_clusters", lambda inf, img, sp: inf.apply_with_clusters(img, threshold=-900, spacing=sp),
                     lambda eng, img, sp, lab: components.cluster_analysis(img, lab, -900, None, 6, spacing=sp, names=NAMES, engine=eng),
                     "components_dev"),
    "median": Case("apply_denoised", lambda inf, img, sp: inf.apply_denoised(img, method="median", size=3, spacing=sp),
                   lambda eng, img, sp, lab: filters.median(img, 3, labels=lab, engine=eng),
                   "filter_dev"),
    "gaussian": Case("apply_denoised", lambda inf, img, sp: inf.apply_denoised(img, method="gaussian", sigma_mm=1.2, spacing=sp),
                     lambda eng, img, sp, lab: filters.gaussian(img, 1.2, spacing=sp, labels=lab, engine=eng),
                     "filter_dev"),
}
FORMS = ("array", "lps", "permuted")


def same_array(a, b):
    return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def assert_same(got, want):
    """Exact equality of the second result of an apply_* method and its stand-alone function."""
    if isinstance(want, np.ndarray):
        assert same_array(got, want)
    elif isinstance(want, roi.Roi):
        assert same_array(got.image, want.image) and same_array(got.labels, want.labels)
        assert got.meta() == want.meta()
        assert (got._geometry is None) == (want._geometry is None)
        if want._geometry is not None:
            a, b = got.as_volume(), want.as_volume()
            assert (a.spacing, a.origin) == (b.spacing, b.origin) and np.array_equal(a.direction, b.direction)
    elif isinstance(want, dict) and any(isinstance(v, mesh.Mesh) for v in want.values()):
        assert list(got) == list(want)
        for k in want:
            assert same_array(got[k].vertices, want[k].vertices) and same_array(got[k].quads, want[k].quads)
            assert got[k].meta() == want[k].meta()
    else:
        assert type(got) is type(want) and got == want


def is_root(a):
    return isinstance(a, np.ndarray) and not isinstance(a.base, np.ndarray) and a.flags.c_contiguous and a.dtype == np.uint8


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", list(CASES))
def test_device_branch_equals_the_stand_alone_function(lung, alive, case, form):
    c = CASES[case]
    image, sp = forms(IMAGE)[form]
    lung.reset()
    with nothing_left(alive):
        labels, second = c.call(lung.inf, image, sp)
        held = labels
        labels2, second2 = c.call(lung.inf, image, sp)
    assert np.array_equal(labels, LABELS) and np.array_equal(labels2, LABELS)
    assert is_root(labels) and is_root(labels2) and not np.shares_memory(held, labels2)
    want = c.ref(lung.engine, image, sp, LABELS)
    assert_same(second, want)
    assert_same(second2, want)
    transform = IDENTITY if form != "permuted" else volume_io.lps_transform(DIRECTION)
    assert lung.calls == [transform + (c.free_input,)] * 2 and lung.applied == 0
    assert volume_io.lps_transform(DIRECTION) != IDENTITY


@pytest.mark.parametrize("case", list(CASES))
def test_a_dropped_result_is_gone_at_once(lung, case):
    """The result array is the caller's alone: nothing of the call keeps it alive (no reference cycle either), so its page-locked
    block returns to the pool when the caller drops it, without waiting for a garbage collection."""
    image, sp = forms(IMAGE)["permuted"]
    labels = CASES[case].call(lung.inf, image, sp)[0]
    assert labels.base is not None  # (a block of the pool, not an ordinary array)
    gone = weakref.ref(labels)
    del labels
    assert gone() is None


def test_mesh_of_all_labels_together(lung, alive):
    image, _ = forms(IMAGE)["permuted"]
    with nothing_left(alive):
        labels, meshes = lung.inf.apply_mesh(image, per_label=False, smooth=2)
    assert np.array_equal(labels, LABELS) and list(meshes) == ["lung"]
    assert_same(meshes, {"lung": mesh.extract_surface(image.like(LABELS), smooth=2, engine=lung.engine)})


class _DummyShard:
    def close(self):
        pass


@pytest.mark.parametrize("case", list(CASES))
def test_several_engines_take_the_host_path(lung, alive, case):
    c = CASES[case]
    image, sp = forms(IMAGE)["permuted"]
    lung.reset()
    lung.inf._shard = _DummyShard()
    try:
        with nothing_left(alive):
            labels, second = c.call(lung.inf, image, sp)
    finally:
        lung.inf._shard = None
    assert np.array_equal(labels, LABELS)
    assert_same(second, c.ref(lung.engine, image, sp, LABELS))
    assert lung.calls == [] and lung.applied == 1


@pytest.mark.parametrize("dtype,offset,threshold", [(np.uint8, 1100, 100), (np.uint16, 1100, 150)])
def test_clusters_of_unsigned_volumes_are_computed_on_the_device(lung, alive, dtype, offset, threshold):
    """uint8 and uint16 are widened to int32 before the device branch is chosen: they take it like every other integer volume."""
    arr = ((IMAGE.astype(np.int32) + offset) % (np.iinfo(dtype).max + 1)).astype(dtype)
    lung.reset()
    with nothing_left(alive):
        labels, clusters = lung.inf.apply_with_clusters(arr, threshold=threshold, spacing=SPACING)
    assert np.array_equal(labels, LABELS)
    assert clusters == components.cluster_analysis(arr, LABELS, threshold, None, 6, spacing=SPACING, names=NAMES, engine=lung.engine)
    assert clusters["lung"]["clusters"] > 0
    assert lung.calls == [IDENTITY + (False,)] and lung.applied == 0


def test_median_of_dtypes_the_kernel_does_not_take_goes_through_the_host_path(lung, alive):
    lung.reset()
    with nothing_left(alive):
        labels, filtered = lung.inf.apply_denoised(IMAGE.astype(np.int64), method="median")
    assert np.array_equal(labels, LABELS)
    assert_same(filtered, filters.median(IMAGE.astype(np.int64), 3, labels=LABELS, engine=lung.engine))
    assert filtered.dtype == np.int64 and lung.calls == [] and lung.applied == 1
    lung.reset()
    with nothing_left(alive):
        with pytest.raises(ValueError) as exc:
            lung.inf.apply_denoised(IMAGE.astype(np.float64), method="median")
    assert str(exc.value) == "median: float64 is not supported; cast the image to float32 first (image.astype(np.float32))"
    assert lung.calls == [] and lung.applied == 1
    lung.reset()
    with nothing_left(alive):  # (the Gaussian takes float64 on the device)
        labels, filtered = lung.inf.apply_denoised(IMAGE.astype(np.float64), method="gaussian", sigma_mm=1.2)
    assert_same(filtered, filters.gaussian(IMAGE.astype(np.float64), 1.2, labels=LABELS, engine=lung.engine))
    assert lung.calls == [IDENTITY + (False,)] and lung.applied == 0


@pytest.mark.parametrize("form", FORMS)
def test_no_labelled_voxel(empty, alive, form):
    image, sp = forms(IMAGE)[form]
    inf, eng = empty.inf, empty.engine
    empty.reset()
    with nothing_left(alive):
        labels, closed = inf.apply_closed(image, radius_mm=2.0, spacing=sp)
    assert is_root(labels) and not labels.any() and same_array(closed, labels) and not np.shares_memory(closed, labels)
    for c, want in ((CASES["median"], IMAGE), (CASES["gaussian"], IMAGE.astype(np.float32))):
        with nothing_left(alive):
            labels, filtered = c.call(inf, image, sp)
        assert not labels.any() and same_array(filtered, want) and not np.shares_memory(filtered, IMAGE)
    for name in ("stats", "texture", "clusters", "mesh"):
        c = CASES[name]
        with nothing_left(alive):
            labels, second = c.call(inf, image, sp)
        assert is_root(labels) and not labels.any()
        if name == "mesh":
            assert second == {}
        else:
            assert_same(second, c.ref(eng, image, sp, NO_LABELS))
    with nothing_left(alive):
        with pytest.raises(ValueError) as exc:
            inf.apply_roi(image, spacing=sp)
    assert str(exc.value) == "ROI: the labels hold no voxel of the kept label values"
    assert len(empty.calls) == 8 and empty.applied == 0


def test_no_labelled_voxel_on_the_host_path(empty, alive):
    image, sp = forms(IMAGE)["lps"]
    empty.reset()
    empty.inf._shard = _DummyShard()
    try:
        with nothing_left(alive):
            labels, closed = empty.inf.apply_closed(image, radius_mm=2.0)
            _, med = empty.inf.apply_denoised(image, method="median")
            _, gau = empty.inf.apply_denoised(image, method="gaussian", sigma_mm=1.2)
    finally:
        empty.inf._shard = None
    assert not labels.any() and same_array(closed, labels) and not np.shares_memory(closed, labels)
    assert same_array(med, IMAGE) and same_array(gau, IMAGE.astype(np.float32))
    assert empty.calls == [] and empty.applied == 3


def test_unmasked_filter_ignores_the_labels(empty, alive):
    with nothing_left(alive):
        labels, filtered = empty.inf.apply_denoised(IMAGE, method="median", size=(1, 3, 3), masked=False)
    assert not labels.any()
    assert_same(filtered, filters.median(IMAGE, (1, 3, 3), engine=empty.engine))


VOLUME = volume_io.Volume(IMAGE, SPACING[::-1], ORIGIN, DIRECTION)
SPACING_TWICE = "spacing is taken from the image (Volume / SimpleITK image): do not pass it as well"
ERRORS = [(c.method, dict(method=k) if c.method == "apply_denoised" else {}, IMAGE[0], ValueError,
           f"{c.method}: a 3-D volume is needed, got shape (12, 9)") for k, c in CASES.items() if k != "gaussian"]
ERRORS += [(c.method, dict(spacing=SPACING), VOLUME, ValueError, SPACING_TWICE) for k, c in CASES.items() if c.takes_spacing and k != "gaussian"]
ERRORS += [
    ("apply_with_texture", dict(aggregate="x"), IMAGE, ValueError, "aggregate: 'average' or 'merge', got 'x'"),
    ("apply_denoised", dict(method="x"), IMAGE, ValueError, "method: 'median' or 'gaussian', got 'x'"),
    ("apply_denoised", dict(method="gaussian"), IMAGE, ValueError, "apply_denoised: method 'gaussian' needs sigma_mm"),
    ("apply_mesh", dict(smooth=-1), IMAGE, ValueError, "smooth: a number of iterations >= 0, got -1"),
    ("apply_mesh", {}, IMAGE[:0], ValueError, "apply_mesh: the volume has no slice"),
]


@pytest.mark.parametrize("method,kw,image,exc_type,message", ERRORS, ids=[f"{m}-{i}" for i, (m, *_) in enumerate(ERRORS)])
def test_argument_errors_keep_their_type_and_message(lung, alive, method, kw, image, exc_type, message):
    lung.reset()
    with nothing_left(alive):
        with pytest.raises(exc_type, match=re.escape(message)) as exc:
            getattr(lung.inf, method)(image, **kw)
    assert type(exc.value) is exc_type and str(exc.value) == message
    assert lung.calls == []


@pytest.mark.parametrize("form", ("array", "permuted"))
@pytest.mark.parametrize("case", list(CASES))
def test_a_failing_analysis_leaves_no_device_memory_behind(lung, alive, monkeypatch, case, form):
    c = CASES[case]
    image, sp = forms(IMAGE)[form]

    def boom(*a, **k):
        raise Boom(c.boom)

    monkeypatch.setattr(lung.engine, c.boom, boom)
    lung.reset()
    with nothing_left(alive):
        with pytest.raises(Boom):
            c.call(lung.inf, image, sp)
    assert len(lung.calls) == 1
    monkeypatch.undo()  # (the allocation counter with it: the next call is only checked for its results)
    labels, second = c.call(lung.inf, image, sp)
    assert np.array_equal(labels, LABELS)
    assert_same(second, c.ref(lung.engine, image, sp, LABELS))
