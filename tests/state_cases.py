"""Shared case table of the state tests (tests/test_state_emu.py on the emulator, tests/test_gpu_state.py on the GPU): one entry per
device entry point of include/lungmask_hip.h.  A case is a function run(ctx, shape) -> tuple of numpy arrays / plain values that
calls the `_dev` form with every caller buffer taken from ctx.mem:

    PlainMem   every buffer an allocation of its own (what every other test does);
    ArenaMem   every buffer a DeviceView inside ONE allocation filled with 0xA5, 4096 guard bytes on either side of each view
               (4096 keeps the 256-byte alignment of a plain allocation), optionally shifted by k elements so that the base is
               element-aligned only.  finish() checks that nothing outside the output views has changed: guards AND inputs.

    AheadMem   PlainMem whose uploads run on the stream of a second engine: lm_copy_h2d waits for the stream of the engine it is
               given, so an input copied through the engine under test would make the host wait for everything enqueued there.

Results are compared engine against engine, byte for byte (floats through .tobytes(), NaN payloads included).  No field is compared
with a tolerance: none needed one, the float64 distance sums of lm_label_agreement_dev included.

Deferred collection (check_deferred): a case ends in ctx.results(...); in deferred mode that records its items and returns a Pending,
and only Pending.collect() waits for the engine and downloads.  Between the two the host is free to enqueue the next call."""
import ctypes as C
import functools
import time

import numpy as np

from lungmask_amd import _native as nat
from oracle import unet_oracle as uo

GUARD = 4096
FILL = 0xA5

SMALL = [(5, 33, 70), (3, 7, 600), (4, 16, 64)]  # ragged width across one ballot word; rows of more than two 256-voxel pieces; every vector path
DIRTY = [(9, 48, 100)]
VEC = [(4, 16, 64)]       # the width alone selects the vector paths: what the misaligned bases run at
STRESS = [(24, 96, 80)]   # many workgroups on the accumulators (GPU repeatability screen)

SPACING = (2.5, 0.7421875, 0.7421875)


# ---------------------------------------------------------------------------------------------------------------- memory providers
class PlainMem:
    def __init__(self, eng):
        self.eng, self.bufs = eng, []

    def _keep(self, d):
        self.bufs.append(d)
        return d

    def inp(self, arr):
        return self._keep(self.eng.to_device(np.ascontiguousarray(arr)))

    inout = inp

    def out(self, shape, dtype):
        return self._keep(self.eng.empty(shape, dtype))

    def finish(self):
        self.eng.sync()

    def close(self):
        for d in self.bufs:
            d.free()
        self.bufs = []


class AheadMem(PlainMem):
    """PlainMem for a host that runs ahead of the device: allocations are the engine's (hipMalloc waits for nothing), the input
    copies go through `uploader` -- another engine, i.e. another stream -- and are complete when inp() returns."""

    def __init__(self, eng, uploader):
        PlainMem.__init__(self, eng)
        self.uploader = uploader

    def inp(self, arr):
        arr = np.ascontiguousarray(arr)
        d = self._keep(self.eng.empty(arr.shape, arr.dtype))
        if d.nbytes:
            self.eng.L.check(self.eng.L.lib.lm_copy_h2d(self.uploader.h, d.ptr, arr.ctypes.data, d.nbytes), "lm_copy_h2d")
        return d

    inout = inp


class ArenaMem:
    """Views with guard bands inside one allocation.  k: every view starts k elements behind a 4096-byte boundary."""

    def __init__(self, eng, k=0, nbytes=8 << 20):
        self.eng, self.k, self.nbytes = eng, int(k), int(nbytes)
        self.host = np.full(self.nbytes, FILL, np.uint8)
        self.writable = np.zeros(self.nbytes, bool)
        self.arena = eng.to_device(self.host)
        self.cursor = 0
        self.views = []

    def _view(self, shape, dtype):
        dt = np.dtype(dtype)
        shape = tuple(int(s) for s in shape)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
        off = (self.cursor + GUARD - 1) // GUARD * GUARD + GUARD + self.k * dt.itemsize
        self.cursor = off + nbytes + GUARD
        assert self.cursor + GUARD <= self.nbytes, f"arena of {self.nbytes} bytes is too small"
        v = self.arena.view(off, shape, dt)
        assert v.ptr % dt.itemsize == 0 and (self.k == 0 or v.ptr % 16 != 0 or dt.itemsize >= 16)
        self.views.append((off, nbytes))
        return v, off, nbytes

    def inp(self, arr, writable=False):
        arr = np.ascontiguousarray(arr)
        v, off, nbytes = self._view(arr.shape, arr.dtype)
        self.host[off:off + nbytes] = arr.reshape(-1).view(np.uint8)
        self.writable[off:off + nbytes] = writable
        if nbytes:
            v.upload(arr)
        return v

    def inout(self, arr):
        return self.inp(arr, writable=True)

    def out(self, shape, dtype):
        v, off, nbytes = self._view(shape, dtype)
        self.writable[off:off + nbytes] = True
        return v

    def finish(self):
        """Guards intact and inputs unchanged: every byte outside the output views is what was put there."""
        self.eng.sync()
        got = self.arena.download()
        bad = np.flatnonzero((got != self.host) & ~self.writable)
        if bad.size:
            b = int(bad[0])
            near = min(self.views, key=lambda v: min(abs(b - v[0]), abs(b - (v[0] + v[1]))))
            raise AssertionError(f"{bad.size} bytes outside the outputs changed; first at arena offset {b} (value {int(got[b]):#x}, "
                                 f"expected {int(self.host[b]):#x}), nearest view [{near[0]}, {near[0] + near[1]})")

    def close(self):
        self.arena.free()


class Ctx:
    """What a case sees: the engine, the memory provider, the model (loaded on first use) and a peer engine (slab protocol)."""

    def __init__(self, eng, mem, deferred=False):
        self.eng, self.mem, self.deferred = eng, mem, deferred

    def model(self):
        if not getattr(self.eng, "_state_model", False):
            self.eng.load_state_dict(0, uo.synthetic_state_dict(3))
            self.eng._state_model = True
        return 3

    def peer(self):
        if getattr(self.eng, "_state_peer", None) is None:
            self.eng._state_peer = nat.Engine(0, self.eng.L)
        return self.eng._state_peer

    def results(self, *items):
        """finish() the memory provider, then download the device arrays among `items` (dicts and plain values pass through).
        Deferred mode: -> the Pending that does so when asked."""
        pending = Pending(self.mem, items)
        return pending if self.deferred else pending.collect()


class Pending:
    """The results of a case whose calls have been made and not waited for."""

    def __init__(self, mem, items):
        self.mem, self.items = mem, items

    def collect(self):
        self.mem.finish()
        return tuple(it.download() if isinstance(it, nat.DeviceArray) else it for it in self.items)


def engines_of(eng):
    """The engine and the peer a case created on it: what a test fills and closes."""
    peer = getattr(eng, "_state_peer", None)
    return [eng] + ([peer] if peer is not None else [])


def uploader_of(eng):
    """The second engine whose stream carries the input copies of AheadMem."""
    if getattr(eng, "_state_uploader", None) is None:
        eng._state_uploader = nat.Engine(0, eng.L)
    return eng._state_uploader


def close_engine(eng):
    up = getattr(eng, "_state_uploader", None)
    for e in ([up] if up is not None else []) + engines_of(eng)[::-1]:
        e.close()
    eng._state_peer = eng._state_uploader = None


# ---------------------------------------------------------------------------------------------------------------- comparison
def flatten(res, path=""):
    """-> [(path, bytes)]: arrays as dtype, shape and raw bytes; dicts by sorted key; anything else by repr."""
    if isinstance(res, np.ndarray):
        return [(path, repr((res.dtype.str, res.shape)).encode() + np.ascontiguousarray(res).tobytes())]
    if isinstance(res, dict):
        return [x for k in sorted(res) for x in flatten(res[k], f"{path}.{k}")]
    if isinstance(res, (tuple, list)):
        return [x for i, v in enumerate(res) for x in flatten(v, f"{path}[{i}]")]
    return [(path, repr(res).encode())]


def assert_same(got, want, what):
    g, w = flatten(got), flatten(want)
    assert [p for p, _ in g] == [p for p, _ in w], (what, "different structure")
    diff = [p for (p, a), (_, b) in zip(g, w) if a != b]
    assert not diff, f"{what}: differs from the new engine's first call in {diff}"


# ---------------------------------------------------------------------------------------------------------------- inputs
def _once(fn):
    """The inputs are functions of the shape alone: each is made once and shared, read-only, by every run of its case (the baseline's
    included) -- check_deferred needs the host to be quick between the ballast and the call it is put in front of."""
    @functools.lru_cache(maxsize=None)
    def cached(*args, **kw):
        out = fn(*args, **kw)
        out.flags.writeable = False
        return out
    return cached


def seed_of(shape, salt=0):
    return int(shape[0]) * 1000003 + int(shape[1]) * 1009 + int(shape[2]) + 7919 * salt


@_once
def blob_labels(shape, salt=0, nlab=4):
    from oracle.make_golden import random_blobs

    return random_blobs(np.random.default_rng(seed_of(shape, salt)), shape, nlab, 18, 0.3)


@_once
def lattice(shape):
    """check_postprocess_noise's lattice at any shape: on every other slice each voxel is a region of its own."""
    n, h, w = shape
    lat = np.zeros(shape, np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    for z in range(0, n, 2):
        lat[z] = 1 + (xx % 2) + 2 * (yy % 2)
    lat[min(2, n - 1), h // 4:h // 4 + 4, w // 4:w // 4 + 4] = 1  # one larger region for the small ones to merge into
    return lat


def boxes_for(rng, n, h, w):
    out = []
    for _ in range(n):
        r0, c0 = int(rng.integers(0, h // 2)), int(rng.integers(0, w // 2))
        out.append([r0, c0, int(rng.integers(r0 + 2, h + 1)), int(rng.integers(c0 + 2, w + 1))])
    out[0] = [0, 0, h, w]
    return np.asarray(out, np.int32)


# ---------------------------------------------------------------------------------------------------------------- network
def _forward(precision, want_logp):
    def run(ctx, shape):
        c = ctx.model()
        b, h, w = shape
        x = np.random.default_rng(seed_of(shape)).random(shape, dtype=np.float32)
        ctx.eng.set_precision(precision)
        try:
            xd = ctx.mem.inp(x)
            ld = ctx.mem.out(shape, np.uint8)
            pd = ctx.mem.out((b, c, h, w), np.float32) if want_logp else None
            ctx.eng.forward_dev(0, xd, ld, pd)
            return ctx.results(ld, pd)
        finally:
            ctx.eng.set_precision("split_f16")
    return run


def forward_batches(ctx, shape):
    ctx.model()
    n, h, w = shape
    x = np.random.default_rng(seed_of(shape, 1)).random(shape, dtype=np.float32)
    xd = ctx.mem.inp(x)
    ld = ctx.mem.out(shape, np.uint8)
    e = ctx.eng
    e.L.check(e.L.lib.lm_forward_batches_dev(e.h, 0, xd.ptr, n, h, w, 2, ld.ptr), "lm_forward_batches_dev")  # two lanes, ragged last batch
    return ctx.results(ld)


def forward_batches_f32(ctx, shape):
    """lm_forward_batches_dev on the exact-fp32 kernels (no range flag to read back: the call only enqueues), two lanes, batches of
    two with a ragged last one -- and a consumer of the labels on the engine's stream right behind it, which is what a caller of an
    enqueue-only entry point writes: lane 1's labels reach it only through the join at the end of the batch loop."""
    ctx.model()
    n, h, w = shape
    rng = np.random.default_rng(seed_of(shape, 17))
    xd = ctx.mem.inp(rng.random(shape, dtype=np.float32))
    bd = ctx.mem.inp(boxes_for(rng, n, h + 9, w + 5))
    ld = ctx.mem.out(shape, np.uint8)
    od = ctx.mem.out((n, h + 9, w + 5), np.uint8)
    e = ctx.eng
    e.set_precision("f32")
    try:
        e.L.check(e.L.lib.lm_forward_batches_dev(e.h, 0, xd.ptr, n, h, w, 2, ld.ptr), "lm_forward_batches_dev")
        e.reshape_mask_dev(ld, bd, od)
        return ctx.results(ld, od)
    finally:
        e.set_precision("split_f16")


@_once
def _phantom(shape, dtype):
    from oracle import prepost_oracle as po

    vol = po.phantom(*shape, seed=seed_of(shape) % 1000)
    if np.dtype(dtype).kind == "f":
        vol = (vol + np.random.default_rng(seed_of(shape, 2)).normal(0, 0.37, shape)).astype(dtype)
    return vol


def apply_labels(ctx, shape):
    ctx.model()
    vd = ctx.mem.inp(_phantom(shape, np.int16))
    od = ctx.mem.out(shape, np.uint8)
    ctx.eng.apply_dev(0, vd, od, batch_size=2)
    return ctx.results(od)


def apply_f32(ctx, shape):
    """lm_apply_dev on the exact-fp32 kernels without volume post-processing and fill model: no round trip at all.  More than eight
    slices at batch_size 2: the tail is pre-processed on the copy stream, the last batch is ragged."""
    ctx.model()
    vd = ctx.mem.inp(_phantom(shape, np.int16))
    od = ctx.mem.out(shape, np.uint8)
    ctx.eng.set_precision("f32")
    try:
        ctx.eng.apply_dev(0, vd, od, batch_size=2, volume_postprocessing=False)
        return ctx.results(od)
    finally:
        ctx.eng.set_precision("split_f16")


def apply_probs(ctx, shape):
    c = ctx.model()
    vd = ctx.mem.inp(_phantom(shape, np.int16))
    od = ctx.mem.out(shape, np.uint8)
    pd = ctx.mem.out((c,) + tuple(shape), np.float32)
    ctx.eng.apply_probs_dev(0, vd, pd, od, batch_size=2)
    return ctx.results(od, pd)


# ---------------------------------------------------------------------------------------------------------------- pre / un-crop
def _preprocess(dtype):
    def run(ctx, shape):
        n, h, w = shape
        vd = ctx.mem.inp(_phantom(shape, dtype))
        bb = ctx.mem.out((n, 4), np.int32)
        xf = ctx.mem.out((n, 64, 64), np.float32)
        xi = ctx.mem.out((n, 64, 64), np.int16) if np.dtype(dtype).kind == "i" else None
        bm = ctx.mem.out(shape, np.uint8)
        ctx.eng.preprocess_dev(vd, bb, xf, xi, bm, resolution=(64, 64))
        return ctx.results(bb, xf, xi, bm)
    return run


def reshape_mask(ctx, shape):
    n, h, w = shape
    rng = np.random.default_rng(seed_of(shape, 3))
    md = ctx.mem.inp(rng.integers(0, 4, (n, 64, 64)).astype(np.uint8))
    bd = ctx.mem.inp(boxes_for(rng, n, h, w))
    od = ctx.mem.out(shape, np.uint8)
    ctx.eng.reshape_mask_dev(md, bd, od)
    return ctx.results(od)


def uncrop_probs(ctx, shape):
    n, h, w = shape
    rng = np.random.default_rng(seed_of(shape, 4))
    z = rng.normal(0, 2, (n, 3, 32, 32))
    logp = (z - np.log(np.exp(z).sum(1, keepdims=True))).astype(np.float32)
    ld = ctx.mem.inp(logp)
    bd = ctx.mem.inp(boxes_for(rng, n, h, w))
    o32 = ctx.mem.out((3, n, h, w), np.float32)
    o16 = ctx.mem.out((3, n, h, w), np.float16)
    ctx.eng.uncrop_probs_dev(ld, bd, o32)
    ctx.eng.uncrop_probs_dev(ld, bd, o16)
    return ctx.results(o32, o16)


def reorient(ctx, shape):
    n, h, w = shape
    a = np.random.default_rng(seed_of(shape, 5)).integers(-2000, 2000, shape).astype(np.int16)
    sd = ctx.mem.inp(a)
    od = ctx.mem.out((w, n, h), np.int16)
    ctx.eng.reorient_dev(sd, (2, 0, 1), (True, False, True), out=od)
    return ctx.results(od)


# ---------------------------------------------------------------------------------------------------------------- post-processing
def postprocess_blobs(ctx, shape):
    ld = ctx.mem.inout(blob_labels(shape))
    ctx.eng.postprocess_dev(ld, spare=(4,))
    return ctx.results(ld, ctx.eng.postprocess_info()["regions"])


def postprocess_lattice(ctx, shape):
    ld = ctx.mem.inout(lattice(shape))
    ctx.eng.postprocess_dev(ld, skip_below=1)
    info = ctx.eng.postprocess_info()
    return ctx.results(ld, info["regions"], info["boundary_records"])


def bbox_3d(ctx, shape):
    n, h, w = shape
    m = np.zeros(shape, np.uint8)
    m[n // 3:, h // 4:h - 2, 3:w - 5] = blob_labels(shape, 1)[n // 3:, h // 4:h - 2, 3:w - 5]
    md = ctx.mem.inp(m)
    bb = (C.c_int32 * 6)()
    e = ctx.eng
    e.L.check(e.L.lib.lm_bbox3d_dev(e.h, md.ptr, n, h, w, 2, bb), "lm_bbox3d_dev")
    return ctx.results([int(v) for v in bb])


def keep_largest(ctx, shape):
    md = ctx.mem.inout((blob_labels(shape, 2) > 0).astype(np.uint8))
    area = ctx.eng.keep_largest_dev(md)
    return ctx.results(md, area)


def fuse(ctx, shape):
    """lm_fuse_dev and its two halves lm_label_max_dev + lm_fuse_spare_dev."""
    res_l, res_r = blob_labels(shape, 3, 5), blob_labels(shape, 4, 2)
    l1, l2, rd = ctx.mem.inout(res_l), ctx.mem.inout(res_l), ctx.mem.inp(res_r)
    e, lib = ctx.eng, ctx.eng.L.lib
    sp, mx = C.c_int(), C.c_int()
    e.L.check(lib.lm_fuse_dev(e.h, l1.ptr, rd.ptr, l1.nbytes, C.byref(sp)), "lm_fuse_dev")
    e.L.check(lib.lm_label_max_dev(e.h, l2.ptr, l2.nbytes, C.byref(mx)), "lm_label_max_dev")
    e.L.check(lib.lm_fuse_spare_dev(e.h, l2.ptr, rd.ptr, l2.nbytes, mx.value + 1), "lm_fuse_spare_dev")
    return ctx.results(l1, sp.value, l2, mx.value)


def fuse_spare(ctx, shape):
    """lm_fuse_spare_dev alone, with the spare label given: one launch, nothing read back."""
    ld, rd = ctx.mem.inout(blob_labels(shape, 3, 5)), ctx.mem.inp(blob_labels(shape, 4, 2))
    e = ctx.eng
    e.L.check(e.L.lib.lm_fuse_spare_dev(e.h, ld.ptr, rd.ptr, ld.nbytes, 6), "lm_fuse_spare_dev")
    return ctx.results(ld)


def slab_protocol(ctx, shape):
    """The slab protocol with two engines (its device buffers are the protocol's own: no guard bands here)."""
    from lungmask_amd.pipeline import postprocess_slabs_in_process

    n = shape[0]
    out = postprocess_slabs_in_process([ctx.eng, ctx.peer()], blob_labels(shape, 5), [0, (n + 1) // 2, n], spare=(4,))
    return ctx.results(out)


# ---------------------------------------------------------------------------------------------------------------- analysis
@_once
def _image(shape, dtype, salt=0):
    from test_filters_emu import volume

    return volume(shape, dtype, seed_of(shape, salt) % 100000)


@_once
def _lungs(shape, salt=0, border=True):
    from test_filters_emu import lung_labels

    return lung_labels(shape, seed_of(shape, salt) % 100000, border)


def label_stats(ctx, shape):
    ld, vd = ctx.mem.inp(_lungs(shape)), ctx.mem.inp(_image(shape, np.float32))
    return ctx.results(ctx.eng.label_stats_dev(ld, vd, 3))


def texture(ctx, shape):
    from test_texture_emu import random_case

    lab, vol = random_case(np.random.default_rng(seed_of(shape, 6)), shape, 3)
    ld, vd = ctx.mem.inp(lab), ctx.mem.inp(vol)
    return ctx.results(ctx.eng.texture_dev(ld, vd, 3))


@_once
def _metric_blobs(shape, salt):
    from test_metrics_emu import blobs

    return blobs(np.random.default_rng(seed_of(shape, salt)), shape, 4, extra=1)


def edt(ctx, shape):
    fd = ctx.mem.inp((_metric_blobs(shape, 7) > 0).astype(np.uint8))
    od = ctx.mem.out(shape, np.float32)
    ctx.eng.edt_dev(fd, SPACING, out=od)
    return ctx.results(od)


def label_agreement(ctx, shape):
    ad, bd = ctx.mem.inp(_metric_blobs(shape, 8)), ctx.mem.inp(_metric_blobs(shape, 9))
    return ctx.results(ctx.eng.label_agreement_dev(ad, bd, 4, SPACING, (50, 95)))


def roi(ctx, shape):
    """lm_roi_plan_dev + lm_roi_dev with a dilation (the distance workspace) and a resampling grid."""
    from test_roi_emu import blobs, volume

    s = seed_of(shape, 10) % 100000
    vd, ld = ctx.mem.inp(volume(shape, np.int16, s)), ctx.mem.inp(blobs(shape, s))
    img, lab, info = ctx.eng.roi_dev(vd, ld, spacing=SPACING, spacing_out=1.0, margin_mm=4.0, dilate_mm=2.0, keep=(1,),
                                     out=lambda dims: (ctx.mem.out(dims, np.float32), ctx.mem.out(dims, np.uint8)))
    return ctx.results(img, lab, info["bbox"], info["out_dims"])


def _mesh(smooth):
    def run(ctx, shape):
        from test_roi_emu import blobs

        ld = ctx.mem.inp(blobs(shape, seed_of(shape, 11) % 100000))
        verts, quads, info = ctx.eng.mesh_dev(ld, smooth=smooth,
                                              out=lambda nv, nq: (ctx.mem.out((nv, 3), np.float32), ctx.mem.out((nq, 4), np.int32)))
        return ctx.results(verts, quads, info["bbox"])
    return run


def nearest_label(ctx, shape):
    ld = ctx.mem.inp(_lungs(shape, 12, border=False))
    near, d2 = ctx.eng.nearest_label_dev(ld, SPACING, out=ctx.mem.out(shape, np.uint8), d2_out=ctx.mem.out(shape, np.float32))
    near_ws = ctx.eng.nearest_label_dev(ld, SPACING, keep=(1, 3), out=ctx.mem.out(shape, np.uint8))  # distances in the engine's workspace
    return ctx.results(near, d2, near_ws)


def morph_close(ctx, shape):
    ld = ctx.mem.inp(_lungs(shape, 13, border=False))
    od = ctx.mem.out(shape, np.uint8)
    _, changed = ctx.eng.morph_dev(ld, "close", 2.0, spacing=SPACING, out=od)
    return ctx.results(od, changed)


def components(ctx, shape):
    """lm_components_dev + lm_component_table_dev + lm_relabel_dev."""
    from test_components_emu import random_case

    labels, image = random_case(shape, seed_of(shape, 14) % 100000)
    ld, vd = ctx.mem.inp(labels), ctx.mem.inp(image)
    ids, total, counts = ctx.eng.components_dev(ld, vd, hu_range=(-950, None), out=ctx.mem.out(shape, np.int32))
    rows, t2 = ctx.eng.component_table_dev(ids, ld, vd)
    lut = ctx.mem.inp(np.concatenate([[0], 1 + np.argsort(np.argsort(-rows["voxels"], kind="stable"), kind="stable")]).astype(np.int32))
    rel = ctx.eng.relabel_dev(ids, lut, out=ctx.mem.out(shape, np.int32))
    return ctx.results(ids, total, counts, rows, t2, rel)


def filter_median(ctx, shape):
    vd, ld = ctx.mem.inp(_image(shape, np.float32, 15)), ctx.mem.inp(_lungs(shape, 15))
    od = ctx.mem.out(shape, np.float32)
    ctx.eng.filter_dev(vd, ld, kind="median", size=5, out=od)
    return ctx.results(od)


def filter_separable(ctx, shape):
    from test_filters_emu import random_taps

    vd, ld = ctx.mem.inp(_image(shape, np.int16, 16)), ctx.mem.inp(_lungs(shape, 16, border=False))
    od = ctx.mem.out(shape, np.float32)
    ctx.eng.filter_dev(vd, ld, kind="separable", taps=[random_taps(r, 16, nonneg=True) for r in (1, 2, 3)], indicator=(-950, None), out=od)
    return ctx.results(od)


def filter_whole(ctx, shape):
    """lm_filter_dev over the whole volume (no labels: no bounding box to read back first), median and separable."""
    from test_filters_emu import random_taps

    vd = ctx.mem.inp(_image(shape, np.int16, 18))
    om, os_ = ctx.mem.out(shape, np.int16), ctx.mem.out(shape, np.float32)
    ctx.eng.filter_dev(vd, None, kind="median", size=3, out=om)
    ctx.eng.filter_dev(vd, None, kind="separable", taps=[random_taps(r, 18, nonneg=True) for r in (2, 1, 3)], out=os_)
    return ctx.results(om, os_)


# ---------------------------------------------------------------------------------------------------------------- resampling, registration
def moving_shape(shape):
    """The moving volume of a paired case: another shape than the fixed one on every axis."""
    n, h, w = shape
    return (n + 1, h - 3, w + 5)


def oblique():
    """test_register_emu.rot_scale(): a rotation with unequal scales and a shift, under which some samples leave the moving volume."""
    from test_register_emu import rot_scale

    return rot_scale()


@_once
def _reg_volume(shape, dtype, salt=0):
    from test_register_emu import volume

    return volume(shape, dtype, seed_of(shape, salt) % 100000)


@_once
def _field(shape, salt=0):
    """test_deform_emu.make_field's random field (test_field_emu.rand_field is the same one): a few voxels' amplitude in the units of
    SPACING, so that some samples fall outside and the map folds in places."""
    from test_deform_emu import make_field

    return make_field("random", shape, seed_of(shape, salt) % 100000, SPACING)


def resample_grid(shape):
    """An output grid larger than the source along z and x and smaller along y, the scaling that maps one onto the other, and
    rot_scale()'s shift: the first output row samples outside."""
    n, h, w = shape
    out = (n + 2, h - 3, w + 7)
    return out, np.diag([n / out[0], h / out[1], w / out[2]]), oblique()[1]


def spline_prefilter(ctx, shape):
    vd = ctx.mem.inp(_reg_volume(shape, np.int16, 20))
    cd = ctx.mem.out(shape, np.float64)
    ctx.eng.spline_prefilter_dev(vd, out=cd)
    return ctx.results(cd)


def _resample(mode, src_dtype, out_dtype, salt):
    def run(ctx, shape):
        dims, A, b = resample_grid(shape)
        sd = ctx.mem.inp(_reg_volume(shape, src_dtype, salt))
        od = ctx.mem.out(dims, out_dtype)
        ctx.eng.resample_dev(sd, A, b, dims, mode, fill=3, dtype=out_dtype, out=od)
        return ctx.results(od)
    return run


def joint_hist(ctx, shape):
    A, b = oblique()
    fd, md = ctx.mem.inp(_reg_volume(shape, np.int16, 24)), ctx.mem.inp(_reg_volume(moving_shape(shape), np.float32, 25))
    ld = ctx.mem.inp(_reg_volume(shape, np.uint8, 26))
    od = ctx.mem.out((32 * 32 + 4,), np.int64)  # (the four counts live in its tail)
    ctx.eng.joint_hist_dev(fd, md, A, b, 32, step=(1, 2, 2), mode="linear", labels=ld, keep=(1, 3, 5), out=od)
    return ctx.results(od)


def warp(ctx, shape):
    """lm_warp_dev in its three forms: linear through a field, cubic from lm_spline_prefilter_dev's coefficients, nearest without a
    field."""
    A, b = oblique()
    src = moving_shape(shape)
    sd, ud = ctx.mem.inp(_reg_volume(src, np.int16, 27)), ctx.mem.inp(_field(shape, 28))
    cd = ctx.mem.out(src, np.float64)
    lin, cub, near = ctx.mem.out(shape, np.float32), ctx.mem.out(shape, np.int16), ctx.mem.out(shape, np.int16)
    e = ctx.eng
    e.warp_dev(sd, ud, A, b, shape, "linear", spacing=SPACING, out=lin)
    e.spline_prefilter_dev(sd, out=cd)
    e.warp_dev(cd, ud, A, b, shape, "cubic", dtype=np.int16, spacing=SPACING, out=cub)
    e.warp_dev(sd, None, A, b, shape, "nearest", out=near)
    return ctx.results(lin, cd, cub, near)


def demons_step(ctx, shape):
    A, b = oblique()
    fd, md = ctx.mem.inp(_reg_volume(shape, np.int16, 29)), ctx.mem.inp(_reg_volume(moving_shape(shape), np.float32, 30))
    ld, ud = ctx.mem.inp(_reg_volume(shape, np.uint8, 31)), ctx.mem.inp(_field(shape, 32))
    od, cd = ctx.mem.out((3,) + shape, np.float32), ctx.mem.out((5,), np.int64)
    ctx.eng.demons_step_dev(fd, md, ud, od, cd, A, b, spacing=SPACING, inv_k2=0.25, labels=ld, keep=(1, 2, 4))
    return ctx.results(od, cd)


def jacobian(ctx, shape):
    ud = ctx.mem.inp(_field(shape, 33))
    od, cd = ctx.mem.out(shape, np.float32), ctx.mem.out((2,), np.int64)
    ctx.eng.jacobian_dev(ud, SPACING, out=od, counts=cd)
    return ctx.results(od, cd)


@_once
def _lcc_pair(shape):
    """test_lcc_emu.pair as one array [2][n][h][w], with the non-finite voxels of its run_nan_and_labels spread over the volume."""
    from test_lcc_emu import pair

    fm = np.stack(pair(shape, seed_of(shape, 34) % 100000))
    f, m = fm[0].reshape(-1), fm[1].reshape(-1)
    m[5::41], m[11::97], f[17::89] = np.nan, -np.inf, np.nan
    return fm


@_once
def _pair_labels(shape, salt):
    from test_pair_emu import labels_of

    return labels_of(shape, seed_of(shape, salt) % 100000)


def lcc(ctx, shape):
    """lm_local_moments_dev, then lm_lcc_step_dev on its sums."""
    A, b = oblique()
    fm = _lcc_pair(shape)
    fd, md = ctx.mem.inp(fm[0]), ctx.mem.inp(fm[1])
    ld, ud = ctx.mem.inp(_pair_labels(shape, 35)), ctx.mem.inp(_field(shape, 36))
    sd = ctx.mem.out((6,) + shape, np.float64)
    od, cd = ctx.mem.out((3,) + shape, np.float32), ctx.mem.out((6,), np.int64)
    ctx.eng.local_moments_dev(fd, md, (1, 3, 2), out=sd)
    ctx.eng.lcc_step_dev(fd, md, sd, ud, od, cd, A, b, moving_shape(shape), spacing=SPACING, inv_k2=0.25, labels=ld, keep=(1, 3))
    return ctx.results(sd, od, cd)


def field_combine(ctx, shape):
    """All four pointers, `coord` aliasing `add` (the composition u1 + R u2 o T1 of the header's table)."""
    from test_field_emu import ROT

    A, b = oblique()
    sd = ctx.mem.inp(_field(moving_shape(shape), 37))
    ad, rd = ctx.mem.inp(_field(shape, 38)), ctx.mem.inp(_field(shape, 39))
    od, cd = ctx.mem.out((3,) + shape, np.float32), ctx.mem.out((4,), np.int64)
    ctx.eng.field_combine_dev(sd, shape, A, b, R=ROT, add=ad, coord=ad, ref=rd, alpha=0.75, beta=-1.25, spacing=SPACING, out=od, counts=cd)
    return ctx.results(od, cd)


@_once
def _lungish(shape, dtype, salt):
    from test_pair_emu import lungish

    return lungish(shape, dtype, seed_of(shape, salt) % 100000)


def pair_map(ctx, shape):
    A, b = oblique()
    fd, md = ctx.mem.inp(_lungish(shape, np.int16, 40)), ctx.mem.inp(_lungish(moving_shape(shape), np.float32, 41))
    ld, ud = ctx.mem.inp(_pair_labels(shape, 42)), ctx.mem.inp(_field(shape, 43))
    td = ctx.mem.out((4, nat.LM_PAIR_COLS), np.int64)
    cls, chg, jac = ctx.mem.out(shape, np.uint8), ctx.mem.out(shape, np.float32), ctx.mem.out(shape, np.float32)
    ctx.eng.pair_map_dev(fd, ld, md, ud, A, b, td, 4, spacing=SPACING, jac_scale=abs(float(np.linalg.det(A))), classes=cls, change=chg,
                         jacobian=jac)
    return ctx.results(td, cls, chg, jac)


# ---------------------------------------------------------------------------------------------------------------- vessels, skeleton, airways
SIGMAS = [(0.5, 0.5, 0.5), (1.0, 0.75, 1.0)]  # tap radii (2, 2, 2) and (4, 3, 4): within the 7-row shape
V_THRESHOLD = 0.05


@_once
def _vessel_volume(shape, dtype, salt):
    from test_vessels_emu import volume

    return volume(shape, dtype, seed_of(shape, salt) % 100000)


def hessian(ctx, shape):
    vd = ctx.mem.inp(_vessel_volume(shape, np.int16, 44))
    comp, eig = ctx.mem.out((6,) + shape, np.float32), ctx.mem.out((3,) + shape, np.float32)
    ctx.eng.hessian_dev(vd, SIGMAS[1], eigenvalues=True, out=comp, eig_out=eig)
    return ctx.results(comp, eig)


def vesselness(ctx, shape):
    vd = ctx.mem.inp(_vessel_volume(shape, np.float32, 45))
    v, sc = ctx.mem.out(shape, np.float32), ctx.mem.out(shape, np.uint8)
    ctx.eng.vesselness_dev(vd, SIGMAS, return_scale=True, out=v, scale_out=sc)
    return ctx.results(v, sc)


def vesselness_masked(ctx, shape):
    """lm_vesselness_dev inside labels, then lm_vessel_counts_dev and lm_vessel_mask_dev on its maps."""
    vd, ld = ctx.mem.inp(_vessel_volume(shape, np.int16, 46)), ctx.mem.inp(_lungs(shape, 46, border=False))
    v, sc, mask = ctx.mem.out(shape, np.float32), ctx.mem.out(shape, np.uint8), ctx.mem.out(shape, np.uint8)
    ctx.eng.vesselness_dev(vd, SIGMAS, lab=ld, keep=(1, 2), return_scale=True, out=v, scale_out=sc)
    counts = ctx.eng.vessel_counts_dev(v, sc, ld, V_THRESHOLD, n_labels=4)
    ctx.eng.vessel_mask_dev(v, ld, V_THRESHOLD, out=mask)
    return ctx.results(v, sc, counts, mask)


@_once
def _skeleton_volume(shape, salt):
    from test_skeleton_emu import random_volume

    return random_volume(shape, 0.35, seed_of(shape, salt) % 100000)


def skeleton(ctx, shape):
    """lm_skeleton_dev (out distinct from sel), lm_calibre_dev with its distances, lm_skeleton_points_dev sampling them."""
    e = ctx.eng
    sd, ld = ctx.mem.inp(_skeleton_volume(shape, 47)), ctx.mem.inp(blob_labels(shape, 48))
    kd = ctx.mem.out(shape, np.uint8)
    _, info = e.skeleton_dev(sd, out=kd)
    cls, d2 = ctx.mem.out(shape, np.uint8), ctx.mem.out(shape, np.float32)
    _, counts, _ = e.calibre_dev(kd, sd, (1.0, 2.0), spacing=SPACING, lab=ld, n_labels=5, return_distance=True, out=cls, d2_out=d2)
    total = info["skeleton"]  # (every entry of the three lists is written: cap is the number of points)
    idx, code, pd2 = ctx.mem.out((total,), np.int32), ctx.mem.out((total,), np.uint8), ctx.mem.out((total,), np.float32)
    found = e.skeleton_points_dev(kd, d2, index_out=idx, code_out=code, d2_out=pd2)[3]
    return ctx.results(kd, info, cls, counts, d2, idx, code, pd2, found)


AIRWAY_CAP = -800


@_once
def _airway_volume(shape, salt):
    from test_airway_emu import noise

    return noise(shape, -1100, -700, seed_of(shape, salt) % 100000)


def airway(ctx, shape):
    """lm_seed_cost_dev from two seeds (the first and the last passable voxel), then lm_airway_mask_dev with labels.  The number of
    rounds is printed, not compared: a brick reads its halo while the neighbour's workgroup of the same round may or may not have
    written it yet (airway_kernels.hip, "In place"), so the cost, the curve and the voxels reached are the unique fixed point's and
    the rounds it took are the schedule's -- on the emulator they vary with the load of the machine."""
    vol = _airway_volume(shape, 49)
    passable = np.flatnonzero(vol.reshape(-1) <= AIRWAY_CAP)
    seeds = [tuple(int(v) for v in np.unravel_index(passable[k], shape)) for k in (0, -1)]
    vd, ld = ctx.mem.inp(vol), ctx.mem.inp(_lungs(shape, 49))
    cost, mask = ctx.mem.out(shape, np.int16), ctx.mem.out(shape, np.uint8)
    _, curve, info = ctx.eng.seed_cost_dev(vd, seeds, cap_hu=AIRWAY_CAP, out=cost)
    assert info["converged"], info
    print(f"airway {shape}: {info['rounds']} rounds, {info['reached']} of {vol.size} voxels reached")
    _, counts = ctx.eng.airway_mask_dev(cost, -900, lab=ld, out=mask)
    return ctx.results(cost, curve, {k: v for k, v in info.items() if k != "rounds"}, mask, counts)


# ---------------------------------------------------------------------------------------------------------------- the table
class Case:
    """small / dirty / vec: the shapes of the small runs, of the dirtying run and of the misaligned-base run.  gpu_small: further
    small shapes for the GPU module only.  emu: the shapes on the emulator instead, as (small, dirty, vec) -- an emulated forward
    takes ten to thirty seconds, so the network entry points run there at one tiny shape or (None) not at all; the GPU module
    runs every shape.  workspace: the entry point keeps engine workspace (lm_debug_fill_workspaces must report bytes after it has
    run).  stress: the shape of the GPU repeatability screen (None: not part of it).  entries: the C entry points of
    include/lungmask_hip.h the case calls (tests/test_state_emu.py holds the header against them)."""

    def __init__(self, name, fn, small=SMALL, dirty=DIRTY, vec=VEC, gpu_small=(), emu=(), workspace=True, stress=None, arena=8 << 20,
                 entries=()):
        self.name, self.fn, self.workspace, self.stress, self.arena, self.emu = name, fn, workspace, stress, arena, emu
        self.entries = tuple(entries)
        self.gpu_shapes = dict(small=list(small) + list(gpu_small), dirty=list(dirty), vec=list(vec))
        self.emu_shapes = dict(small=list(small), dirty=list(dirty), vec=list(vec)) if emu == () else \
            None if emu is None else dict(zip(("small", "dirty", "vec"), (list(v) for v in emu)))

    def shapes(self, kind, gpu):
        return (self.gpu_shapes if gpu else self.emu_shapes)[kind]

    def run(self, eng, shapes, mem_factory=PlainMem):
        out = []
        for shape in shapes:
            mem = mem_factory(eng)
            try:
                out.append(self.fn(Ctx(eng, mem), tuple(shape)))
            finally:
                mem.close()
        return tuple(out)

    def enqueue(self, eng, shape, mem_factory=PlainMem):
        """The calls of one shape, not waited for -> (Pending, memory provider).  The caller collects, then closes the provider."""
        mem = mem_factory(eng)
        try:
            return self.fn(Ctx(eng, mem, deferred=True), tuple(shape)), mem
        except BaseException:
            mem.close()
            raise

    def __repr__(self):
        return self.name


# forward: 32 x 32 (16-wide geometry lower down), 48 x 80 (fallback kernel), 64 x 96 (persistent kernel); GPU only: 256 x 256 (fused
# first conv, fused head, split-K 1x1)
FWD = dict(small=[(2, 32, 32), (3, 48, 80), (2, 64, 96)], dirty=[(3, 64, 128)], vec=[(2, 32, 32)], gpu_small=[(3, 256, 256)], emu=None,
           arena=24 << 20)
FWD_EMU = dict(FWD, emu=([(1, 32, 32)], [(1, 48, 48)], [(1, 32, 32)]))  # the production arithmetic, once, on the emulator
APPLY = dict(small=[(5, 96, 80)], dirty=[(6, 112, 96)], vec=[(5, 96, 80)], emu=None, arena=16 << 20)

CASES = [
    Case("forward_f32_logp", _forward("f32", True), **FWD, entries=("lm_forward_dev",)),
    Case("forward_f32_labels", _forward("f32", False), **FWD, entries=("lm_forward_dev",)),
    Case("forward_split_f16_logp", _forward("split_f16", True), **FWD_EMU, entries=("lm_forward_dev",)),
    Case("forward_split_f16_labels", _forward("split_f16", False), **FWD, entries=("lm_forward_dev",)),
    Case("forward_batches", forward_batches, small=[(5, 32, 32)], dirty=[(7, 64, 96)], vec=[(5, 32, 32)], emu=None, entries=("lm_forward_batches_dev",)),
    # (256 x 256: the kernels fill the device, so the second lane -- the lowest stream priority -- is behind the first when the consumer starts)
    Case("forward_batches_f32", forward_batches_f32, small=[(11, 32, 32)], gpu_small=[(11, 256, 256)], dirty=[(13, 256, 256)], vec=[(11, 32, 32)], emu=None,
         arena=24 << 20, entries=("lm_forward_batches_dev", "lm_reshape_mask_dev")),
    Case("preprocess_int16", _preprocess(np.int16), workspace=False, entries=("lm_preprocess_dev",)),
    Case("preprocess_float32", _preprocess(np.float32), workspace=False, entries=("lm_preprocess_dev",)),
    Case("reshape_mask", reshape_mask, workspace=False, entries=("lm_reshape_mask_dev",)),
    Case("uncrop_probs", uncrop_probs, workspace=False, entries=("lm_uncrop_probs_dev",)),
    Case("reorient", reorient, workspace=False, entries=("lm_reorient_dev",)),
    Case("postprocess_blobs", postprocess_blobs, stress=STRESS, entries=("lm_postprocess_dev",)),
    Case("postprocess_lattice", postprocess_lattice, entries=("lm_postprocess_dev",)),
    Case("bbox_3d", bbox_3d, entries=("lm_bbox3d_dev",)),
    Case("keep_largest", keep_largest, entries=("lm_keep_largest_dev",)),
    Case("fuse", fuse, entries=("lm_fuse_dev", "lm_label_max_dev", "lm_fuse_spare_dev")),
    Case("fuse_spare", fuse_spare, workspace=False, entries=("lm_fuse_spare_dev",)),
    Case("label_stats", label_stats, stress=STRESS, entries=("lm_label_stats_dev",)),
    Case("texture", texture, stress=STRESS, entries=("lm_texture_dev",)),
    Case("edt", edt, workspace=False, entries=("lm_edt_dev",)),  # (works in place in its output)
    Case("label_agreement", label_agreement, stress=STRESS, entries=("lm_label_agreement_dev",)),
    Case("roi", roi, entries=("lm_roi_plan_dev", "lm_roi_dev")),
    Case("mesh_smooth0", _mesh(0), stress=STRESS, entries=("lm_mesh_plan_dev", "lm_mesh_dev")),
    Case("mesh_smooth2", _mesh(2), stress=STRESS, entries=("lm_mesh_plan_dev", "lm_mesh_dev")),
    Case("nearest_label", nearest_label, entries=("lm_nearest_label_dev",)),
    Case("morph_close", morph_close, stress=STRESS, entries=("lm_morph_dev",)),
    Case("components", components, stress=STRESS, entries=("lm_components_dev", "lm_component_table_dev", "lm_relabel_dev")),
    Case("filter_median", filter_median, stress=STRESS, entries=("lm_filter_dev",)),
    Case("filter_separable", filter_separable, entries=("lm_filter_dev",)),
    Case("filter_whole", filter_whole, entries=("lm_filter_dev",)),
    Case("spline_prefilter", spline_prefilter, workspace=False, entries=("lm_spline_prefilter_dev",)),  # (works in place in its output)
    Case("resample_linear", _resample("linear", np.float32, np.float32, 21), workspace=False, entries=("lm_resample_dev",)),
    Case("resample_cubic", _resample("cubic", np.int16, np.int16, 22), entries=("lm_resample_dev",)),  # (resample.coef)
    Case("resample_labels", _resample("label_linear", np.uint8, np.uint8, 23), workspace=False, entries=("lm_resample_dev",)),
    Case("joint_hist", joint_hist, stress=STRESS, entries=("lm_joint_hist_dev",)),  # (jhist.partial)
    Case("warp", warp, workspace=False, entries=("lm_warp_dev", "lm_spline_prefilter_dev")),  # (cubic from the caller's coefficients)
    Case("demons_step", demons_step, workspace=False, stress=STRESS, entries=("lm_demons_step_dev",)),
    Case("jacobian", jacobian, workspace=False, stress=STRESS, entries=("lm_jacobian_dev",)),
    Case("lcc", lcc, stress=STRESS, entries=("lm_local_moments_dev", "lm_lcc_step_dev")),  # (lcc.sums: radius (1, 3, 2) has line passes)
    Case("field_combine", field_combine, workspace=False, stress=STRESS, entries=("lm_field_combine_dev",)),
    Case("pair_map", pair_map, workspace=False, stress=STRESS, entries=("lm_pair_map_dev",)),
    Case("hessian", hessian, entries=("lm_hessian_dev",)),
    Case("vesselness", vesselness, entries=("lm_vesselness_dev",)),
    Case("vesselness_masked", vesselness_masked, stress=STRESS, entries=("lm_vesselness_dev", "lm_vessel_counts_dev", "lm_vessel_mask_dev")),
    Case("skeleton", skeleton, stress=STRESS, entries=("lm_skeleton_dev", "lm_calibre_dev", "lm_skeleton_points_dev")),
    Case("airway", airway, stress=STRESS, entries=("lm_seed_cost_dev", "lm_airway_mask_dev")),
    Case("apply", apply_labels, **APPLY, entries=("lm_apply_dev",)),
    Case("apply_f32", apply_f32, small=[(11, 96, 80)], dirty=[(13, 112, 96)], vec=[(11, 96, 80)], emu=None, arena=16 << 20, entries=("lm_apply_dev",)),
    Case("apply_probs", apply_probs, **APPLY, entries=("lm_apply_probs_dev",)),
    Case("slab_protocol", slab_protocol, vec=[]),
]
BY_NAME = {c.name: c for c in CASES}


def names(gpu):
    return [c.name for c in CASES if gpu or c.emu_shapes is not None]


# The entry points that return WITHOUT a round trip to the device -- no blocking copy, no stream or event synchronisation between
# the first launch and the return -- found by reading each launcher: case -> (entry point, where the code shows it).  After such a
# call the host is ahead of the device, and whatever it does next (the next call, growing a workspace, refilling a buffer) meets
# work still in flight.  check_deferred makes every one of them the first call of a window.  Everything else in CASES reads
# something back (region tables, counters, boxes, the f16 range flag) and so waits at least once inside the call.
ENQUEUE_ONLY = {
    "forward_f32_logp": ("lm_forward_dev, exact-fp32 kernels", "nn_engine.hip forward_guarded -> forward_range_check returns at `!h3`, before its copy and sync"),
    "forward_f32_labels": ("lm_forward_dev, exact-fp32 kernels", "as above; the split-f16 form reads the range flag back and is NOT in this table"),
    "forward_batches_f32": ("lm_forward_batches_dev, exact-fp32 kernels", "forward_guarded -> forward_batches: the lanes are joined by ev_join on the device, then `!h3`"),
    "apply_f32": ("lm_apply_dev, exact-fp32 kernels, no post-processing, no fill model",
                  "post_engine.hip inference(): vol_post == 0 -> forward_range_check (`!h3`), then launch_reshape_mask; apply_volume returns at fill_slot < 0"),
    "preprocess_int16": ("lm_preprocess_dev", "capi.hip: launch_bodymask_bbox + launch_resample_norm on e->stream, nothing else"),
    "preprocess_float32": ("lm_preprocess_dev", "as above"),
    "reshape_mask": ("lm_reshape_mask_dev", "capi.hip: one launch_reshape_mask on e->stream"),
    "uncrop_probs": ("lm_uncrop_probs_dev", "capi.hip: one launch_uncrop_probs on e->stream"),
    "reorient": ("lm_reorient_dev", "capi.hip: one launch_reorient on e->stream"),
    "edt": ("lm_edt_dev", "metrics_kernels.hip edt -> edt_box: edt_x_kernel and two edt_line_kernel launches, in place in the output"),
    "nearest_label": ("lm_nearest_label_dev", "morph_kernels.hip nearest_label -> nearest_box: three launches; morph.d2 is reserved, never read back"),
    "filter_whole": ("lm_filter_dev without labels", "filter_kernels.hip filter(): roi_plan only when masked; median_launch / sep_pass launch only"),
    "filter_median": ("lm_filter_dev with labels", "ONE round trip in FRONT (roi_plan -> bbox3d reads the box back), none behind: returns before the median has run"),
    "filter_separable": ("lm_filter_dev with labels", "as filter_median: the three passes are enqueued behind the box's round trip"),
    "fuse_spare": ("lm_fuse_spare_dev", "capi.hip: one fuse_labels launch (lm_fuse_dev reads the maximum back first and is NOT in this table)"),
    "spline_prefilter": ("lm_spline_prefilter_dev", "resample_kernels.hip spline_prefilter(): rs_convert and up to three prefilter launches, in place in the output"),
    "resample_linear": ("lm_resample_dev, LM_RS_LINEAR", "resample_kernels.hip resample() -> sample_common.h launch_gather: one launch"),
    "resample_cubic": ("lm_resample_dev, LM_RS_CUBIC", "resample(): resample.coef is reserved, spline_prefilter's launches fill it, launch_gather reads it; never read back"),
    "resample_labels": ("lm_resample_dev, LM_RS_LABEL_LINEAR", "as resample_linear: one gather_label_linear_kernel launch"),
    "joint_hist": ("lm_joint_hist_dev", "register_kernels.hip joint_hist(): jhist.partial is reserved; jh_kernel and jh_reduce_kernel write the caller's hist and counts"),
    "warp": ("lm_warp_dev, lm_spline_prefilter_dev", "deform_kernels.hip warp() -> launch_gather: one launch per call, no workspace; the prefilter as above"),
    "demons_step": ("lm_demons_step_dev", "deform_kernels.hip demons_step(): hipMemsetAsync on the caller's counts, one df_demons_kernel launch"),
    "jacobian": ("lm_jacobian_dev", "deform_kernels.hip jacobian(): hipMemsetAsync on the caller's counts, one df_jacobian_kernel launch"),
    "lcc": ("lm_local_moments_dev, lm_lcc_step_dev", "lcc_kernels.hip local_moments(): lcc.sums is reserved, up to three launches; lcc_step(): hipMemsetAsync + one launch"),
    "field_combine": ("lm_field_combine_dev", "field_kernels.hip field_combine(): hipMemsetAsync on the caller's counts, one fc_combine_kernel launch"),
    "pair_map": ("lm_pair_map_dev", "pair_kernels.hip pair_map(): hipMemsetAsync on the caller's table, one pm_pair_kernel launch"),
    "hessian": ("lm_hessian_dev without labels", "vessel_kernels.hip vessel_run(): roi_plan only when masked; vessel_scale reserves vessel.vol[0..8] and launches x, y, z"),
    "vesselness": ("lm_vesselness_dev without labels", "as hessian: two hipMemsetAsync on the outputs, then three launches per scale (vesselness_masked ends in "
                   "lm_vessel_counts_dev, which reads its counts back, and is NOT in this table)"),
}
assert set(ENQUEUE_ONLY) <= set(BY_NAME)


# ---------------------------------------------------------------------------------------------------------------- the checks
class Baselines:
    """name -> the small-shape results of a NEW engine's first call (computed once, never modified)."""

    def __init__(self, lib, gpu):
        self.lib, self.gpu, self.cache = lib, gpu, {}

    def __call__(self, name):
        if name not in self.cache:
            eng = nat.Engine(0, self.lib)
            try:
                self.cache[name] = BY_NAME[name].run(eng, BY_NAME[name].shapes("small", self.gpu))
            finally:
                close_engine(eng)
        return self.cache[name]


def fill_all(eng, byte):
    return sum(e.debug_fill_workspaces(byte) for e in engines_of(eng))


def check_dirty_workspace(base, name):
    """A smaller call after a larger one, and after every workspace has been set to 0x00, 0xFF and 0x5A."""
    case, want = BY_NAME[name], base(name)
    small, dirty = case.shapes("small", base.gpu), case.shapes("dirty", base.gpu)
    eng = nat.Engine(0, base.lib)
    try:
        case.run(eng, dirty)
        assert_same(case.run(eng, small), want, f"{name} after the dirtying shape")
        for byte in (0x00, 0xFF, 0x5A):
            filled = fill_all(eng, byte)
            assert filled > 0 or not case.workspace, f"{name}: lm_debug_fill_workspaces reached no workspace of this entry point"
            assert_same(case.run(eng, small), want, f"{name} after workspaces filled with {byte:#04x}")
    finally:
        close_engine(eng)


def check_call_order(base, which, seeds=(1, 2)):
    """Two fixed permutations of the cases on ONE engine; the small run of a case follows the dirtying run of the next one."""
    eng = nat.Engine(0, base.lib)
    try:
        for seed in seeds:
            order = [which[i] for i in np.random.default_rng(seed).permutation(len(which))]
            pending = None
            for name in order + [None]:
                if name is not None:
                    BY_NAME[name].run(eng, BY_NAME[name].shapes("dirty", base.gpu))
                if pending is not None:
                    assert_same(BY_NAME[pending].run(eng, BY_NAME[pending].shapes("small", base.gpu)), base(pending),
                                f"{pending} in permutation {seed} (order {order})")
                pending = name
    finally:
        close_engine(eng)


class Ballast:
    """Device work in front of a window that the host does not wait for, so that the device is BEHIND the host while the window's
    calls are made: lm_forward_dev on the exact-fp32 kernels (enqueue-only, see ENQUEUE_ONLY) on a few 256 x 256 slices of the model
    the cases use, already loaded and probed, with inputs and outputs nothing else touches.  On the emulator (synchronous streams,
    an emulated forward takes seconds) a small lm_edt_dev stands in: it keeps the harness's path the same."""

    def __init__(self, eng, gpu, slices=6, repeat=4, load_model=True, restore="split_f16"):
        self.eng, self.gpu, self.repeat, self.restore = eng, gpu, repeat, restore
        rng = np.random.default_rng(99)
        if gpu:
            self.slot = 0
            if load_model:
                Ctx(eng, None).model()
            self.x = eng.to_device(rng.random((slices, 256, 256), dtype=np.float32))
            self.out = eng.empty((slices, 256, 256), np.uint8)
        else:
            self.x = eng.to_device((rng.random((4, 16, 16)) < 0.05).astype(np.uint8))
            self.out = eng.empty((4, 16, 16), np.float32)
        self.push()  # (workspaces allocated here, not inside a window)
        eng.sync()

    def push(self):
        if not self.gpu:
            self.eng.edt_dev(self.x, SPACING, out=self.out)
            return
        self.eng.set_precision("f32")
        try:
            for _ in range(self.repeat):
                self.eng.forward_dev(self.slot, self.x, self.out, None)
        finally:
            self.eng.set_precision(self.restore)  # (split_f16: the models are already probed -- no forward, no wait)

    def close(self):
        self.x.free()
        self.out.free()


def check_deferred(base, which, seeds=(1, 2)):
    """Deferred by one.  ONE engine, the permutations of check_call_order, cyclic: behind a ballast the small shapes of case i are
    enqueued and NOT collected, then the dirtying shape of case i + 1 (a larger shape grows workspaces: hipFree / hipMalloc while
    case i may still be in flight); only then is case i collected and compared with the new engine's first call.  Every call has
    buffers of its own (AheadMem).  Prints, per permutation, the host time spent enqueuing and the time then spent inside the first
    collect(): the second is the work the device still had when the host was done -- where it is zero the host did not run ahead
    (a next case that reads something back waits inside its own call, and that wait is counted as enqueuing).  They are host
    timings on a shared machine: printed, never asserted."""
    eng = nat.Engine(0, base.lib)
    try:
        ahead = lambda e: AheadMem(e, uploader_of(e))
        bal = Ballast(eng, base.gpu)
        differ = []
        for seed in seeds:
            order = [which[i] for i in np.random.default_rng(seed).permutation(len(which))]
            # (the order is cyclic: every case, so every enqueue-only one, opens a window once per permutation)
            t_enqueue = t_collect = 0.0
            eo = [0.0, 0.0, 0.0]  # the windows opened by an enqueue-only case: ballast + case i enqueued, case i + 1 enqueued, first collect()
            eo_wait = {}          # the last of the three per window: case -> seconds
            for i, name in enumerate(order):
                case, after = BY_NAME[name], BY_NAME[order[(i + 1) % len(order)]]
                opened = []
                try:
                    t0 = time.perf_counter()
                    bal.push()
                    for shape in case.shapes("small", base.gpu):
                        opened.append(case.enqueue(eng, shape, ahead))
                    n_mine, tm = len(opened), time.perf_counter()
                    for shape in after.shapes("dirty", base.gpu):
                        opened.append(after.enqueue(eng, shape, ahead))
                    t1 = time.perf_counter()
                    got = [opened[0][0].collect()]
                    t2 = time.perf_counter()
                    got += [p.collect() for p, _ in opened[1:n_mine]]
                    t_enqueue, t_collect = t_enqueue + (t1 - t0), t_collect + (t2 - t1)
                    if name in ENQUEUE_ONLY:
                        eo = [eo[0] + (tm - t0), eo[1] + (t1 - tm), eo[2] + (t2 - t1)]
                        eo_wait[name] = t2 - t1
                    try:  # (every window is run: the list of ALL cases that differ says more than the first one)
                        assert_same(tuple(got), base(name), f"{name} collected after {after.name}'s dirtying shape was enqueued, permutation {seed}")
                    except AssertionError as exc:
                        differ.append(str(exc))
                    for p, _ in opened[n_mine:]:
                        p.collect()
                finally:
                    eng.sync()
                    for _, mem in opened:
                        mem.close()
            print(f"deferred by one, permutation {seed}: {len(order)} windows, host enqueued for {t_enqueue * 1e3:.1f} ms, "
                  f"then waited {t_collect * 1e3:.1f} ms in the first collect(); of that the {len(set(ENQUEUE_ONLY) & set(order))} windows opened by an "
                  f"enqueue-only case: {eo[0] * 1e3:.1f} ms for the ballast and the case (inputs made and copied in between), {eo[1] * 1e3:.1f} ms for the next "
                  f"case's dirtying shape (its own round trips included), {eo[2] * 1e3:.1f} ms in the first collect()")
            print(f"deferred by one, permutation {seed}: first collect() of each window opened by an enqueue-only case [ms]: "
                  + ", ".join(f"{n} {eo_wait[n] * 1e3:.1f}" for n in ENQUEUE_ONLY if n in eo_wait))
        bal.close()
        assert not differ, "; ".join(differ)
    finally:
        close_engine(eng)


def check_red_zones(base, name, k=0):
    """k == 0: guard bands round 256-byte aligned views at every small shape.  k > 0: bases that are element-aligned only, at the
    shape whose width alone selects the vector paths.  Guards intact, inputs unchanged, outputs those of the new engine."""
    case = BY_NAME[name]
    small = case.shapes("small", base.gpu)
    shapes = small if k == 0 else case.shapes("vec", base.gpu)
    want = tuple(base(name)[small.index(s)] for s in shapes)
    eng = nat.Engine(0, base.lib)
    try:
        got = case.run(eng, shapes, lambda e: ArenaMem(e, k, case.arena))
        assert_same(got, want, f"{name} in guarded views, base offset {k} elements")
    finally:
        close_engine(eng)


def check_repeatable(lib, name, runs=10):
    """Race screen: the same input `runs` times on one engine, identical bytes every time."""
    case = BY_NAME[name]
    eng = nat.Engine(0, lib)
    try:
        first = case.run(eng, case.stress)
        for it in range(1, runs):
            assert_same(case.run(eng, case.stress), first, f"{name}: run {it} of {runs}")
    finally:
        close_engine(eng)
