"""CPU suite: host-side logic of the mirrored operator interface (lungmask_amd/mask.py) that needs no device."""
import gc

import numpy as np
import pytest


def test_result_arrays_are_the_callers_alone(emu_engine):
    """mask.py:210 -- every apply() returns an array of its own.  LMInferer hands out root arrays over page-locked blocks of its pool
    (lm_host_alloc); a block goes back to the pool from a weakref.finalize on the root, i.e. only once the result AND every view /
    slice taken from it are gone -- no interpreter reference count is inspected (the getrefcount constant)."""
    from lungmask_amd.mask import LMInferer
    from oracle import unet_oracle as uo

    inf = LMInferer(state_dict=uo.synthetic_state_dict(3), engine=emu_engine)
    a = inf._result_array((3, 4, 5))
    a[:] = 7
    addr = a.ctypes.data
    view = a[1]
    del a
    gc.collect()
    b = inf._result_array((3, 4, 5))
    assert b.ctypes.data != addr and not np.shares_memory(b, view)  # a slice of the first result is still alive
    b[:] = 9
    assert (view == 7).all()
    del view
    gc.collect()
    c = inf._result_array((3, 4, 5))
    assert c.ctypes.data == addr            # everything dropped: the block is handed out again
    d = inf._result_array((2, 4, 5))        # another size never aliases
    assert not np.shares_memory(c, d) and not np.shares_memory(b, d)
    e, f = inf._result_array((3, 4, 5)), inf._result_array((3, 4, 5))
    assert len({x.ctypes.data for x in (b, c, e, f)}) == 4  # live results never share
    del b, c, d, e, f
    gc.collect()
    assert len(inf._pool.idle) <= 2  # two idle blocks kept at most, the others were freed


def test_force_cpu_is_an_error_without_the_opt_in(monkeypatch):
    """mask.py:118-134 selects a device; this engine has no CPU to select (checked before any engine is created)."""
    from lungmask_amd.mask import LMInferer

    monkeypatch.delenv("LUNGMASK_AMD_ALLOW_CPU_FLAG", raising=False)
    with pytest.raises(RuntimeError, match="MI355X-only"):
        LMInferer(force_cpu=True)
    with pytest.raises(AssertionError):
        LMInferer(modelname="no-such-model")  # mask.py:95-97


def test_a_kept_result_does_not_keep_the_engine_alive():
    """a result array used to reach the engine through its finalizer (result -> pool -> engine), so a caller who kept
    the masks of several `apply()` calls of the deprecated shims held one ~5 GB device workspace per mask.  The pool now holds the
    library and a weak reference: the engine goes away with the inferer, the kept result stays valid, and its page-locked block
    is freed through lm_host_free(NULL, p) when it is dropped."""
    import weakref

    from lungmask_amd import _native as nat
    from lungmask_amd.build import build_emu
    from lungmask_amd.mask import LMInferer
    from oracle import unet_oracle as uo

    eng = nat.Engine(0, nat.Library(build_emu(), allow_emulation=True))
    inf = LMInferer(state_dict=uo.synthetic_state_dict(3), engine=eng)
    res = inf._result_array((2, 8, 8))
    res[:] = 3
    eng_ref, pool = weakref.ref(eng), inf._pool
    del inf, eng
    gc.collect()
    assert eng_ref() is None, "the result array must not pin the engine"
    assert (res == 3).all()  # the block outlives the engine
    assert pool.closed  # LMInferer.__del__ closed the pool: the block will be freed, not parked, when the result goes
    del res
    gc.collect()
    assert pool.idle == []


def test_result_array_falls_back_to_pageable_memory(emu_engine, monkeypatch):
    """when page-locked memory runs out the idle blocks are released and `apply` gets an ordinary array
    (lm_apply_host accepts either) instead of raising."""
    from lungmask_amd import _native as nat
    from lungmask_amd.mask import LMInferer
    from oracle import unet_oracle as uo

    inf = LMInferer(state_dict=uo.synthetic_state_dict(3), engine=emu_engine)
    a = inf._result_array((2, 4, 4))
    del a
    gc.collect()
    assert len(inf._pool.idle) == 1

    def no_memory(n):
        raise nat.LMError("lm_host_alloc failed (-4): out of page-locked memory")

    monkeypatch.setattr(emu_engine, "host_alloc", no_memory)
    b = inf._result_array((3, 4, 4))  # another size: must allocate -> fails -> idle blocks freed -> pageable array
    assert b.shape == (3, 4, 4) and b.dtype == np.uint8 and inf._pool.idle == []
    inf.close()


class _FakePipeEngine:
    """Stands in for _native.Engine under `LMInferer.apply_async`'s two threads: records the lm_pipe_* calls, checks the caller's part
    of the protocol (include/lungmask_hip.h: an input buffer is only refilled after the hot path of the volume that used it has
    returned; a volume's hot path runs behind its own copy-in; downloads follow their hot path) and "labels" a volume with a
    function of its contents.  hold_copyback: a copy-back "arrives" only when the test sets `arrived[k]` (lm_pipe_query says no until
    then and lm_pipe_wait blocks)."""

    class _Lib:
        lm_pipe_upload = True  # (apply_async looks for the entry point)
        lm_pipe_query = True

    class _L:
        pass

    def __init__(self, fail_on=None, hold_copyback=False):
        import threading

        self.L = self._L()
        self.L.lib = self._Lib()
        self.lock = threading.Lock()
        self.log = []
        self.buf = [None, None]
        self.busy = [False, False]   # buffer k is between its upload and the return of its hot path
        self.out = [None, None]
        self.fail_on = fail_on
        self.n_apply = 0
        self.hold_copyback = hold_copyback
        self.arrived = [threading.Event(), threading.Event()]

    def host_alloc(self, n):
        raise RuntimeError("no page-locked memory in the fake")  # -> pageable result arrays

    def pipe_upload(self, k, vol):
        import time

        if vol is None:
            return
        with self.lock:
            assert not self.busy[k], "input buffer refilled while its volume is still on the hot path"
            self.busy[k] = True
            self.log.append(("upload", k))
        time.sleep(0.002)
        self.buf[k] = vol.copy()

    def pipe_apply(self, k, slot, shape, dtype, fill_slot=-1, batch_size=20, volume_postprocessing=True):
        import time

        with self.lock:
            assert self.busy[k] and self.buf[k] is not None and tuple(shape) == self.buf[k].shape, "hot path before its copy-in"
            self.log.append(("apply", k))
            self.n_apply += 1
            n = self.n_apply
        time.sleep(0.005)
        if self.fail_on == n:
            with self.lock:
                self.busy[k] = False
            raise RuntimeError("device error in volume %d" % n)
        self.out[k] = (self.buf[k] % 7).astype(np.uint8)
        with self.lock:
            self.busy[k] = False

    def pipe_download(self, k, out):
        with self.lock:
            self.log.append(("download", k))
        out[...] = self.out[k]
        if self.hold_copyback:
            self.arrived[k].clear()
        else:
            self.arrived[k].set()

    def pipe_wait(self, k):
        with self.lock:
            self.log.append(("wait", k))
        assert self.arrived[k].wait(timeout=30), "lm_pipe_wait on a copy-back that never arrives"

    def pipe_query(self, k):
        with self.lock:
            self.log.append(("query", k))
        return self.arrived[k].is_set()


def _fake_inferer(engine):
    from lungmask_amd.mask import LMInferer, _ResultPool

    inf = LMInferer.__new__(LMInferer)
    inf.engine, inf._engines, inf._shard, inf._async, inf._own_engine = engine, [engine], None, None, False
    inf.fill_slot, inf.batch_size, inf.volume_postprocessing, inf.fillmodel, inf.modelname = -1, 20, True, None, "R231"
    inf.reuse_output, inf._out = False, None
    inf._pool = _ResultPool.__new__(_ResultPool)
    import threading

    inf._pool.L, inf._pool._engine, inf._pool.lock, inf._pool.idle, inf._pool.closed = engine.L, (lambda: None), threading.Lock(), [], False
    return inf


def test_apply_async_keeps_two_volumes_in_flight_in_order():
    """`LMInferer.apply_async`: results in submission order and equal to what each volume alone gives; the uploader
    runs ahead of the hot path by at most one volume; the protocol of lm_pipe_* holds under the two host threads."""
    eng = _FakePipeEngine()
    inf = _fake_inferer(eng)
    rng = np.random.default_rng(4)
    vols = [rng.integers(-1000, 400, size=(3 + i % 2, 6, 5)).astype(np.int16) for i in range(7)]
    pend, got = [], []
    for v in vols:
        pend.append(inf.apply_async(v))
        if len(pend) > 1:
            got.append(pend.pop(0).result())
    while pend:
        got.append(pend.pop(0).result())
    for v, r in zip(vols, got):
        assert r.dtype == np.uint8 and np.array_equal(r, (v % 7).astype(np.uint8))
    ups = [i for i, (what, _) in enumerate(eng.log) if what == "upload"]
    aps = [i for i, (what, _) in enumerate(eng.log) if what == "apply"]
    assert len(ups) == len(aps) == 7 and all(u < a for u, a in zip(ups, aps))
    assert all(ups[i + 2] > aps[i] for i in range(5))                # buffer k refilled only after its volume left the hot path
    assert [k for what, k in eng.log if what == "apply"] == [i % 2 for i in range(7)]
    # other dtypes are widened like apply() does; an unsupported one raises from result()
    assert np.array_equal(inf.apply_async(vols[0].astype(np.uint8).astype(np.int8)).result(), (vols[0].astype(np.uint8).astype(np.int8).astype(np.int32) % 7).astype(np.uint8))
    with pytest.raises(TypeError):
        inf.apply_async(vols[0].astype(np.complex64)).result()
    inf._async.close()


def test_apply_async_propagates_a_failing_volume_and_carries_on():
    eng = _FakePipeEngine(fail_on=2)
    inf = _fake_inferer(eng)
    vols = [np.full((2, 4, 4), i, np.int16) for i in range(4)]
    hs = [inf.apply_async(v) for v in vols]
    assert np.array_equal(hs[0].result(), (vols[0] % 7).astype(np.uint8))
    with pytest.raises(RuntimeError, match="device error in volume 2"):
        hs[1].result()
    assert np.array_equal(hs[2].result(), (vols[2] % 7).astype(np.uint8)) and np.array_equal(hs[3].result(), (vols[3] % 7).astype(np.uint8))
    inf._async.flush()
    inf._async.close()


def test_apply_async_failing_volume_leaves_no_old_job_behind():
    """The queue's table holds the two volumes in flight and nothing older, also when a hot path raises: the failing path pops and
    finishes the volume two back like the other one does (it used to stay in the table, with its volume's handle, until close())."""
    eng = _FakePipeEngine(fail_on=4)
    inf = _fake_inferer(eng)
    vols = [np.full((2, 4, 4), i, np.int16) for i in range(7)]
    hs = []
    for i, v in enumerate(vols):
        hs.append(inf.apply_async(v))
        if i >= 2:
            hs[i - 2]._enqueued.wait(30)
    inf._async.flush()
    pipe = inf._async
    assert sorted(pipe.jobs) == [5, 6], sorted(pipe.jobs)
    for i, (v, h) in enumerate(zip(vols, hs)):
        if i == 3:
            with pytest.raises(RuntimeError, match="device error in volume 4"):
                h.result()
        else:
            assert np.array_equal(h.result(), (v % 7).astype(np.uint8))
    # volume 1 (two before the failing one) was finished by the failing path: its copy-back was waited for there
    assert hs[1].done() and hs[1]._wait is None
    # ... and a failure as the LAST volume leaves only itself and its predecessor
    eng.fail_on = eng.n_apply + 3
    more = [inf.apply_async(v) for v in vols[:3]]
    inf._async.flush()
    assert sorted(pipe.jobs) == [8, 9], sorted(pipe.jobs)
    with pytest.raises(RuntimeError):
        more[2].result()
    assert np.array_equal(more[0].result(), (vols[0] % 7).astype(np.uint8))
    inf._async.close()


def test_async_result_done_polls_the_copy_back_and_never_blocks():
    """`AsyncResult.done()` turns True for a volume whose copy-back has arrived with nobody calling result(), flush() or submitting
    another volume -- it asks the engine (lm_pipe_query) -- and it returns at once while the copy is still on its way."""
    eng = _FakePipeEngine(hold_copyback=True)
    inf = _fake_inferer(eng)
    vol = np.arange(2 * 4 * 4, dtype=np.int16).reshape(2, 4, 4)
    h = inf.apply_async(vol)
    assert h._enqueued.wait(30)
    assert h.done() is False and h.done() is False  # enqueued, not arrived: an answer, not a wait (lm_pipe_wait would block here)
    eng.arrived[0].set()
    assert h.done() is True
    assert ("wait", 0) not in eng.log and ("query", 0) in eng.log
    n_queries = eng.log.count(("query", 0))
    assert h.done() is True and eng.log.count(("query", 0)) == n_queries  # known to have arrived: the engine is not asked again
    assert np.array_equal(h.result(), (vol % 7).astype(np.uint8)) and ("wait", 0) not in eng.log
    # a handle that failed is done as well
    eng.fail_on = eng.n_apply + 1
    bad = inf.apply_async(vol)
    assert bad._enqueued.wait(30) and bad.done()
    with pytest.raises(RuntimeError):
        bad.result()
    for k in (0, 1):
        eng.arrived[k].set()
    inf._async.close()


def test_async_result_done_without_the_query_entry_point():
    """A library that lacks lm_pipe_query (the binding marks it optional): done() answers as it did before there was one -- False
    until somebody has waited for the copy-back, True afterwards -- instead of raising."""
    eng = _FakePipeEngine()
    del_lib = type("_Lib", (), {"lm_pipe_upload": True})
    eng.L.lib = del_lib()
    inf = _fake_inferer(eng)
    vol = np.full((2, 4, 4), 3, np.int16)
    h = inf.apply_async(vol)
    assert h._enqueued.wait(30)
    assert h.done() is False and not any(what == "query" for what, _ in eng.log)
    assert np.array_equal(h.result(), (vol % 7).astype(np.uint8)) and h.done() is True and h._src is None
    inf._async.close()


def test_apply_async_threads_do_not_keep_the_inferer_alive():
    """The queue's two host threads hold a weak reference to the inferer: an inferer that is dropped without close() is collected, and
    its finalizer ends the threads (they would otherwise pin it, and through it the engine, for the life of the process)."""
    import threading
    import time
    import weakref

    eng = _FakePipeEngine()
    inf = _fake_inferer(eng)
    assert np.array_equal(inf.apply_async(np.full((2, 4, 4), 5, np.int16)).result(), np.full((2, 4, 4), 5, np.uint8))
    pipe = inf._async
    threads = list(pipe.threads)
    assert all(t.is_alive() for t in threads)
    ref = weakref.ref(inf)
    del inf, pipe
    gc.collect()
    assert ref() is None, "the queue's threads must not pin the inferer"
    for t in threads:
        t.join(timeout=5)
    assert not any(t.is_alive() for t in threads)
