"""Drop-in for `lungmask/mask.py` (reference v0.2.20): same names, arguments and
error behaviour; everything below `LMInferer.apply` runs in liblungmask_hip.so
on an MI355X (one C-ABI call, volume device-resident).

Reference lines are cited per method.  PyTorch is used only to deserialise the
`.pth` state_dict (mask.py:48-54); there is no CPU compute path.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import sys
import threading
import warnings
import weakref
from typing import Optional, Union

import numpy as np

from . import _native
from .logger import logger

warnings.filterwarnings("ignore", category=UserWarning)  # mask.py:18

# mask.py:22-35
MODEL_URLS = {
    "R231": ("https://github.com/JoHof/lungmask/releases/download/v0.0/unet_r231-d5d2fc3d.pth", 3),
    "LTRCLobes": ("https://github.com/JoHof/lungmask/releases/download/v0.0/unet_ltrclobes-3a07043d.pth", 6),
    "R231CovidWeb": ("https://github.com/JoHof/lungmask/releases/download/v0.0/unet_r231covid-0de78a7e.pth", 3),
}


def get_model(modelname: str, modelpath: Optional[str] = None):
    """mask.py:38-68 -- returns the *state_dict* (the network itself lives in HBM).
    `modelpath` overrides `modelname`; `$LUNGMASK_WEIGHTS_DIR/<basename of the url>` is
    tried before the network download."""
    import torch

    if modelpath is None:
        model_url, _ = MODEL_URLS[modelname]
        local = os.path.join(os.environ.get("LUNGMASK_WEIGHTS_DIR", ""), os.path.basename(model_url))
        if os.environ.get("LUNGMASK_WEIGHTS_DIR") and os.path.exists(local):
            state_dict = torch.load(local, map_location=torch.device("cpu"))
        else:
            state_dict = torch.hub.load_state_dict_from_url(model_url, progress=True, map_location=torch.device("cpu"))
    else:
        state_dict = torch.load(modelpath, map_location=torch.device("cpu"))
    return state_dict


class _ResultPool:
    """Page-locked result blocks of one LMInferer: (address, bytes) pairs, idle ones kept for the next call.  A block is either in
    `idle` or owned by exactly one live root array (whose finalizer gives it back).  `close()` frees the idle blocks and marks the
    pool closed; blocks still owned by live arrays are freed by their finalizers.
    The pool keeps the LIBRARY alive, not the engine: a result array a caller holds on to must not pin the engine's ~5 GB of
    device workspace -- page-locked memory is freed through `lm_host_free(NULL, p)` once the engine is gone."""

    def __init__(self, engine):
        self.L = engine.L
        self._engine = weakref.ref(engine)
        self.lock = threading.Lock()
        self.idle = []
        self.closed = False
        # (at interpreter exit the blocks are left to the process teardown: the HIP runtime may already be gone)
        weakref.finalize(self, _ResultPool._free_all, self.L, self._engine, self.idle, self.lock).atexit = False

    @staticmethod
    def _host_free(L, engine_ref, addr):
        # Always with a NULL engine (allowed: include/lungmask_hip.h): this runs from finalizers, possibly on another thread, and an
        # engine handle read here could be destroyed by a concurrent Engine.close() before lm_host_free synchronises its stream
        # (ADVICE r05).  A page-locked block needs no stream sync to be freed: hipHostFree waits for the copies that use it.
        try:
            L.lib.lm_host_free(None, ctypes.c_void_p(addr))
        except Exception:
            pass

    @staticmethod
    def _free_all(L, engine_ref, idle, lock):
        with lock:
            blocks, idle[:] = list(idle), []
        for addr, _ in blocks:
            _ResultPool._host_free(L, engine_ref, addr)

    def alloc(self, n: int):
        """A page-locked block of n bytes, or None when the runtime has none left (after releasing the idle blocks)."""
        eng = self._engine()
        if eng is None or not getattr(eng, "h", None) or not hasattr(self.L.lib, "lm_host_alloc"):
            return None
        for attempt in range(2):
            try:
                return (eng.host_alloc(n), n)
            except _native.LMError:
                if attempt == 0:
                    _ResultPool._free_all(self.L, self._engine, self.idle, self.lock)  # idle blocks of other sizes
        return None

    def give_back(self, blk):  # runs from a finalizer, possibly on another thread / during interpreter shutdown
        with self.lock:
            if not self.closed and len(self.idle) < 2:
                self.idle.append(blk)
                return
        _ResultPool._host_free(self.L, self._engine, blk[0])

    def close(self):
        with self.lock:
            self.closed = True
        _ResultPool._free_all(self.L, self._engine, self.idle, self.lock)


class _ShardedApply:
    """`LMInferer.apply` over several MI355X: the volume's slices in contiguous blocks, one block per GPU.
    Two forms, both on `pipeline.ShardedPipeline`:
      * one process, N engines (`engines`, one per device) driven by N threads, exchanges as peer copies (`InProcessGroup`);
        every thread writes its block of the result straight into the caller's array;
      * one process per GPU (`dist`: torch.distributed or a `NativeDist`): this process owns one engine and one block; every
        rank calls `apply` with the same volume and gets the complete label volume, like the reference's single process."""

    def __init__(self, engines, fill_slot, batch_size, volume_postprocessing, dist=None, sharded_post=None, resolution=(256, 256)):
        from concurrent.futures import ThreadPoolExecutor

        from .pipeline import InProcessGroup, ShardedPipeline

        def dev(e):
            return f"cuda:{e.device_id}" if e.L.is_gpu else "cpu"

        self.engines = list(engines)
        self.dist = dist
        self.group = None
        kw = dict(slot=0, batch_size=batch_size, volume_postprocessing=volume_postprocessing, fill_slot=fill_slot, sharded_post=sharded_post,
                  resolution=resolution)
        if dist is not None:
            assert len(self.engines) == 1
            self.pipes = [ShardedPipeline(self.engines[0], dist=dist, device=dev(self.engines[0]), **kw)]
            self.pool = None
        else:
            self.group = InProcessGroup(len(self.engines))
            self.pipes = [ShardedPipeline(e, dist=self.group.member(r, e), device=dev(e), **kw) for r, e in enumerate(self.engines)]
            self.pool = ThreadPoolExecutor(max_workers=len(self.engines), thread_name_prefix="lungmask_amd-rank")

    @property
    def world(self):
        return self.pipes[0].world

    def apply(self, vol: np.ndarray, out: np.ndarray) -> np.ndarray:
        from .pipeline import shard_bounds

        n = int(vol.shape[0])
        if self.dist is not None:
            p = self.pipes[0]
            b = shard_bounds(n, p.world)
            return p.apply_local(vol[b[p.rank] : b[p.rank + 1]], n, gather=True, out=out)
        b = shard_bounds(n, len(self.pipes))

        def run(r):
            try:
                self.pipes[r].apply_local(vol[b[r] : b[r + 1]], n, gather=False, out=out[b[r] : b[r + 1]])
            except BaseException:
                self.group.abort()  # the other ranks raise BrokenBarrierError instead of waiting for this one
                raise

        futs = [self.pool.submit(run, r) for r in range(len(self.pipes))]
        errs = [f.exception() for f in futs]  # (waits for every rank)
        if any(e is not None for e in errs):
            self.group.reset()
            real = [e for e in errs if e is not None and not isinstance(e, threading.BrokenBarrierError)]
            raise (real or [e for e in errs if e is not None])[0]
        return out

    def close(self):
        if self.pool is not None:
            self.pool.shutdown(wait=True)
            self.pool = None
        self.pipes = []


class AsyncResult:
    """What `LMInferer.apply_async` returns: `result()` blocks until the volume's labels have arrived and returns the uint8 array
    (or raises what the call raised); `done()` does not block: it asks the engine whether the copy-back has arrived
    (lm_pipe_query) and needs nobody else to wait for it."""

    def __init__(self):
        self._enqueued = threading.Event()  # the hot path has run and the copy-back is enqueued (or the call failed)
        self._lock = threading.Lock()
        self._res = None
        self._exc = None
        self._wait = None  # waits for the copy-back; None once it is known to have arrived
        self._poll = None  # asks, without blocking, whether the copy-back has arrived (valid while _wait is set; None: the library has no lm_pipe_query)
        self._src = None  # the input volume until the copy-back has arrived: a page-locked source is read by the copy-in itself, after the calls have returned
        self._keep = None  # the inferer, while the volume is queued (the queue's threads only hold a weak reference to it)

    def _finish(self):
        with self._lock:
            w = self._wait
        if w is not None:
            w()  # (done() keeps saying what the engine says until the wait is over)
            with self._lock:
                self._wait = self._poll = self._src = None

    def done(self) -> bool:
        if not self._enqueued.is_set():
            return False
        with self._lock:
            if self._wait is None:
                return True
            # (While _wait is set no later volume has been handed this result buffer: the runner finishes this handle before it
            # enqueues that volume's copy-back, so the query is about THIS volume's copy.)
            if self._poll is None or not self._poll():
                return False
            self._wait = self._poll = self._src = None
        return True

    def result(self) -> np.ndarray:
        self._enqueued.wait()
        if self._exc is not None:
            raise self._exc
        self._finish()
        return self._res


class _AsyncPipe:
    """Volumes queued through ONE engine (include/lungmask_hip.h: lm_pipe_*): an uploader thread copies volume i + 1 into the
    engine's other input buffer while the runner thread has volume i on the hot path; the copy-back of volume i runs on a third
    stream beside volume i + 1.  Two volumes in flight, results in submission order."""

    def __init__(self, inferer):
        import queue

        # The two threads must not keep the inferer alive (they are GC roots for as long as they run): they hold a weak reference, a
        # queued volume's handle holds the strong one until its result is enqueued, and a finalizer on the inferer ends the threads
        # when it goes away without close().
        self.inf_ref = weakref.ref(inferer)
        self.eng = inferer.engine
        self.eng.pipe_upload(0, None)  # streams and events exist before the two threads touch them
        self.jobs = {}
        self.seq = 0
        self.up_q, self.run_q = queue.Queue(), queue.Queue()
        self.idle = threading.Condition()
        self.pending = 0
        self.timing = os.environ.get("LM_ASYNC_TIMING") == "1"  # per-volume breakdown of the two threads on stderr
        self.threads = [threading.Thread(target=self._uploader, name="lungmask_amd-upload", daemon=True),
                        threading.Thread(target=self._runner, name="lungmask_amd-run", daemon=True)]
        for t in self.threads:
            t.start()
        weakref.finalize(inferer, _AsyncPipe._stop_threads, self.up_q, self.run_q).atexit = False

    @staticmethod
    def _stop_threads(up_q, run_q):
        up_q.put(None)
        run_q.put(None)

    def submit(self, vol: np.ndarray) -> AsyncResult:
        h = AsyncResult()
        h._keep = self.inf_ref()
        job = dict(seq=self.seq, k=self.seq % 2, vol=vol, handle=h, uploaded=threading.Event(), computed=threading.Event(), error=None)
        self.seq += 1
        with self.idle:
            self.pending += 1
        self.jobs[job["seq"]] = job
        self.up_q.put(job)
        self.run_q.put(job)
        return h

    def _uploader(self):
        import time

        while True:
            job = self.up_q.get()
            if job is None:
                return
            try:
                prev = self.jobs.get(job["seq"] - 2)
                if prev is not None:
                    prev["computed"].wait()  # the hot path of the volume that used this input buffer has returned
                t0 = time.perf_counter()
                self.eng.pipe_upload(job["k"], job["vol"])
                if self.timing:
                    sys.stderr.write("apply_async: volume %d copy-in call %.2f ms\n" % (job["seq"], (time.perf_counter() - t0) * 1e3))
            except BaseException as exc:  # noqa: BLE001
                job["error"] = exc
            job["uploaded"].set()

    def _runner(self):
        import time

        eng = self.eng
        t_prev = time.perf_counter()
        while True:
            job = self.run_q.get()
            if job is None:
                return
            h = job["handle"]
            inf = h._keep
            try:
                t0 = time.perf_counter()
                job["uploaded"].wait()
                if job["error"] is not None:
                    raise job["error"]
                vol = job["vol"]
                t1 = time.perf_counter()
                res = inf._result_array(vol.shape)
                t2 = time.perf_counter()
                eng.pipe_apply(job["k"], 0, vol.shape, vol.dtype, fill_slot=inf.fill_slot, batch_size=inf.batch_size,
                               volume_postprocessing=inf.volume_postprocessing)
                t3 = time.perf_counter()
                job["computed"].set()
                prev = self.jobs.pop(job["seq"] - 2, None)
                if prev is not None:
                    prev["handle"]._finish()  # (its copy-back is long done: this volume's hot path waited for it on the device)
                eng.pipe_download(job["k"], res)
                if self.timing:
                    sys.stderr.write("apply_async: volume %d waited for its copy-in %.2f ms, result array %.2f, hot path %.2f, hand-over %.2f (idle before: %.2f)\n" % (
                        job["seq"], (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (time.perf_counter() - t3) * 1e3, (t0 - t_prev) * 1e3))
                t_prev = time.perf_counter()
                h._res = res
                k = job["k"]
                h._src = vol
                # (an older library without lm_pipe_query: done() answers as before -- True once somebody has waited)
                h._poll = (lambda: eng.pipe_query(k)) if hasattr(eng.L.lib, "lm_pipe_query") else None
                h._wait = lambda: eng.pipe_wait(k)
            except BaseException as exc:  # noqa: BLE001
                h._exc = exc
                job["computed"].set()
                # the volume two back leaves the table here as on the other path (its copy-back is the last one on this result buffer)
                prev = self.jobs.pop(job["seq"] - 2, None)
                if prev is not None and prev["handle"]._exc is None:
                    try:
                        prev["handle"]._finish()
                    except BaseException as late:  # noqa: BLE001
                        prev["handle"]._exc = late
            job["vol"] = None
            h._keep = inf = None
            h._enqueued.set()
            with self.idle:
                self.pending -= 1
                self.idle.notify_all()

    def flush(self):
        """Returns when every submitted volume has left the hot path and its copy-back has arrived."""
        with self.idle:
            self.idle.wait_for(lambda: self.pending == 0)
        for job in list(self.jobs.values()):
            if job["handle"]._exc is None:
                job["handle"]._finish()

    def close(self):
        self.flush()
        self.up_q.put(None)
        self.run_q.put(None)
        for t in self.threads:
            t.join(timeout=10)
        self.jobs.clear()


class _DeviceLabels(_native.DeviceScope):
    """What `LMInferer._device_labels` yields: a scope of device arrays with `raw` (the device volume, None once it was freed
    early), `back` (the device labels in the caller's orientation) and `labels` (the host result array)."""

    raw = back = labels = None
    fetched = False

    def fetch(self) -> np.ndarray:
        """`labels`, filled from the device now if it is not yet."""
        if not self.fetched:
            self.back.download_into(self.labels)
            self.fetched = True
        return self.labels


class LMInferer:
    """mask.py:71-232."""

    def __init__(
        self,
        modelname: str = "R231",
        modelpath: Optional[str] = None,
        fillmodel: Optional[str] = None,
        fillmodel_path: Optional[str] = None,
        force_cpu: bool = False,
        batch_size: int = 20,
        volume_postprocessing: bool = True,
        tqdm_disable: bool = False,
        device_id: int = 0,
        precision: str = "split_f16",
        reuse_output: bool = False,
        state_dict=None,
        fill_state_dict=None,
        engine=None,
        device_ids=None,
        dist=None,
        engines=None,
        sharded_post=None,
        resolution=(256, 256),
    ):
        assert modelname in MODEL_URLS, "Modelname not found. Please choose from: {}".format(MODEL_URLS.keys())  # mask.py:95-97
        if fillmodel is not None:
            assert fillmodel in MODEL_URLS, "Modelname not found. Please choose from: {}".format(MODEL_URLS.keys())
        if modelpath is not None:  # mask.py:104-107
            modelname = os.path.basename(modelpath)
        if fillmodel_path is not None:
            fillmodel = os.path.basename(fillmodel_path)
        self.fillmodel = fillmodel
        self.modelname = modelname
        self.force_cpu = force_cpu
        self.batch_size = batch_size
        self.volume_postprocessing = volume_postprocessing
        self.tqdm_disable = tqdm_disable
        # reuse_output=True: apply() returns the SAME uint8 array on every call with an unchanged volume shape (the caller must
        # consume or copy a result before the next call).  The reference returns a fresh array per call (mask.py:210) and that
        # stays the default; a fresh 79 MB array per 300-slice volume costs ~3-4 ms of page faults and unmapping.
        self.reuse_output = reuse_output
        self._out = None
        self._async = None  # apply_async's pipeline (two host threads), created on first use
        self._pool = None  # page-locked result blocks (see _result_array); created with the engine below
        if force_cpu:
            # mask.py:118-134 selects torch-CPU.  This engine has no CPU compute path by design, so by default the request is an
            # ERROR -- a caller who asks for the CPU (no usable GPU, reproducing a CPU result) must not silently get GPU execution.
            # LUNGMASK_AMD_ALLOW_CPU_FLAG=1 opts in to "accept the flag, warn, run on the MI355X": what code written against the
            # reference needs when it passes force_cpu=True as a matter of course (the reference's own tests do,
            # tests/test_mask.py:32,43,53; the reference-derived tests here set the variable).
            # (LUNGMASK_AMD_STRICT_CPU=0, the name of this switch before round 3, is still honoured)
            if os.environ.get("LUNGMASK_AMD_ALLOW_CPU_FLAG") != "1" and os.environ.get("LUNGMASK_AMD_STRICT_CPU") != "0":
                raise RuntimeError(
                    "lungmask_amd is an MI355X-only engine: force_cpu=True / --cpu is not available (use the reference package for CPU, "
                    "or set LUNGMASK_AMD_ALLOW_CPU_FLAG=1 to accept the flag and run on the GPU)")
            logger.warning("force_cpu requested and LUNGMASK_AMD_ALLOW_CPU_FLAG=1: lungmask_amd has no CPU path, running on the MI355X")
        # Extensions (not in the reference): `state_dict` / `fill_state_dict` = weights that are already in memory (what the
        # deprecated `apply(image, model)` shim and bench.py pass) instead of a file or download; `engine` = an existing
        # _native.Engine to load them into instead of a new one (one engine owns ~5 GB of workspace).
        # Multi-GPU (not in the reference, which runs on one device): `device_ids=[0, 1, ...]` -- one engine per
        # listed device inside THIS process, the volume's slices spread over them (`engines=[...]`: the same with existing engines);
        # `dist=` -- one process per GPU: the initialised torch.distributed module or a `pipeline.NativeDist`, this process being
        # one rank with its own `device_id`.  Either way `apply` keeps its contract: the complete label volume comes back.
        self._own_engine = engine is None and engines is None
        if engines is not None:
            engs = list(engines)
        elif device_ids is not None and len(device_ids) > 0:
            assert dist is None, "device_ids (one process, several GPUs) and dist (one process per GPU) are alternatives"
            engs = [_native.Engine(int(d)) for d in device_ids]
        else:
            engs = [engine if engine is not None else _native.Engine(device_id)]
        self.engine = engs[0]
        self._engines = engs
        self._pool = _ResultPool(self.engine)
        sd = state_dict if state_dict is not None else get_model(self.modelname, modelpath)
        fsd = None
        if self.fillmodel is not None:  # mask.py:136-139
            fsd = fill_state_dict if fill_state_dict is not None else get_model(self.fillmodel, fillmodel_path)
        self.fill_slot = 1 if fsd is not None else -1
        for eng in engs:  # weights replicated: 110 MiB per model and GPU
            eng.set_precision(precision)  # "split_f16" (default, fp32-class) or "f32" (exact fp32 matrix ops)
            eng.load_state_dict(0, sd)
            if fsd is not None:
                eng.load_state_dict(1, fsd)
        self._shard = None
        if len(engs) > 1 or dist is not None:
            self._shard = _ShardedApply(engs, self.fill_slot, batch_size, volume_postprocessing, dist=dist, sharded_post=sharded_post, resolution=resolution)
        # mask.py:166 hard-codes the network resolution [256, 256]; only the multi-GPU form (built from the stage-level calls) can run
        # another one -- what the CPU test-suite's emulated kernels need -- and nothing else may ask for it
        assert tuple(resolution) == (256, 256) or self._shard is not None, "resolution is fixed at 256 x 256 (mask.py:166)"

    def _result_array(self, shape, dtype=np.uint8) -> np.ndarray:
        """A uint8 result array that is the caller's alone -- the reference's contract (mask.py:210) -- without paying for fresh
        memory on every call (a new 79 MB numpy array costs ~4.7 ms of page faults and unmapping per 300-slice volume) and in
        page-locked memory (`lm_host_alloc`), which the device writes at link speed.
        Ownership is explicit: every array handed out is a NEW root ndarray over a block of this object's pool, and the block goes
        back to the pool from a `weakref.finalize` on that root -- numpy points every view, slice and reshape a caller takes at the
        root, so the finalizer runs exactly when the result and everything derived from it are gone.  No interpreter reference
        count is inspected (round 3 compared `sys.getrefcount` with a CPython-version-specific constant).  While a caller keeps
        earlier results, further blocks are allocated; at most two idle blocks are retained.  A consumer that keeps only a raw
        address (ctypes, a C extension) must keep the array alive as with any numpy array -- or pass its own `out=`."""
        dtype = np.dtype(dtype)
        n = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        pool = self._pool
        with pool.lock:
            blk = next((b for b in pool.idle if b[1] == n), None)
            if blk is not None:
                pool.idle.remove(blk)
        if blk is None and n:
            blk = pool.alloc(n)
        if blk is None:  # empty volume, an older library, or no page-locked memory left: an ordinary array (lm_apply_host takes either)
            return np.empty(shape, dtype=dtype)
        root = np.ndarray(shape, dtype=dtype, buffer=(ctypes.c_uint8 * n).from_address(blk[0]))
        weakref.finalize(root, _ResultPool.give_back, pool, blk).atexit = False
        return root

    def close(self):
        """Releases the idle result blocks and the engine(s) this object created.  Results already handed out stay valid (their
        blocks are freed when they are dropped)."""
        if getattr(self, "_async", None) is not None:
            self._async.close()
            self._async = None
        if getattr(self, "_pool", None) is not None:
            self._pool.close()
        sh = getattr(self, "_shard", None)
        if sh is not None:
            sh.close()
            self._shard = None
        if getattr(self, "_own_engine", False):
            for eng in getattr(self, "_engines", []):
                eng.close()
        self._own_engine = False

    def __del__(self):
        try:
            if getattr(self, "_pool", None) is not None:
                self._pool.close()
            sh = getattr(self, "_shard", None)
            if sh is not None:
                sh.close()
        except Exception:
            pass

    def apply_async(self, image) -> AsyncResult:
        """`apply` for a STREAM of volumes (extension; SURVEY.md section 8f #4, "multi-volume queueing"): returns at once with a handle
        whose `result()` is what `apply(image)` would have returned.  Volumes go through the engine in submission order, two in
        flight: the copy-in of the next volume and the copy-back of the previous one run beside the hot path of the current one
        (lm_pipe_*), so a caller that keeps the queue fed sees the device-resident rate.  `image` must stay unchanged until
        `result()` returns.  Inputs that need more than the one call (a re-orientation to LPS, several GPUs, an empty volume) are
        computed by `apply` itself, in order."""
        done = AsyncResult()
        eligible = isinstance(image, np.ndarray) and image.ndim == 3 and image.shape[0] > 0 and self._shard is None and hasattr(self.engine.L.lib, "lm_pipe_upload")
        if eligible:
            try:
                vol = np.ascontiguousarray(self._engine_dtype(image))
            except TypeError as exc:
                done._exc = exc
                done._enqueued.set()
                return done
            if self._async is None:
                self._async = _AsyncPipe(self)
            return self._async.submit(vol)
        try:
            done._res = self.apply(image)  # (waits for the queued volumes first)
        except BaseException as exc:  # noqa: BLE001
            done._exc = exc
        done._enqueued.set()
        return done

    @staticmethod
    def _engine_dtype(inimg_raw: np.ndarray) -> np.ndarray:
        """The dtypes the engine pre-processes on the device; everything else value-preserving widened (numpy mode of mask.py:153-155)."""
        if inimg_raw.dtype not in (np.int16, np.int32, np.int64, np.float32, np.float64):
            if inimg_raw.dtype.kind in "ib" or inimg_raw.dtype.kind == "u" and inimg_raw.dtype.itemsize < 8:
                # value preserving; np.clip(-1024, 600) then behaves as for a wider signed type
                return inimg_raw.astype(np.int32 if inimg_raw.dtype.itemsize < 4 else np.int64)
            if inimg_raw.dtype == np.float16:
                return inimg_raw.astype(np.float32)  # value preserving
            raise TypeError(f"lungmask_amd: unsupported volume dtype {inimg_raw.dtype}")
        return inimg_raw

    @staticmethod
    def _orientation(image):
        """(axes, flips), the index transform that brings `image` to LPS (mask.py:156-164): the identity for a numpy array and for an
        image whose direction matrix is LPS already.  The only place that looks at a direction matrix."""
        if not isinstance(image, np.ndarray):
            from . import volume_io

            direction = image.direction if isinstance(image, volume_io.Volume) else image.GetDirection()
            if volume_io.orientation_code(direction) != "LPS":
                return volume_io.lps_transform(direction)
        return (0, 1, 2), (False, False, False)

    @staticmethod
    def _array_of(image) -> np.ndarray:
        if isinstance(image, np.ndarray):
            return image
        from . import stats as st

        return st.geometry(image)[0]

    def _volume_input(self, who: str, image, spacing=None):
        """The input step of the apply_* extensions: `image` (numpy [n,h,w] with its optional `spacing`, a `volume_io.Volume` or a
        SimpleITK image) -> (array, spacing in array axis order or None, index_to_physical or None, (axes, flips), the array
        C-contiguous in a dtype of the engine)."""
        from . import stats as st

        arr, sp, to_phys = st.geometry(image, spacing)
        arr = np.asarray(arr)
        if arr.ndim != 3:
            raise ValueError(f"{who}: a 3-D volume is needed, got shape {arr.shape}")
        return arr, sp, to_phys, self._orientation(image), np.ascontiguousarray(self._engine_dtype(arr))

    def _on_host(self, arr) -> bool:
        """The host detour of the apply_* extensions: several engines (the labels come gathered from `apply`) or no slice."""
        return self._shard is not None or arr.shape[0] == 0

    def _model_labels(self, names=None):
        """(n_labels, {label: name}) of the loaded model for the per-label analyses."""
        from . import stats as st

        n_labels = max(1, min(self.engine.n_classes(0), st.MAX_LABELS))
        return n_labels, names if names is not None else st.label_names(self.modelname, n_labels)

    @contextlib.contextmanager
    def _device_labels(self, vol: np.ndarray, orientation, free_input: bool = False):
        """The one device-resident labelling under `apply` and its extensions on one GPU.  Waits for the queued volumes, takes a
        result array from the pool, uploads `vol` (C-contiguous, an engine dtype, the caller's orientation) and labels it with
        `_labels_dev`; `free_input` frees the device volume as soon as it is in LPS (a lower peak for callers that need the labels
        only).  Yields the `_DeviceLabels` scope; the body registers what it allocates with `add`.  On exit `labels` is filled if
        it is not yet, and everything is freed, on every path."""
        if self._async is not None:
            self._async.flush()  # one engine, one hot path at a time: the queued volumes first
        with _DeviceLabels(self.engine) as lb:
            lb.labels = self._result_array(vol.shape)
            raw = lb.upload(vol)
            lb.back = lb.add(self._labels_dev(raw, *orientation, free_input=free_input))
            lb.raw = None if free_input else raw
            yield lb
            lb.fetch()

    def apply(self, image, out: Optional[np.ndarray] = None) -> np.ndarray:
        """mask.py:212-232 (+ _inference :141-210).  `image`: numpy volume [n,h,w], a `volume_io.Volume`, or a SimpleITK
        image.  Images with a direction matrix are brought to LPS and back (mask.py:156-164, 204-208) by an index
        transform on the device (`lm_reorient_dev`) instead of `sitk.DICOMOrient`.
        `out` (extension): a caller-owned C-contiguous uint8 array of the volume's shape that receives the labels."""
        axes, flips = self._orientation(image)
        inimg_raw = self._engine_dtype(self._array_of(image))
        if self._async is not None:
            self._async.flush()  # one engine, one hot path at a time: the queued volumes first
        if self.fillmodel is not None:
            logger.info(f"Apply: {self.modelname}")
            logger.info(f"Apply: {self.fillmodel}")
            logger.info("Fusing results... this may take up to several minutes!")
        if self._shard is not None and inimg_raw.ndim == 3 and inimg_raw.shape[0] > 0:
            # slices spread over the GPUs.  The LPS re-orientation (mask.py:156-164, 204-208) is an index permutation: on the host
            # here, because after it the slice axis may be another one than the axis the caller's array is split along.
            direct = axes == (0, 1, 2) and not any(flips)
            if direct:
                vol = np.ascontiguousarray(inimg_raw)
            else:
                from . import volume_io

                vol = np.ascontiguousarray(volume_io.apply_transform(inimg_raw, axes, flips))
            res = out if (direct and out is not None) else self._result_array(vol.shape)
            if res.dtype != np.uint8 or tuple(res.shape) != tuple(vol.shape) or not res.flags.c_contiguous:
                raise _native.LMError("apply(out=...): need a C-contiguous uint8 array of the volume's shape")
            res = self._shard.apply(vol, res)
            if direct:
                return res
            back = volume_io.apply_transform(res, *volume_io.inverse_transform(axes, flips))
            if out is not None:
                out[...] = back
                return out
            return np.ascontiguousarray(back)
        if axes == (0, 1, 2) and not any(flips):
            own = out is None  # an array of this object's: its old contents are nobody's (lm_apply_host_ex, LM_APPLY_OUT_SCRATCH)
            if out is None and self.reuse_output:
                if self._out is None or self._out.shape != tuple(inimg_raw.shape):
                    self._out = np.empty(inimg_raw.shape, dtype=np.uint8)
                out = self._out
            elif out is None and inimg_raw.ndim == 3:
                out = self._result_array(inimg_raw.shape)
            # (the labels land in `out` / the result array straight from the device: no further host copy)
            return self.engine.apply(0, inimg_raw, fill_slot=self.fill_slot, batch_size=self.batch_size,
                                     volume_postprocessing=self.volume_postprocessing, out=out, out_scratch=own)
        with self._device_labels(np.ascontiguousarray(inimg_raw), (axes, flips), free_input=True) as lb:
            pass  # (the labels alone: brought to LPS, labelled and brought back on the device)
        if out is not None:
            out[...] = lb.labels
            return out
        return lb.labels

    def _labels_dev(self, raw, axes, flips, free_input: bool = False):
        """The labels of the device-resident volume `raw` (the caller's orientation; `axes` / `flips`: its transform to LPS) as a
        new device array in that same orientation -- what the single-GPU `apply` computes for an image that is not LPS, and, for an
        LPS one, lm_apply_dev with the fill model.  `free_input`: `raw` is freed as soon as it has been brought to LPS."""
        from . import volume_io

        eng = self.engine
        if axes == (0, 1, 2) and not any(flips):
            back = eng.empty(raw.shape, np.uint8)
            eng.apply_dev(0, raw, back, fill_slot=self.fill_slot, batch_size=self.batch_size, volume_postprocessing=self.volume_postprocessing)
            if free_input:
                raw.free()
            return back
        lps = eng.reorient_dev(raw, axes, flips)
        if free_input:
            raw.free()
        inv = volume_io.inverse_transform(axes, flips)
        out_lps = eng.empty(lps.shape, np.uint8)
        if self.fill_slot < 0:
            eng.apply_dev(0, lps, out_lps, fill_slot=-1, batch_size=self.batch_size, volume_postprocessing=self.volume_postprocessing)
            back = eng.reorient_dev(out_lps, *inv)
        else:
            # The reference orients EACH model's result back inside _inference (mask.py:204-208) and then fuses and post-processes
            # in the image's ORIGINAL orientation (mask.py:228-232): the 3-D post-processing is equivariant under axis
            # permutations and flips except where raster order decides (region numbering behind the merge order and its ties,
            # equal-area components) and in its single-slice branch (utils.py:344) -- so it must see the original axes.
            eng.apply_dev(0, lps, out_lps, fill_slot=-1, batch_size=self.batch_size, volume_postprocessing=self.volume_postprocessing)
            back = eng.reorient_dev(out_lps, *inv)                                     # res_l (mask.py:222)
            eng.apply_dev(self.fill_slot, lps, out_lps, fill_slot=-1, batch_size=self.batch_size, volume_postprocessing=self.volume_postprocessing)
            res_r = eng.reorient_dev(out_lps, *inv)                                    # res_r (mask.py:227)
            spare = ctypes.c_int()
            eng.L.check(eng.L.lib.lm_fuse_dev(eng.h, back.ptr, res_r.ptr, back.nbytes, ctypes.byref(spare)), "lm_fuse_dev")  # mask.py:228-230
            eng.postprocess_dev(back, spare=[spare.value])                             # mask.py:232
            res_r.free()
        for d in (lps, out_lps):
            d.free()
        return back


    def apply_probabilities(self, image, dtype=np.float32):
        """Labels AND per-class probability maps at the geometry of the input (extension; the reference returns labels only):
        -> (labels, probs).  `image`: what `apply` takes (numpy [n,h,w], a `volume_io.Volume`, a SimpleITK image); `dtype`: float32
        or float16 (half the bytes; equal to the float32 maps' `.astype(np.float16)` bit for bit).

        `labels` is exactly what `apply(image)` returns, post-processing included.  `probs` is class-major [C][n][h][w]: `probs[c]`
        is a volume shaped like the input.  They are the RAW network probabilities resampled back into each slice's body box -- the
        recipe of reshape_mask (utils.py:114-129) with linear instead of nearest-neighbour interpolation: for slice z, class c and
        the slice's box (r0, c0, r1, c1) from the pre-processing (utils.py:102-106),
            p = exp(logp[z, c])  (the network's log-softmax, [256, 256] float32)
            probs[c, z, r0:r1, c0:c1] = scipy.ndimage.zoom(p, ((r1-r0)/256, (c1-c0)/256), order=1)   (fp64 inside, float32 result)
            probs[c, z, elsewhere] = 1.0 if c == 0 else 0.0   (reshape_mask's zero fill = label 0 = background)
        and the fill, too, where ndimage.zoom's coordinate rounds beyond the last source row / column (scipy's cval 0 in every class).
        The maps sum to one everywhere (linear interpolation is a convex combination).  Volume post-processing changes labels only,
        never probabilities: `probs.argmax(0)` may differ from `labels` where post-processing removed or filled a region, and where
        nearest-neighbour and linear resampling disagree.
        One forward pass gives both: each batch's log-softmax is un-cropped on the device right behind the batch.  Not available in
        the fused mode (`fillmodel`: the reference defines no probabilities of a fused result) nor in the multi-GPU forms."""
        dt = np.dtype(dtype)
        if dt not in _native.LM_PROB_DTYPES:
            raise TypeError(f"apply_probabilities: dtype float32 or float16, not {dt}")
        if self.fill_slot >= 0:
            raise ValueError("apply_probabilities: the fused mode (fillmodel) has no probability maps -- the reference fuses labels only "
                             "(mask.py:223-232); use one LMInferer per model for each model's probabilities")
        if self._shard is not None:
            raise NotImplementedError("apply_probabilities runs on one GPU: use an LMInferer with a single device_id (no device_ids, dist "
                                      "or several engines) for the probability maps; apply() still spreads labels over the GPUs")
        axes, flips = self._orientation(image)
        inimg_raw = self._array_of(image)
        inimg_raw = np.ascontiguousarray(self._engine_dtype(inimg_raw))
        if self._async is not None:
            self._async.flush()  # one engine, one hot path at a time: the queued volumes first
        eng = self.engine
        ncls = eng.n_classes(0)
        shape = tuple(inimg_raw.shape)
        # Both results come back into page-locked blocks of the result pool (_result_array): the maps are the big transfer --
        # C x the volume's voxels x 4 bytes, 0.9 GB for R231 and 1.9 GB for LTRCLobes at 300 x 512^2 -- and the device writes
        # page-locked memory at link speed.
        labels = self._result_array(shape)
        probs = self._result_array((ncls,) + shape, dt)
        if axes == (0, 1, 2) and not any(flips):
            return eng.apply_probs(0, inimg_raw, batch_size=self.batch_size, volume_postprocessing=self.volume_postprocessing, dtype=dt,
                                   labels_out=labels, probs_out=probs)
        from . import volume_io

        # mask.py:156-164 / 204-208: to LPS on the device, labels and every class map back with the inverse index transform
        inv = volume_io.inverse_transform(axes, flips)
        with eng.scope() as dev:
            raw = dev.upload(inimg_raw)
            lps = dev.add(eng.reorient_dev(raw, axes, flips))
            raw.free()
            lab_lps = dev.empty(lps.shape, np.uint8)
            p_lps = dev.empty((ncls,) + lps.shape, dt)
            p_back = dev.empty((ncls,) + shape, dt)
            eng.apply_probs_dev(0, lps, p_lps, lab_lps, batch_size=self.batch_size, volume_postprocessing=self.volume_postprocessing)
            back = dev.add(eng.reorient_dev(lab_lps, *inv))
            per = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
            for c in range(ncls):  # (element size 4 or 2)
                eng.reorient_dev(p_lps.view(c * per, lps.shape), *inv, out=p_back.view(c * per, shape))
            back.download_into(labels)
            p_back.download_into(probs)
        return labels, probs

    def apply_with_stats(self, image, spacing=None, percentiles=(15,), thresholds=(-950,), names=None):
        """`apply(image)` plus the volume and density statistics of its labels (extension; lungmask_amd.stats): -> (labels, stats).
        `labels` is exactly what `apply(image)` returns; `stats` is `stats.label_statistics(image, labels, ...)` (spacing only for
        numpy input, in its axis order; names default to the model's: R231 right / left lung, LTRCLobes and the fused mode the five
        lobes, a checkpoint of its own "label k").  On one GPU the volume crosses to the device once: the statistics are computed
        from the device-resident input and labels in the caller's orientation.  The multi-GPU forms take the labels of their
        `apply` and upload them once, with the volume, to the first engine."""
        from . import stats as st

        arr, sp, to_phys, orientation, vol = self._volume_input("apply_with_stats", image, spacing)
        n_labels, nm = self._model_labels(names)
        if self._on_host(arr):
            labels = self.apply(image)
            raw = self.engine.label_stats(labels, vol, n_labels)
        else:
            with self._device_labels(vol, orientation) as lb:
                raw = self.engine.label_stats_dev(lb.back, lb.raw, n_labels)  # (returns once the result is on the host: the stream has run)
            labels = lb.labels
        return labels, st.finalize(raw, sp, percentiles, thresholds, nm, to_phys)

    def apply_with_texture(self, image, hu_range=(-1000, 199), bin_width=25, distance=1, names=None, aggregate="average"):
        """`apply(image)` plus the GLCM / GLRLM texture features of its labels (extension; lungmask_amd.texture): -> (labels, texture).
        `labels` is exactly what `apply(image)` returns; `texture` is `texture.texture_features(image, labels, ...)` (names default to
        the model's, as in `apply_with_stats`).  On one GPU the volume crosses to the device once: the matrices are computed from the
        device-resident input and labels in the caller's orientation, and the `lung` entry from the returned labels binarised and
        uploaded once.  The multi-GPU forms take the labels of their `apply` and upload them once, with the volume, to the first
        engine."""
        from . import texture as tx

        if aggregate not in ("average", "merge"):
            raise ValueError(f"aggregate: 'average' or 'merge', got {aggregate!r}")
        lo, hi, bw, dist, _ = tx.check_parameters(hu_range, bin_width, distance)
        arr, _, _, orientation, vol = self._volume_input("apply_with_texture", image)
        n_labels, nm = self._model_labels(names)
        if self._on_host(arr):
            labels = self.apply(image)
            return labels, tx.texture_features(arr, labels, n_labels=n_labels, hu_range=(lo, hi), bin_width=bw, distance=dist, names=nm,
                                               aggregate=aggregate, engine=self.engine)
        with self._device_labels(vol, orientation) as lb:
            raw = tx.matrices_dev(self.engine, lb.back, lb.raw, n_labels, lo, hi, bw, dist)  # (returns once the result is on the host)
            lb.back.upload(lb.fetch() > 0)
            raw_lung = tx.matrices_dev(self.engine, lb.back, lb.raw, 2, lo, hi, bw, dist)
        return lb.labels, tx.finalize(raw, raw_lung, nm, aggregate)

    def apply_roi(self, image, spacing_out=None, margin_mm=5.0, keep=None, dilate_mm=0.0, mask_outside=True, fill=-1024, window=None,
                  dtype=np.float32, spacing=None):
        """`apply(image)` plus the lung ROI cut out with its labels (extension; lungmask_amd.roi): -> (labels, roi).  `labels` is
        exactly what `apply(image)` returns; `roi` is `roi.extract_roi(image, labels, ...)`: the box of the kept labels grown by
        `margin_mm`, resampled to `spacing_out` (None: the source spacing, a pure crop), blanked to `fill` outside the kept labels
        (`dilate_mm`: and their surroundings), optionally windowed to [0, 1] -- see lungmask_amd/roi.py for the definition.
        `spacing`: numpy input only, in its axis order.  On one GPU the volume crosses to the device once: the ROI is computed from
        the device-resident input and labels in the caller's orientation.  The multi-GPU forms take the labels of their `apply` and
        upload them once, with the volume, to the first engine."""
        from . import roi as lmroi

        arr, sp, _, orientation, vol = self._volume_input("apply_roi", image, spacing)
        lmroi.check_arguments(vol.dtype, sp, spacing_out, margin_mm, keep, dilate_mm, window, dtype)
        kw = dict(spacing_out=spacing_out, margin_mm=margin_mm, keep=keep, dilate_mm=dilate_mm, mask_outside=mask_outside, fill=fill,
                  window=window, dtype=dtype)
        if self._on_host(arr):
            labels = self.apply(image)
            return labels, lmroi.extract_roi(image, labels, spacing=spacing, engine=self.engine, **kw)
        with self._device_labels(vol, orientation) as lb:
            img, out_lab, info = self.engine.roi_dev(lb.raw, lb.back, spacing=sp, **kw)  # (the box's read-back waits for the labels)
            lb.add(img, out_lab)
            result = lmroi.from_device(img, out_lab, info, lmroi._geometry_of(image))
        return lb.labels, result

    def apply_resampled(self, volume, spacing_out=1.0, like=None, order=3, label_mode="linear", fill=-1024, dtype=np.float32, spacing=None):
        """`apply(volume)` plus the volume and its labels resampled onto another grid (extension; lungmask_amd.resample): -> (labels,
        resampled).  `labels` is exactly what `apply(volume)` returns; `resampled` carries `.image` (`resample.resample_image(volume,
        grid, order=order, fill=fill, dtype=dtype)`), `.labels` (`resample.resample_labels(labels, grid, mode=label_mode)`), `.grid`,
        `.meta()` and `.as_volume()` / `.labels_volume()`.  The grid is `like` (a `resample.Grid`, a Volume or an image) or, without
        it, `resample.Grid.isotropic(volume, spacing_out)`: the same box with new spacing (one value or three in array axis order).
        `order` 0, 1 or 3 (cubic B-spline, the radiomics convention for images); `label_mode` "nearest" or "linear".  `spacing`:
        numpy input only, in its axis order.  On one GPU the volume crosses to the device once: both results are computed from the
        device-resident input and labels in the caller's orientation.  The multi-GPU forms take the labels of their `apply` and
        upload them once, with the volume, to the first engine."""
        from . import resample as rs

        arr, sp, _, orientation, vol = self._volume_input("apply_resampled", volume, spacing)
        if arr.shape[0] == 0:
            raise ValueError("apply_resampled: the volume has no slice")
        if label_mode not in ("nearest", "linear"):
            raise ValueError(f"label_mode: 'nearest' or 'linear', got {label_mode!r}")
        dt = rs.image_dtype(order, vol.dtype, dtype if order != 0 else None)
        src_grid = rs.Grid.of(volume if not isinstance(volume, np.ndarray) else arr, spacing)
        grid = rs.Grid.of(like) if like is not None else rs.Grid.isotropic(src_grid, spacing_out)
        has_geometry = not isinstance(volume, np.ndarray) or spacing is not None
        eng = self.engine
        if self._shard is not None:
            labels = self.apply(volume)
            with eng.scope() as dev:
                img, lab = rs.resample_pair_dev(eng, dev.upload(vol), dev.upload(labels), src_grid, grid, order, label_mode, fill, dt, dev)
        else:
            with self._device_labels(vol, orientation) as lb:
                img, lab = rs.resample_pair_dev(eng, lb.raw, lb.back, src_grid, grid, order, label_mode, fill, dt, lb)
            labels = lb.labels
        return labels, rs.Resampled(img, lab, grid, order, label_mode, has_geometry)

    def apply_registered(self, volume, moving, transform="rigid", margin_mm=10.0, order=3, spacing=None, moving_spacing=None, **register_kw):
        """`apply(volume)` plus the registration of a second image onto it (extension; lungmask_amd.registration): -> (labels, reg).
        `labels` is exactly what `apply(volume)` returns; `reg` is `registration.register(volume, moving, transform,
        labels=morphology.dilate(labels, margin_mm), **register_kw)`: only the lungs and a rim of `margin_mm` around them are
        sampled, so differing fields of view, the table and the arms take no part, and their centroid is the rotation centre.
        `reg.image` is `moving` on `volume`'s grid (`reg.resample(moving, order=order)` as an array).  `register_kw`: initial (an
        `Affine`), metric, bins, hu_range, moving_hu_range, levels_mm, min_overlap, max_evaluations.  `spacing`, `moving_spacing`:
        numpy inputs only, in their axis order.  ValueError when no voxel is labelled.  Works in every mode, the fused one
        included.  On one GPU the volume crosses to the device once: the registration is computed from the device-resident input
        and labels in the caller's orientation; the multi-GPU forms take the gathered labels of their `apply` and upload them once,
        with the volume, to the first engine."""
        return self._registered("apply_registered", volume, moving, transform, margin_mm, order, spacing, moving_spacing, register_kw)[:2]

    def _registered(self, who, volume, moving, transform, margin_mm, order, spacing, moving_spacing, register_kw, after=None):
        """`apply_registered` -> (labels, reg, extra).  `after(raw, lab, mv_dev, field_dev, affine, fixed_grid, moving_grid, scope)`
        enqueues further work on the device-resident pieces (the volume, the labels, the moving volume, no field, the transform found)
        and returns a callable that collects it once the engine has been waited for: its result is `extra`.  What `apply_pair`
        hangs its analysis on."""
        from . import registration as lmreg
        from . import resample as rs

        sp, orientation, vol, fixed_grid, moving_grid, mv, dt = self._two_image_input(
            who, volume, moving, transform, margin_mm, order, spacing, moving_spacing, register_kw, lmreg._volume_array)
        eng = self.engine

        def run(raw, lab, scope):
            reg, _, mv_dev = self._register_in_lungs(who, raw, lab, scope, fixed_grid, moving_grid, mv, sp, margin_mm, transform, register_kw)
            A, b = rs.index_map(moving_grid, fixed_grid, reg.transform)
            img = scope.add(eng.resample_dev(mv_dev, A, b, fixed_grid.shape, rs._ORDERS[order], -1024, dt))
            collect = after(raw, lab, mv_dev, None, reg.transform, fixed_grid, moving_grid, scope) if after is not None else None
            eng.sync()
            reg.image = img.download()
            return reg, collect() if collect is not None else None

        return self._labels_then(volume, vol, orientation, run)

    def _two_image_input(self, who, volume, moving, transform, margin_mm, order, spacing, moving_spacing, register_kw, load, deformable_kw=None):
        """The opening `_registered` and `_deformable` share: the checks of the volume, the rim, the keyword arguments (with
        `deformable_kw` those and their schedule too) and the transform, the two grids, and `moving` as the array `load` makes of it
        (`registration._volume_array` keeps uint8, `resample._image_array` does not) -> (spacing, orientation, the volume for the
        engine, fixed grid, moving grid, moving array, the dtype of the resampled image)."""
        from . import morphology as lmmorph
        from . import registration as lmreg
        from . import resample as rs

        arr, sp, _, orientation, vol = self._volume_input(who, volume, spacing)
        if arr.shape[0] == 0:
            raise ValueError(f"{who}: the volume has no slice")
        lmmorph.check_arguments("dilate", margin_mm, sp, None, (0,))
        unknown = (set(register_kw) - self._REGISTER_KW) | (set(deformable_kw or ()) - self._DEFORMABLE_KW)
        if unknown:
            raise TypeError(f"{who}: unexpected arguments {sorted(unknown)}")
        if register_kw.get("initial") is not None and not isinstance(register_kw["initial"], rs.Affine):
            raise TypeError(f"{who}: initial must be an Affine")
        if transform not in lmreg.TRANSFORMS:
            raise ValueError(f"transform: one of {sorted(lmreg.TRANSFORMS)}, got {transform!r}")
        if deformable_kw is not None:
            from . import deformable as lmdef

            lmdef.check_schedule(deformable_kw.get("levels_mm", (8.0, 4.0, 2.0)), deformable_kw.get("iterations", (60, 40, 20)),
                                 deformable_kw.get("patience", lmdef.PATIENCE), deformable_kw.get("den_min", lmdef.DEN_MIN))
            lmdef.check_metric(deformable_kw.get("metric", "ssd"), deformable_kw.get("window_mm"), deformable_kw.get("var_eps", lmdef.VAR_EPS),
                               deformable_kw.get("a_max", lmdef.A_MAX))
        fixed_grid = rs.Grid.of(volume if not isinstance(volume, np.ndarray) else arr, spacing)
        moving_grid = rs.Grid.of(moving if not isinstance(moving, np.ndarray) else np.asarray(moving), moving_spacing)
        mv = load(moving)
        return sp, orientation, vol, fixed_grid, moving_grid, mv, rs.image_dtype(order, mv.dtype, None)

    def _labels_then(self, volume, vol, orientation, run):
        """`run(raw, lab, scope)` on the device-resident volume and its labels -> (labels, *its result): the sharded form takes the
        gathered labels of `apply` and uploads them once, with the volume, to the first engine; one engine runs under
        `_device_labels`."""
        if self._shard is not None:
            labels = self.apply(volume)
            with self.engine.scope() as dev:
                return (labels,) + run(dev.upload(vol), dev.upload(labels), dev)
        with self._device_labels(vol, orientation) as lb:
            result = run(lb.raw, lb.back, lb)
        return (lb.labels,) + result

    def _register_in_lungs(self, who, raw, lab, scope, fixed_grid, moving_grid, mv, sp, margin_mm, transform, register_kw):
        """The affine stage `apply_registered` and `apply_deformable` share, on the device-resident volume `raw` and labels `lab`:
        the labels dilated by `margin_mm` (the sampling region), their centroid as the rotation centre, `registration.register_dev`
        -> (Registration, the dilated labels, the moving volume), the two device arrays owned by `scope`."""
        from . import registration as lmreg

        eng = self.engine
        try:
            rim = scope.add(eng.morph_dev(lab, "dilate", margin_mm, spacing=sp)[0])
        except _native.NoKeptVoxel:
            raise ValueError(f"{who}: no voxel is labelled, nothing to register on") from None
        acc = eng.label_stats_dev(rim, raw, 16, hist=False)
        voxels = int(sum(int(v) for v in acc["voxels"][1:]))
        centre = fixed_grid.index_to_physical([int(sum(int(s) for s in acc["index_sum"][1:, a])) / voxels for a in range(3)])
        mv_dev = scope.add(eng.to_device(mv))
        reg = lmreg.register_dev(eng, raw, mv_dev, fixed_grid, moving_grid, scope, transform, rim, None, centre, **register_kw)
        return reg, rim, mv_dev

    _REGISTER_KW = {"initial", "metric", "bins", "hu_range", "moving_hu_range", "levels_mm", "min_overlap", "max_evaluations"}
    _DEFORMABLE_KW = {"levels_mm", "iterations", "sigma_mm", "max_step_mm", "den_min", "patience", "metric", "window_mm", "var_eps", "a_max"}

    def apply_deformable(self, volume, moving, transform="rigid", margin_mm=10.0, order=3, spacing=None, moving_spacing=None, register_kw=None,
                         inverse=False, **deformable_kw):
        """`apply(volume)` plus the two-stage registration of a second image onto it (extension; lungmask_amd.deformable): ->
        (labels, reg).  `labels` is exactly what `apply(volume)` returns.  First the affine stage of `apply_registered` (`transform`,
        `register_kw`: its keyword arguments as a dict) inside the lungs dilated by `margin_mm`; then
        `deformable.register_deformable(volume, moving, initial=that transform, labels=the same dilated labels, **deformable_kw)`
        (levels_mm, iterations, sigma_mm, max_step_mm, den_min, patience, and metric, window_mm, var_eps, a_max: `metric="lcc"` is the
        local correlation metric for an inspiration / expiration pair): only the lungs and their rim take demons steps.  `reg` is
        the `DeformableRegistration`; `reg.affine_registration` the affine stage's `Registration`; `reg.image` is `moving` on
        `volume`'s grid (`reg.resample(moving, order=order)` as an array).  `spacing`, `moving_spacing`: numpy inputs only, in their
        axis order.  ValueError when no voxel is labelled.  Works in every mode, the fused one included.  On one GPU the volume
        crosses to the device once: both stages run on the device-resident input and labels in the caller's orientation; the
        multi-GPU forms take the gathered labels of their `apply` and upload them once, with the volume, to the first engine.
        `inverse=True`: also the inverse transform, from the same device-resident field and labels, in every mode --
        `reg.inverse_field` (`deformable.invert(reg.field, onto=the moving grid)`, a field on `moving`'s grid), `reg.inverse_info`
        (also `reg.meta()["inverse"]`) and `reg.labels_on_moving`: `labels` carried onto `moving`'s grid,
        `deformable.warp_labels(labels, reg.inverse_field, "linear")` as an array."""
        return self._deformable("apply_deformable", volume, moving, transform, margin_mm, order, spacing, moving_spacing, register_kw, inverse,
                                deformable_kw)[:2]

    def _deformable(self, who, volume, moving, transform, margin_mm, order, spacing, moving_spacing, register_kw, inverse, deformable_kw,
                    after=None):
        """`apply_deformable` -> (labels, reg, extra); `after` as for `_registered`, with the device-resident field and the affine
        under it."""
        from . import deformable as lmdef
        from . import resample as rs

        register_kw = dict(register_kw or {})
        sp, orientation, vol, fixed_grid, moving_grid, mv, dt = self._two_image_input(
            who, volume, moving, transform, margin_mm, order, spacing, moving_spacing, register_kw, rs._image_array, deformable_kw)
        eng = self.engine

        def run(raw, lab, scope):
            first, rim, mv_dev = self._register_in_lungs(who, raw, lab, scope, fixed_grid, moving_grid, mv, sp, margin_mm, transform, register_kw)
            reg = lmdef.register_deformable_dev(eng, raw, mv_dev, fixed_grid, moving_grid, scope, first.transform, rim, None, **deformable_kw)
            reg.affine_registration = first
            img = scope.add(lmdef.warp_dev(eng, mv_dev, reg.field_dev, moving_grid, fixed_grid, first.transform, rs._ORDERS[order], -1024, dt, scope))
            if inverse:
                inv, inv_grid, inv_affine, info = lmdef.invert_dev(eng, reg.field_dev, fixed_grid, first.transform, scope, onto=moving_grid)
                on_moving = scope.add(lmdef.warp_dev(eng, lab, inv, fixed_grid, inv_grid, inv_affine, "label_linear", 0, np.uint8, scope))
                eng.sync()
                reg.inverse_field, reg.inverse_info = lmdef.DisplacementField(inv.download(), inv_grid, inv_affine), info
                reg._inverse_key = (30, 0.01)
                reg.labels_on_moving = on_moving.download()
            collect = after(raw, lab, mv_dev, reg.field_dev, first.transform, fixed_grid, moving_grid, scope) if after is not None else None
            eng.sync()
            reg.image, reg.field_dev = img.download(), None
            return reg, collect() if collect is not None else None

        return self._labels_then(volume, vol, orientation, run)

    def apply_pair(self, volume, moving, deformable=True, roles=("inspiration", "expiration"), fixed_threshold=None, moving_threshold=None,
                   hu_range=(-1000, -500), air_hu=-1000.0, keep=None, n_labels=None, names=None, maps=("classes", "change", "jacobian"),
                   spacing=None, moving_spacing=None, transform="rigid", margin_mm=10.0, register_kw=None, deformable_kw=None):
        """`apply(volume)`, the registration of a second CT of the same patient onto it and their paired analysis (extension;
        lungmask_amd.pairs): -> (labels, reg, pair).  `labels` is exactly what `apply(volume)` returns.  `reg` is
        `apply_deformable(volume, moving, transform, margin_mm, register_kw=register_kw, **deformable_kw)`'s result, or with
        `deformable=False` `apply_registered(volume, moving, transform, margin_mm, **register_kw)`'s.  `pair` is
        `pairs.pair_analysis(volume, moving, labels, reg, roles, ...)` with the model's label names and label count unless `names` /
        `n_labels` are given: the parametric response map, the mass-corrected density change and the Jacobian inside the labels,
        with the per-label table (see lungmask_amd/pairs.py for the arguments and for what it does not do: no median filter, no
        clinical validation of the thresholds).  For the default roles, an inspiration / expiration pair, pass
        `deformable_kw=dict(metric="lcc")`: the default metric assumes one intensity scale in both scans.  Works in every mode, the fused one included: the analysis runs on the
        device-resident volume, labels, moving volume and field, so nothing but its results crosses back; the multi-GPU forms take
        the gathered labels of their `apply` and upload them once, with the volume, to the first engine."""
        from . import deformable as lmdef
        from . import pairs as lmpairs

        cfg = lmpairs.check_arguments(roles, fixed_threshold, moving_threshold, hu_range, air_hu, keep, n_labels, maps)
        model_rows, model_names = self._model_labels(names)
        rows = cfg["n_labels"] if cfg["n_labels"] is not None else (lmpairs.label_count(np.zeros(0, np.uint8), None, names) if names else model_rows)
        eng = self.engine
        has_mm = not isinstance(volume, np.ndarray) or spacing is not None

        def after(raw, lab, mv_dev, field_dev, affine, fixed_grid, moving_grid, scope):
            table, out, scale = lmpairs.pair_dev(eng, raw, lab, mv_dev, field_dev, fixed_grid, moving_grid, affine, scope, cfg, rows)
            sp_mm = lmdef.spacing_zyx(fixed_grid) if has_mm else None
            return lambda: lmpairs.collect(table, out, cfg, model_names, sp_mm, scale, "deformable" if field_dev is not None else "affine")

        if deformable:
            return self._deformable("apply_pair", volume, moving, transform, margin_mm, 3, spacing, moving_spacing, register_kw, False,
                                    dict(deformable_kw or {}), after)
        if deformable_kw:
            raise TypeError("apply_pair: deformable_kw needs deformable=True")
        return self._registered("apply_pair", volume, moving, transform, margin_mm, 3, spacing, moving_spacing, dict(register_kw or {}), after)

    def apply_mesh(self, image, labels=None, per_label=True, smooth=0, lam=0.5, mu=-0.53, spacing=None):
        """`apply(image)` plus the surface meshes of its labels (extension; lungmask_amd.mesh): -> (labels, meshes).  `labels` (the
        first result) is exactly what `apply(image)` returns.  `meshes` is {label value: Mesh} with `per_label` -- one mesh for each
        of the argument `labels` (label values; None: every label of the model) that has a voxel, each equal to
        `mesh.extract_surface(result, label=k)` -- and {"lung": Mesh} of those labels together (None: every label >= 1) without.
        `smooth`, `lam`, `mu`: Taubin smoothing, see lungmask_amd/mesh.py.  `spacing`: numpy input only, in its axis order.  Vertices
        are LPS millimetres for images, whatever their orientation.  On one GPU the meshes are taken from the device-resident labels in
        the caller's orientation, one device call per mesh; the multi-GPU forms take the gathered labels of their `apply` and upload
        them once to the first engine."""
        from . import mesh as lmmesh

        arr, _, _, orientation, vol = self._volume_input("apply_mesh", image, spacing)
        affine = lmmesh.index_affine(image if not isinstance(image, np.ndarray) else arr, spacing)
        lmmesh.label_list(labels)
        if int(smooth) != smooth or smooth < 0:
            raise ValueError(f"smooth: a number of iterations >= 0, got {smooth!r}")
        every = list(range(1, max(2, self.engine.n_classes(0))))
        kw = dict(labels=labels, per_label=per_label, smooth=smooth, lam=lam, mu=mu, all_labels=every)
        if arr.shape[0] == 0:
            raise ValueError("apply_mesh: the volume has no slice")
        if self._shard is not None:
            result = self.apply(image)
            with self.engine.scope() as dev:
                return result, lmmesh.surfaces_dev(self.engine, dev.upload(result), affine, **kw)
        with self._device_labels(vol, orientation, free_input=True) as lb:
            meshes = lmmesh.surfaces_dev(self.engine, lb.back, affine, **kw)
        return lb.labels, meshes

    def apply_closed(self, volume, radius_mm=10.0, into=(0,), spacing=None):
        """`apply(volume)` plus its morphological closing (extension; lungmask_amd.morphology): -> (labels, closed).  `labels` is
        exactly what `apply(volume)` returns; `closed` is `morphology.close(labels, radius_mm, into=into)` with the image's spacing:
        every label >= 1 together is closed by a ball of `radius_mm` -- juxta-pleural nodules, consolidations and dense fibrosis cut
        out of the mask come back -- and each new voxel takes the nearest label, so lobes stay lobes.  `into`: the label values a
        new voxel may overwrite.  `spacing`: numpy input only, in its axis order (None: the radius is in voxels).  No labelled voxel:
        `closed` equals `labels`.  Works in every mode, the fused one included.  On one GPU the closing is computed from the
        device-resident labels in the caller's orientation, without a round trip; the multi-GPU forms (device_ids, dist, several
        engines) are supported too: they take the gathered labels of their `apply` and upload them once to the first engine."""
        from . import morphology as lmmorph

        arr, sp, _, orientation, vol = self._volume_input("apply_closed", volume, spacing)
        lmmorph.check_arguments("close", radius_mm, sp, None, into)
        if self._on_host(arr):
            labels = self.apply(volume)
            if not labels.any():
                return labels, labels.copy()
            return labels, self.engine.morph(labels, "close", radius_mm, spacing=sp, into=into)[0]
        with self._device_labels(vol, orientation, free_input=True) as lb:
            try:
                out = lb.add(self.engine.morph_dev(lb.back, "close", radius_mm, spacing=sp, into=into)[0])  # (the box's read-back waits for the labels)
                closed = out.download()
            except _native.NoKeptVoxel:  # no labelled voxel: nothing to close (every other error is the caller's)
                closed = lb.fetch().copy()
        return lb.labels, closed

    def apply_with_clusters(self, volume, threshold=-950, hu_range=None, connectivity=6, spacing=None):
        """`apply(volume)` plus the cluster analysis of its labels (extension; lungmask_amd.components): -> (labels, clusters).
        `labels` is exactly what `apply(volume)` returns; `clusters` is `components.cluster_analysis(volume, labels, threshold,
        hu_range, connectivity)` with the model's label names: per label and for the whole lung the connected clusters of voxels with
        hu < threshold (or inside `hu_range`), their count, sizes and the cumulative cluster-size exponent D.  `spacing`: numpy input
        only, in its axis order.  Works in every mode, the fused one included.  On one GPU the volume crosses to the device once: the
        clusters are computed from the device-resident input and labels in the caller's orientation; the multi-GPU forms (device_ids,
        dist, several engines) take the gathered labels of their `apply` and upload them once, with the volume, to the first engine."""
        from . import components as cp

        arr, sp, _, orientation, vol = self._volume_input("apply_with_clusters", volume, spacing)
        rng = cp.cluster_range(threshold, hu_range)
        cp.check_arguments(rng, None, connectivity)
        thr = None if hu_range is not None else threshold
        _, nm = self._model_labels()
        if self._on_host(arr):
            labels = self.apply(volume)
            return labels, cp.cluster_analysis(arr, labels, threshold, hu_range, connectivity, spacing=sp, names=nm, engine=self.engine)
        with self._device_labels(vol, orientation) as lb:
            clusters = cp.analysis_dev(self.engine, lb.back, lb.raw, rng, connectivity, sp, nm, thr)  # (returns once the tables are on the host)
        return lb.labels, clusters

    def apply_denoised(self, volume, method="median", size=3, sigma_mm=None, masked=True, spacing=None):
        """`apply(volume)` plus the noise-reduced volume (extension; lungmask_amd.filters): -> (labels, filtered).  `labels` is exactly
        what `apply(volume)` returns; `filtered` is `filters.median(volume, size, labels=labels)` (method "median": the input's dtype)
        or `filters.gaussian(volume, sigma_mm, labels=labels)` (method "gaussian": float32, `sigma_mm` in millimetres of the image's
        spacing, voxels without one), confined to the labelled voxels with `masked` (every other voxel keeps its value; no labelled
        voxel: the volume as it is) and over the whole volume without.  `spacing`: numpy input only, in its axis order.  Works in
        every mode, the fused one included.  On one GPU the volume crosses to the device once: the filter runs on the
        device-resident input and labels in the caller's orientation; the multi-GPU forms (device_ids, dist, several engines) take
        the gathered labels of their `apply` and upload them once, with the volume, to the first engine."""
        from . import filters as flt

        arr, sp, _, orientation, vol = self._volume_input("apply_denoised", volume, spacing)
        if method == "median":
            kw = dict(kind="median", size=size)
            _native.Engine._filter_params(**kw)
        elif method == "gaussian":
            if sigma_mm is None:
                raise ValueError("apply_denoised: method 'gaussian' needs sigma_mm")
            if sp is not None and not all(v > 0 and np.isfinite(v) for v in sp):
                raise ValueError(f"spacing needs three positive values in the array's axis order, got {sp!r}")
            kw = dict(kind="separable", taps=flt.separable_taps(sigma_mm, sp))
        else:
            raise ValueError(f"method: 'median' or 'gaussian', got {method!r}")
        on_device = vol.dtype in ((np.int16, np.int32, np.float32) if method == "median" else (np.int16, np.int32, np.int64, np.float32, np.float64))
        if self._on_host(arr) or not on_device:
            labels = self.apply(volume)
            lab = labels if masked and labels.any() else None
            if masked and lab is None:
                return labels, arr.copy() if method == "median" else arr.astype(np.float32)
            if method == "median":
                return labels, flt.median(arr, size, labels=lab, engine=self.engine)
            return labels, flt.gaussian(arr, sigma_mm, spacing=sp, labels=lab, engine=self.engine)
        with self._device_labels(vol, orientation) as lb:
            try:
                out = lb.add(self.engine.filter_dev(lb.raw, lb.back if masked else None, **kw))  # (the box's read-back waits for the labels)
                self.engine.sync()
                filtered = out.download()
            except _native.NoKeptVoxel:  # no labelled voxel: nothing is filtered (every other error is the caller's)
                filtered = vol.copy() if method == "median" else vol.astype(np.float32)
        return lb.labels, filtered if filtered.dtype == arr.dtype or method != "median" else filtered.astype(arr.dtype)


    def apply_with_vessels(self, volume, sigmas_mm=(1.0, 1.5, 2.0, 3.0), threshold=0.5, erode_mm=2.0, alpha=0.5, beta=0.5, c=100.0,
                           names=None, spacing=None):
        """`apply(volume)` plus the pulmonary vessel analysis of its labels (extension; lungmask_amd.vessels): -> (labels, result).
        `labels` is exactly what `apply(volume)` returns; `result.vesselness` is `vessels.vesselness(volume, sigmas_mm,
        labels=labels)` (Frangi's measure, the maximum over the scales in millimetres of the image's spacing, voxels without one; 0
        outside the labels), `result.scale` the 1-based index of the scale that gave it, `result.mask` the voxels with vesselness >=
        `threshold` inside the lung eroded by `erode_mm`, and `result.analysis` is `vessels.vessel_analysis`'s dict with the model's
        label names.  `spacing`: numpy input only, in its axis order.  No labelled voxel: zeros and an analysis of empties.  Works in
        every mode, the fused one included.  On one GPU the volume crosses to the device once: the filter runs on the
        device-resident input and labels in the caller's orientation; the multi-GPU forms (device_ids, dist, several engines) take
        the gathered labels of their `apply` and upload them once, with the volume, to the first engine."""
        from . import vessels as vs

        arr, sp, _, orientation, vol = self._volume_input("apply_with_vessels", volume, spacing)
        if sp is not None and not all(v > 0 and np.isfinite(v) for v in sp):
            raise ValueError(f"spacing needs three positive values in the array's axis order, got {sp!r}")
        vs.check_analysis_arguments(threshold, erode_mm)
        _native.Engine._vessel_params(vs.scale_sigmas(sigmas_mm, sp), 4.0, True, None, alpha, beta, c)
        _, nm = self._model_labels(names)
        kw = dict(sigmas_mm=sigmas_mm, threshold=threshold, erode_mm=erode_mm, spacing=sp, names=nm, alpha=alpha, beta=beta, c=c)
        if self._on_host(arr):
            labels = self.apply(volume)
            return labels, vs.vessel_result(arr, labels, engine=self.engine, **kw)
        with self._device_labels(vol, orientation) as lb:
            try:
                result = vs.result_dev(self.engine, lb.raw, lb.back, **kw)  # (the box's read-back waits for the labels)
            except _native.NoKeptVoxel:  # no labelled voxel (every other error is the caller's)
                kw.pop("alpha"), kw.pop("beta"), kw.pop("c")
                result = vs.empty_result(vol.shape, params={"alpha": float(alpha), "beta": float(beta), "c": float(c), "bright": True}, **kw)
        return lb.labels, result

    def apply_with_vessel_tree(self, volume, sigmas_mm=(1.0, 1.5, 2.0, 3.0), threshold=0.5, erode_mm=2.0, calibres_mm2=(5.0, 10.0),
                               alpha=0.5, beta=0.5, c=100.0, names=None, spacing=None):
        """`apply_with_vessels(volume, ...)` plus the centrelines of the vessel mask (extension; lungmask_amd.skeleton): -> (labels,
        result).  `labels` is exactly what `apply(volume)` returns; `result` is `skeleton.vessel_tree(volume, labels, ...)`: the
        fields of `apply_with_vessels`' result and `result.skeleton` (uint8 codes of the mask's curve skeleton: 0, or 1 + the number
        of skeleton neighbours), `result.calibre` (uint8, per mask voxel the calibre class of the nearest skeleton voxel; the classes
        are split at the radii of circles of `calibres_mm2`, by default BV5 / BV10's 5 and 10 mm^2, a conventional choice that is
        not clinically validated) and `result.tree` (per label and for the lung: skeleton voxels, segments, length in mm, junctions,
        ends, volume per calibre class; and the graph).  Works in every mode, as `apply_with_vessels` does: on one GPU everything
        runs on the device-resident input and labels, the multi-GPU forms upload the gathered labels once to the first engine."""
        from . import skeleton as sk
        from . import vessels as vs

        arr, sp, _, orientation, vol = self._volume_input("apply_with_vessel_tree", volume, spacing)
        if sp is not None and not all(v > 0 and np.isfinite(v) for v in sp):
            raise ValueError(f"spacing needs three positive values in the array's axis order, got {sp!r}")
        vs.check_analysis_arguments(threshold, erode_mm)
        sk.calibre_edges_mm(calibres_mm2)
        _native.Engine._vessel_params(vs.scale_sigmas(sigmas_mm, sp), 4.0, True, None, alpha, beta, c)
        _, nm = self._model_labels(names)
        kw = dict(sigmas_mm=sigmas_mm, threshold=threshold, erode_mm=erode_mm, alpha=alpha, beta=beta, c=c)
        if self._on_host(arr):
            labels = self.apply(volume)
            return labels, sk.vessel_tree(arr, labels, calibres_mm2=calibres_mm2, spacing=sp, names=nm, engine=self.engine, **kw)
        with self._device_labels(vol, orientation) as lb:
            try:
                result = sk.tree_dev(self.engine, lb.raw, lb.back, calibres_mm2, sp, nm, **kw)  # (the box's read-back waits for the labels)
            except _native.NoKeptVoxel:  # no labelled voxel (every other error is the caller's)
                result = sk.empty_vessel_tree(vol.shape, calibres_mm2, sp, nm, **kw)
        return lb.labels, result

    def apply_with_airways(self, volume, seed=None, cap_hu=-800, threshold=None, spacing=None, names=None, spur_factor=1.5, **rule_kw):
        """`apply(volume)` plus the airway segmentation (extension; lungmask_amd.airways): -> (labels, result).  `labels` is exactly
        what `apply(volume)` returns; `result` is `airways.segment_airways(volume, labels, ...)`: `result.mask` (uint8, the trachea
        and the bronchi that one global threshold reaches), `result.cost` (int16, the minimax flood from the seed), `result.threshold`,
        `result.seed`, `result.curve`, `result.analysis` (seed, threshold, volume, volume per label with the model's label names;
        "0" is what lies outside the lung labels) and `result.tree` (segments with generation, length and diameter).  `seed`:
        (z, y, x) in the caller's array, or None to look for the trachea; a volume in which none is found returns an empty result
        with the reason in `analysis["error"]` instead of raising, because the labels are still wanted.  `spacing`: numpy input
        only, in its axis order.  One global threshold, no leak repair; the defaults are conventional and not validated on patient
        data.  Works in every mode, as `apply_with_vessel_tree` does: on one GPU everything runs on the device-resident input and
        labels, the multi-GPU forms upload the gathered labels once to the first engine."""
        from . import airways as aw

        arr, sp, _, orientation, vol = self._volume_input("apply_with_airways", volume, spacing)
        if sp is not None and not all(v > 0 and np.isfinite(v) for v in sp):
            raise ValueError(f"spacing needs three positive values in the array's axis order, got {sp!r}")
        aw.check_arguments(cap_hu, threshold, seed, spur_factor, **rule_kw)
        _, nm = self._model_labels(names)
        kw = dict(seed=seed, cap_hu=cap_hu, threshold=threshold, spacing=sp, names=nm, spur_factor=spur_factor, **rule_kw)
        if self._on_host(arr):
            labels = self.apply(volume)
            return labels, aw.segment_or_empty(arr, labels, engine=self.engine, **kw)
        with self._device_labels(vol, orientation) as lb:
            result = aw.airways_dev(self.engine, lb.raw, lb.back, **kw)  # (no trachea: the empty result with analysis["error"])
        return lb.labels, result


def apply(image, model=None, force_cpu=False, batch_size=20, volume_postprocessing=True, tqdm_disable=False):
    """Deprecated shim, mask.py:235-255.  `model` may be a state_dict."""
    warnings.warn("The function `apply` will be removed in a future version. Please use the LMInferer class!", DeprecationWarning)
    sd = None
    if model is not None:
        sd = model.state_dict() if hasattr(model, "state_dict") else model
    inferer = LMInferer(force_cpu=force_cpu, batch_size=batch_size, volume_postprocessing=volume_postprocessing, tqdm_disable=tqdm_disable,
                        state_dict=sd)
    return inferer.apply(image)


def apply_fused(image, basemodel="LTRCLobes", fillmodel="R231", force_cpu=False, batch_size=20, volume_postprocessing=True, tqdm_disable=False):
    """Deprecated shim, mask.py:258-279."""
    warnings.warn("The function `apply_fused` will be removed in a future version. Please use the LMInferer class!", DeprecationWarning)
    inferer = LMInferer(modelname=basemodel, force_cpu=force_cpu, fillmodel=fillmodel, batch_size=batch_size,
                        volume_postprocessing=volume_postprocessing, tqdm_disable=tqdm_disable)
    return inferer.apply(image)
