"""Ownership of the library's native plans: who may use a plan, on which stream, and when it is freed.

A plan is single-owner in the C ABI (one stream and one host thread at a time: its device workspace is per plan).  A
plan that several host threads share -- one handed out by a PlanCache -- is used through `run()`: its `lock` held,
the stream ordered behind the previous user's.  A plan is destroyed by close() or when its last holder drops it.
"""
import ctypes as C
import threading
from collections import OrderedDict

import numpy as np
import torch

from . import _lib, _dev


class NativePlan:
    """Owns one C plan handle (`_h`) and destroys it with the library function named by `_destroy`."""
    _destroy = None

    def __init__(self):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.lock = threading.RLock()

    @property
    def handle(self):
        return self._h

    def _enter_stream(self):
        """Call with `lock` held, BEFORE enqueueing on the current stream: the plan's workspace is about to be used
        there.  If the previous user enqueued on a DIFFERENT stream its work must finish first -- as a DEVICE-side
        dependency (an event recorded behind the previous user's enqueue, waited for by the current stream), never a
        host wait: with the reference's dask-thread pattern (several threads, one plan, a stream per thread,
        pcg.py:346-356) a host synchronize here would stall every thread queued on the lock until the previous thread's
        whole stream had drained.  Same stream: stream order already serialises the kernels.  Returns the current
        stream's handle."""
        cur = torch.cuda.current_stream()
        last = self.__dict__.get('_last_stream')
        if last is not None and last != cur:
            ev = torch.cuda.Event()
            ev.record(last)               # behind everything the previous user has enqueued so far (it holds no lock now)
            cur.wait_event(ev)
        self._last_stream = cur
        return cur.cuda_stream

    def run(self, fn_name, *args):
        """Enqueue the library's `fn_name(handle, *args, stream)` on the current stream: under `lock`, behind the
        previous user's work (_enter_stream), the status checked.  THE way into a native plan."""
        with self.lock:
            stream = self._enter_stream()
            _lib.check(getattr(self._lib, fn_name)(self._h, *args, stream))

    def close(self):
        """Destroy the plan once the device is idle; later calls do nothing."""
        if getattr(self, '_h', None) is not None and self._h.value:
            torch.cuda.synchronize()
            getattr(self._lib, self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PsiPlan(NativePlan):
    """pfb_psi plan: `nband` bands of an (nx, ny) image, one wavelet basis per entry of `ks` (K taps / 2, 0 for
    'self'), filters `filt` (nbasis, 4, 18) fp64, `nlevel` levels, dtype float32 / float64.  Nymax, Nxmax: the
    extents of one basis' packed coefficient block."""
    _destroy = 'pfb_psi_plan_destroy'

    def __init__(self, nband, nx, ny, ks, filt, nlevel, dtype):
        super().__init__()
        _dev.require_device()
        filt = np.ascontiguousarray(filt, dtype=np.float64)
        _lib.check(self._lib.pfb_psi_plan_create(int(nband), int(nx), int(ny), len(ks), (C.c_int * len(ks))(*ks),
                                                 filt.ctypes.data_as(C.POINTER(C.c_double)), int(nlevel),
                                                 _dev.code(dtype), C.byref(self._h)))
        ny_, nx_ = C.c_int(), C.c_int()
        _lib.check(self._lib.pfb_psi_plan_dims(self._h, C.byref(ny_), C.byref(nx_)))
        self.Nymax, self.Nxmax = ny_.value, nx_.value


def array_key(a):
    """"Is this the array the caller presented last time?" as a hashable key.  numpy: address, shape, dtype, strides and
    the sum of a strided sample of at most 257 elements (as a complex number: exact for real, integer and bool arrays,
    and the imaginary part of a complex one counts).  Tensors: data_ptr, shape, dtype, version counter and device.
    None is None; anything else is its identity."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        flat = a.reshape(-1)
        samp = flat[::max(1, flat.size // 257)][:257]
        return ('np', a.__array_interface__['data'][0], a.shape, str(a.dtype), a.strides, complex(samp.sum()))
    if isinstance(a, torch.Tensor):
        return ('t', a.data_ptr(), tuple(a.shape), str(a.dtype), a._version, str(a.device))
    return ('o', id(a))


class PlanCache:
    """Bounded LRU of shared plans.  get(key, make) returns the cached plan or stores make()'s; beyond `maxsize`
    entries the least recently used is dropped.  Dropping (and clear()) only releases the cache's reference: a plan
    is destroyed when its last holder lets go, so a thread that has fetched one can go on using it.

    A key made with array_key() holds an address, so an entry has to keep the array behind it alive: freed, its memory
    could come back as DIFFERENT data under the same key.  What is kept differs per cache, on purpose: operators/psf.py
    keeps tensors only (a pinned numpy psfhat cube can be gigabytes; its key samples the content), operators/gridder.py
    keeps all three of uvw, freq and mask, utils/misc.py keeps its coordinate tensors."""

    def __init__(self, maxsize):
        self.maxsize = maxsize
        self._entries = OrderedDict()
        self._lock = threading.Lock()

    def get(self, key, make):
        with self._lock:
            hit = self._entries.get(key)
            if hit is not None:
                self._entries.move_to_end(key)
                return hit
            made = self._entries[key] = make()
            while len(self._entries) > self.maxsize:
                self._entries.popitem(last=False)
            return made

    def clear(self):
        with self._lock:
            self._entries.clear()
