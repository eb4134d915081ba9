"""A stream that is truly the caller's, and caller's work on it, for tests of bn_ctx_set_stream.

Everything here goes to the HIP runtime directly through ctypes -- stream and event creation, asynchronous copies and
memsets, the caller's own device buffers -- so none of it passes through the library under test: the library cannot know
what the caller put on the stream, it can only keep its own launches in order on it.

A stream handle is valid only inside the runtime instance that made it, and a process may map more than one libamdhip64 (torch
ships one beside the ROCm installation's and asks for it by another name, so both get mapped).  What matters for a stream
handed to bn_ctx_set_stream is the ONE image the library under test calls into.  runtime() finds it the way the dynamic
linker bound the library's own HIP calls: every call the caller's side uses is looked up through the library's handle (its
dependency scope), dladdr names the image each lives in, and all must live in the same one; a definition of the same call in
the global scope at another address would have been bound first, so that case is refused (AmbiguousRuntime: the tests
skip, the reason names the images).  A stream created through these very entry points is the library's runtime's own,
however many other images the process maps.  No handle of any other image is ever passed to the library: a torch stream
belongs to torch's image and is valid for the library only in a process that maps a single image.
"""
import ctypes as C
import os
import time

import numpy as np

HIP_STREAM_NON_BLOCKING = 1
H2D, D2H, D2D = 1, 2, 3

_rt = None


class AmbiguousRuntime(Exception):
    pass


class _DlInfo(C.Structure):
    _fields_ = [("dli_fname", C.c_char_p), ("dli_fbase", C.c_void_p), ("dli_sname", C.c_char_p), ("dli_saddr", C.c_void_p)]


def mapped_hip_images():
    """Every libamdhip64 image mapped into this process (for the record: see runtime())."""
    paths = set()
    with open("/proc/self/maps") as f:
        for line in f:
            parts = line.split(None, 5)
            if len(parts) == 6 and "libamdhip64" in parts[5].rsplit("/", 1)[-1]:
                paths.add(parts[5].strip())
    return sorted(paths)


class _Runtime:
    pass


def runtime():
    """The HIP runtime image the library under test is bound to, as an object with the calls the caller's side uses (and
    .path, the image's file), or AmbiguousRuntime."""
    global _rt
    if isinstance(_rt, Exception):
        raise _rt
    if _rt is not None:
        return _rt
    import binius_amd._ffi as ffi

    ffi.lib()
    own = C.CDLL(ffi._SO)  # the handle of the library already loaded: lookups go through its dependencies, as its own calls did
    glob = C.CDLL(None)    # the global scope, which the dynamic linker searches first
    glob.dladdr.argtypes = [C.c_void_p, C.POINTER(_DlInfo)]
    vp, sz, i32, u32 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint
    sig = {
        "hipStreamCreateWithFlags": [C.POINTER(vp), u32],
        "hipStreamDestroy": [vp],
        "hipStreamSynchronize": [vp],
        "hipMemcpyAsync": [vp, vp, sz, i32, vp],
        "hipMemsetAsync": [vp, i32, sz, vp],
        "hipEventCreate": [C.POINTER(vp)],
        "hipEventDestroy": [vp],
        "hipEventRecord": [vp, vp],
        "hipEventElapsedTime": [C.POINTER(C.c_float), vp, vp],
        "hipMalloc": [C.POINTER(vp), sz],
        "hipFree": [vp],
    }
    rt, homes = _Runtime(), set()
    for name, args in sig.items():
        fn = getattr(own, name)
        addr = C.cast(fn, vp).value
        info = _DlInfo()
        if not glob.dladdr(addr, C.byref(info)) or not info.dli_fname:
            _rt = AmbiguousRuntime("%s of the library's runtime belongs to no mapped image" % name)
            raise _rt
        homes.add(os.path.realpath(info.dli_fname.decode()))
        try:
            other = C.cast(getattr(glob, name), vp).value
        except AttributeError:
            other = addr
        if other != addr:
            homes.add("another definition of %s in the global scope" % name)
        fn.argtypes = args
        fn.restype = i32
        setattr(rt, name, fn)
    if len(homes) != 1:
        _rt = AmbiguousRuntime("the library's HIP calls do not resolve to one image (%s; mapped: %s)" % (", ".join(sorted(homes)), ", ".join(mapped_hip_images())))
        raise _rt
    rt.path = homes.pop()
    _rt = rt
    return rt


def _ok(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed with HIP error %d" % (what, rc))


class DevBuf:
    """Device memory of the caller's own (hipMalloc), addressed in field elements of 16 bytes."""

    def __init__(self, owner, ptr, n):
        self.owner, self.ptr, self.len = owner, ptr, n


class CallerStream:
    """One non-blocking stream created by the caller, the caller's buffers and events, and the caller's work on the stream.
    close() destroys the stream exactly once; use as a context manager."""

    def __init__(self):
        self.rt = runtime()
        h = C.c_void_p()
        _ok(self.rt.hipStreamCreateWithFlags(C.byref(h), HIP_STREAM_NON_BLOCKING), "hipStreamCreateWithFlags")
        self.handle = h.value
        assert self.handle, "a created stream is never the null stream"
        self.destroyed = 0
        self._bufs, self._events, self._keep = [], [], []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def close(self):
        if self.handle is None:
            return
        self.rt.hipStreamSynchronize(self.handle)
        for e in self._events:
            self.rt.hipEventDestroy(e)
        for b in self._bufs:
            self.rt.hipFree(b.ptr)
        _ok(self.rt.hipStreamDestroy(self.handle), "hipStreamDestroy")
        self.destroyed += 1
        self.handle = None
        self._keep = []

    # ---- the caller's memory
    def malloc(self, n_elems):
        p = C.c_void_p()
        _ok(self.rt.hipMalloc(C.byref(p), 16 * n_elems), "hipMalloc")
        b = DevBuf(self, p.value, n_elems)
        self._bufs.append(b)
        return b

    def staged(self, arr):
        """A caller's device buffer that holds `arr` now (copied and waited for): the source of later asynchronous writes."""
        arr = np.ascontiguousarray(arr)
        b = self.malloc((arr.nbytes + 15) // 16)
        _ok(self.rt.hipMemcpyAsync(b.ptr, arr.ctypes.data, arr.nbytes, H2D, self.handle), "hipMemcpyAsync (H2D)")
        self.synchronize()
        return b

    # ---- the caller's work, all of it asynchronous on the stream
    def copy_d2d(self, dst_ptr, src_ptr, n_elems):
        _ok(self.rt.hipMemcpyAsync(dst_ptr, src_ptr, 16 * n_elems, D2D, self.handle), "hipMemcpyAsync (D2D)")

    def memset(self, dst_ptr, byte, n_elems):
        _ok(self.rt.hipMemsetAsync(dst_ptr, byte, 16 * n_elems, self.handle), "hipMemsetAsync")

    def read_async(self, src_ptr, n_elems):
        """Enqueues a device-to-host copy; the returned (n, 2) uint64 array is valid after synchronize()."""
        out = np.zeros((n_elems, 2), dtype=np.uint64)
        self._keep.append(out)
        _ok(self.rt.hipMemcpyAsync(out.ctypes.data, src_ptr, out.nbytes, D2H, self.handle), "hipMemcpyAsync (D2H)")
        return out

    def synchronize(self):
        _ok(self.rt.hipStreamSynchronize(self.handle), "hipStreamSynchronize")

    def event(self):
        e = C.c_void_p()
        _ok(self.rt.hipEventCreate(C.byref(e)), "hipEventCreate")
        self._events.append(e.value)
        return e.value

    def record(self, ev):
        _ok(self.rt.hipEventRecord(ev, self.handle), "hipEventRecord")

    def elapsed_ms(self, ev0, ev1):
        ms = C.c_float()
        _ok(self.rt.hipEventElapsedTime(C.byref(ms), ev0, ev1), "hipEventElapsedTime")
        return ms.value


class Delay:
    """Caller's work that needs no kernel of the caller's and keeps a stream busy: a chain of device-to-device copies between the
    halves of a large scratch buffer.  Whatever is enqueued behind it starts only when it is through, so a launch that went to
    another stream runs (and reads) long before the caller's writes behind the delay have happened.  The buffer and the two
    events that bracket the delay belong to `owner`; the delay itself goes to the stream given to enqueue()."""

    def __init__(self, owner, mib_per_copy=512, copies=48):
        self.owner, self.copies = owner, copies
        self.half = (mib_per_copy << 20) // 16
        self.buf = owner.malloc(2 * self.half)
        owner.memset(self.buf.ptr, 0x5A, 2 * self.half)
        owner.synchronize()
        self.ev0, self.ev1 = owner.event(), owner.event()

    def enqueue(self, cs):
        """Returns the host time of the first enqueue."""
        lo, hi = self.buf.ptr, self.buf.ptr + 16 * self.half
        t0 = time.perf_counter()
        cs.record(self.ev0)
        for i in range(self.copies):
            if i & 1:
                cs.copy_d2d(lo, hi, self.half)
            else:
                cs.copy_d2d(hi, lo, self.half)
        cs.record(self.ev1)
        return t0

    def ms(self):
        """Device time of the last delay; call after the stream it went to has been synchronised."""
        return self.owner.elapsed_ms(self.ev0, self.ev1)


def require_delay_covers(delay_ms, host_ms, what):
    """The ordering tests prove something only if the caller's writes were still far in the future when the library's call was
    issued: the delay on the device must be at least five times the host time of the whole enqueue."""
    print("caller-stream ordering [%s]: delay %.2f ms on the device, host enqueue %.3f ms" % (what, delay_ms, host_ms))
    assert delay_ms >= 5.0 * host_ms, "delay too short: %.2f ms on the device against %.3f ms of host enqueue time (%s)" % (delay_ms, host_ms, what)
