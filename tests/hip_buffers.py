"""Caller-owned device memory for the GPU tests: hipMalloc / hipMemcpy through ctypes on the HIP runtime libnexus_amd.so is bound to.

TEST INFRASTRUCTURE ONLY.

    with DeviceBuffers() as dev:
        src = dev.upload(array)              # a device pointer (int); freed when the block is left
        dst = dev.alloc(nbytes)
        ...launch through the context, ctx.sync()...
        out = dev.download(dst, (n, 4), np.float32)

hipMemcpy is synchronous with respect to the host; work the context has queued on its own stream is waited for with ctx.sync()
before a download.
"""
import ctypes as C

import numpy as np

_H2D, _D2H = 1, 2
_hip = None


def _runtime():
    global _hip
    if _hip is None:
        hip = C.CDLL("libamdhip64.so.7")  # the HIP runtime libnexus_amd.so is already bound to (matched by soname)
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipFree.argtypes = [C.c_void_p]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip = hip
    return _hip


class DeviceBuffers:
    def __init__(self):
        self._hip = _runtime()
        self._owned = {}  # pointer -> bytes

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in list(self._owned):
            self._hip.hipFree(C.c_void_p(p))
        self._owned.clear()
        return False

    def alloc(self, nbytes):
        p = C.c_void_p()
        rc = self._hip.hipMalloc(C.byref(p), int(nbytes))
        assert rc == 0 and p.value, "hipMalloc(%d) -> %d" % (nbytes, rc)
        self._owned[p.value] = int(nbytes)
        return p.value

    def write(self, ptr, array, capacity=None):
        """copy a numpy array to device memory at ptr; the size is checked against the allocation (or `capacity` bytes for memory
        this object does not own, such as a context's buffer)"""
        a = np.ascontiguousarray(array)
        room = self._owned.get(ptr, capacity)
        assert room is not None and a.nbytes <= room, "write of %d bytes into %r" % (a.nbytes, room)
        rc = self._hip.hipMemcpy(C.c_void_p(ptr), a.ctypes.data_as(C.c_void_p), a.nbytes, _H2D)
        assert rc == 0, "hipMemcpy (host to device) -> %d" % rc

    def upload(self, array):
        a = np.ascontiguousarray(array)
        p = self.alloc(a.nbytes)
        self.write(p, a)
        return p

    def download(self, ptr, shape, dtype, capacity=None):
        out = np.zeros(shape, dtype)
        room = self._owned.get(ptr, capacity)
        assert room is not None and out.nbytes <= room, "read of %d bytes from %r" % (out.nbytes, room)
        rc = self._hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes, _D2H)
        assert rc == 0, "hipMemcpy (device to host) -> %d" % rc
        return out
