"""Device buffers for tests that wrap resident arrays (gq_reads_wrap_device): a numpy array copied
to device memory with the HIP runtime the library links (hipMalloc / hipMemcpy through ctypes),
exposing what native._ptr needs; or a zeroed buffer of a given size holding a few pieces (a pool
of gigabytes with a handful of reads in it, without a host array of that size)."""
import ctypes as C

import numpy as np

_hip = None


def hip():
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so.7")  # by SONAME: the runtime libgqpileup.so already uses
    return _hip


class DeviceArray:
    def __init__(self, a):
        a = np.ascontiguousarray(a)
        self._alloc(a.shape, a.dtype, a.nbytes)
        self._copy(0, a)

    @classmethod
    def sparse(cls, size, pieces, dtype=np.uint8):
        """`size` zeroed elements with the arrays of `pieces` = [(element offset, array)] copied in."""
        self = cls.__new__(cls)
        dtype = np.dtype(dtype)
        self._alloc((int(size),), dtype, int(size) * dtype.itemsize)
        assert hip().hipMemset(self.ptr, 0, C.c_size_t(self.nbytes)) == 0
        for off, a in pieces:
            a = np.ascontiguousarray(a, dtype)
            assert 0 <= off and off + a.shape[0] <= size
            self._copy(int(off) * dtype.itemsize, a)
        return self

    def _alloc(self, shape, dtype, nbytes):
        self.shape, self.dtype, self.nbytes = shape, dtype, max(nbytes, 16)
        self.ptr = C.c_void_p()
        assert hip().hipMalloc(C.byref(self.ptr), C.c_size_t(self.nbytes)) == 0

    def _copy(self, byte_off, a):
        if a.nbytes:
            assert hip().hipMemcpy(C.c_void_p(self.ptr.value + byte_off), a.ctypes.data_as(C.c_void_p),
                                   C.c_size_t(a.nbytes), 1) == 0

    def data_ptr(self):
        return self.ptr.value

    def __del__(self):
        if getattr(self, "ptr", None) and _hip is not None:
            _hip.hipFree(self.ptr)


def device_arrays(a):
    """The arrays of a packed read set on the device (scalars stay ints; DeviceArrays pass through)."""
    return {k: (v if isinstance(v, DeviceArray) else DeviceArray(np.asarray(v)) if np.ndim(v) else int(v))
            for k, v in a.items()}
