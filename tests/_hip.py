"""The HIP runtime through ctypes, for tests that hand the library device pointers without torch: hip_of() and a canary-padded buffer."""
import ctypes

CANARY = 0xA5
PAD = 4096


def hip_of():
    """the HIP runtime libzsmi.so is linked against (by its soname: the copy already loaded with it)"""
    from zstandard_amd import _lib
    _lib.lib()
    H = ctypes.CDLL("libamdhip64.so.7")
    H.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    H.hipFree.argtypes = [ctypes.c_void_p]
    H.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    H.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    return H


class Dev:
    """device buffer of n bytes + PAD canary bytes on each side; .p is the first byte after the front canary"""

    def __init__(self, H, n, fill=b""):
        self.H, self.n = H, n
        self.base = ctypes.c_void_p()
        assert H.hipMalloc(ctypes.byref(self.base), n + 2 * PAD) == 0
        assert H.hipMemset(self.base, CANARY, n + 2 * PAD) == 0
        self.p = self.base.value + PAD
        if fill:
            assert H.hipMemcpy(ctypes.c_void_p(self.p), fill, len(fill), 1) == 0

    def all(self) -> bytes:
        out = ctypes.create_string_buffer(self.n + 2 * PAD)
        assert self.H.hipMemcpy(out, self.base, self.n + 2 * PAD, 2) == 0
        return out.raw

    def free(self):
        self.H.hipFree(self.base)


HIP_OUT_OF_MEMORY = 2                                        # hipErrorOutOfMemory
BIG_BYTES = (1 << 32) + (64 << 20)


class OutOfDeviceMemory(Exception):
    """hipMalloc answered hipErrorOutOfMemory: the one condition a test of big places may skip on"""


class BigDev:
    """ONE device buffer of 2^32 + 64 MiB filled with the canary on the device (a memset: milliseconds), for items placed beyond 2 GiB and
    4 GiB.  .p is its first byte.  It is read and written through windows only: there is no whole-buffer copy in either direction"""

    def __init__(self, H, n=BIG_BYTES):
        self.H, self.n = H, n
        self.base = ctypes.c_void_p()
        rc = H.hipMalloc(ctypes.byref(self.base), n)
        if rc == HIP_OUT_OF_MEMORY:
            raise OutOfDeviceMemory(f"hipMalloc of {n} bytes: out of memory")
        assert rc == 0, ("hipMalloc", rc)
        self.p = self.base.value
        assert H.hipMemset(self.base, CANARY, n) == 0

    def write(self, off, data):
        assert 0 <= off and off + len(data) <= self.n
        if data:
            assert self.H.hipMemcpy(ctypes.c_void_p(self.p + off), bytes(data), len(data), 1) == 0

    def read(self, off, n) -> bytes:
        assert 0 <= off and off + n <= self.n and n <= 64 << 20
        out = ctypes.create_string_buffer(max(n, 1))
        if n:
            assert self.H.hipMemcpy(out, ctypes.c_void_p(self.p + off), n, 2) == 0
        return out.raw[:n]

    def refill(self, off, n):
        """the canary again over [off, off + n)"""
        assert 0 <= off and off + n <= self.n
        if n:
            assert self.H.hipMemset(ctypes.c_void_p(self.p + off), CANARY, n) == 0

    def free(self):
        self.H.hipFree(self.base)
