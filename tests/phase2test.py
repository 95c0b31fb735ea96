"""Test-only helpers of phase 2: the host build of csrc/zkwg_phase2_core.h (tests/native/phase2test.cpp) -- the recoder, the scaling
series of the kernels on the CPU and the file operation over it."""
import ctypes as C

import nativelib


def load():
    lib = nativelib.build("phase2test")
    u64p = C.POINTER(C.c_uint64)
    lib.p2_violations.restype = C.c_ulonglong
    lib.p2_recode.restype = None
    lib.p2_recode.argtypes = [C.c_char_p, C.POINTER(C.c_uint32)]
    lib.p2_scale.restype = C.c_int
    lib.p2_scale.argtypes = [C.c_int, C.c_char_p, C.c_uint64, C.c_char_p, C.c_void_p]
    lib.p2_apply_size.restype = C.c_int
    lib.p2_apply_size.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, u64p, C.c_char_p, C.c_uint64]
    lib.p2_apply.restype = C.c_int
    lib.p2_apply.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, u64p, C.c_char_p, C.c_uint64]
    return lib


def violations():
    return load().p2_violations()


def recode(s):
    """-> the digits of the non-adjacent form of s < 2^256, least significant first, as the kernel reads them"""
    out = (C.c_uint32 * 20)()
    load().p2_recode(int(s).to_bytes(32, "little"), out)
    nz = sum(out[i] << (32 * i) for i in range(9))
    neg = sum(out[9 + i] << (32 * i) for i in range(9))
    assert neg & ~nz == 0
    digits = [(-1 if (neg >> i) & 1 else 1) if (nz >> i) & 1 else 0 for i in range(out[18])]
    assert nz >> out[18] == 0 and sum(1 for d in digits if d) == out[19]
    return digits


def scale(group, points, s):
    """s * every point of `points` (bytes in the zkey's form) on the host mirror; None when a point is refused"""
    pt = 64 if group == 1 else 128
    n = len(points) // pt
    out = (C.c_uint8 * max(1, len(points)))()
    rc = load().p2_scale(group, bytes(points), n, int(s).to_bytes(32, "little"), out)
    return bytes(out)[:len(points)] if rc == 0 else None


def apply_delta(z, k, section10):
    """-> (rc, message, new key or None)"""
    lib = load()
    size, err, out_len = C.c_uint64(), C.create_string_buffer(256), C.c_uint64()
    rc = lib.p2_apply_size(bytes(z), len(z), len(section10), C.byref(size), err, 256)
    if rc != 0:
        return rc, err.value.decode(), None
    out = (C.c_uint8 * size.value)()
    rc = lib.p2_apply(bytes(z), len(z), int(k).to_bytes(32, "little"), bytes(section10), len(section10), out, size.value, C.byref(out_len), err, 256)
    return rc, err.value.decode(), (bytes(out)[:out_len.value] if rc == 0 else None)
