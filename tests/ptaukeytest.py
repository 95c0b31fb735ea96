"""Test-only helpers of a powers-of-tau contribution: the host build of csrc/zkwg_ptau_key_core.h (tests/native/ptaukeytest.cpp) -- the
regular recoding, the per-lane scalars c t^k, "each point times its own scalar" on the CPU and the file operation over it."""
import ctypes as C

import nativelib

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
# the scalars every multiplication test meets: the ends of the range, both parities there, the only two that meet P = +-Q (0, r - 1)
EDGES = [0, 1, 2, 3, 4, R - 2, R - 1, 1 << 253, R - 3]


def load():
    lib = nativelib.build("ptaukeytest")
    u64, u64p = C.c_uint64, C.POINTER(C.c_uint64)
    lib.pk_violations.restype = C.c_ulonglong
    lib.pk_window.restype = C.c_uint32
    lib.pk_recode.restype = None
    lib.pk_recode.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
    lib.pk_powers.restype = C.c_int
    lib.pk_powers.argtypes = [C.c_char_p, C.c_char_p, u64, u64, C.c_void_p]
    lib.pk_mul.restype = C.c_int
    lib.pk_mul.argtypes = [C.c_int, C.c_char_p, u64, C.c_char_p, C.c_void_p, u64]
    lib.pk_apply_key_size.restype = C.c_int
    lib.pk_apply_key_size.argtypes = [C.c_char_p, u64, u64, u64p, C.c_char_p, u64]
    lib.pk_apply_key.restype = C.c_int
    lib.pk_apply_key.argtypes = [C.c_char_p, u64, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, u64, C.c_void_p, u64, u64p, u64, C.c_char_p, u64]
    return lib


def violations():
    return load().pk_violations()


def _le(v):
    return int(v).to_bytes(32, "little")


def recode(k):
    """-> (digits of k | 1 from the least significant window up, as the walk reads them; whether P is subtracted at the end)"""
    out = (C.c_int * 65)()
    load().pk_recode(_le(k), out)
    return list(out)[:64], bool(out[64])


def powers(c, t, first, n):
    """-> [c t^(first + k) mod r for k < n] by the per-lane function, or None when c or t is refused"""
    out = (C.c_uint8 * (32 * n))()
    if load().pk_powers(_le(c), _le(t), first, n, out) != 0:
        return None
    b = bytes(out)
    return [int.from_bytes(b[32 * k:32 * k + 32], "little") for k in range(n)]


def mul(group, points, scalars, piece=1 << 20):
    """scalars[i] * points[i] on the host mirror (bytes in the zkey's form); None when a point is refused"""
    pt = 64 if group == 1 else 128
    assert len(points) == pt * len(scalars)
    out = (C.c_uint8 * max(1, len(points)))()
    rc = load().pk_mul(group, bytes(points), len(scalars), b"".join(_le(s) for s in scalars), out, piece)
    return bytes(out)[:len(points)] if rc == 0 else None


def apply_key(data, tau, alpha, beta, section7=b"", piece=1 << 20):
    """-> (rc, message, new file or None) by zk_ptau_apply_key_host"""
    lib = load()
    size, err, out_len = C.c_uint64(), C.create_string_buffer(256), C.c_uint64()
    rc = lib.pk_apply_key_size(bytes(data), len(data), len(section7), C.byref(size), err, 256)
    if rc != 0:
        return rc, err.value.decode(), None
    out = (C.c_uint8 * size.value)()
    rc = lib.pk_apply_key(bytes(data), len(data), _le(tau), _le(alpha), _le(beta), bytes(section7), len(section7), out, size.value, C.byref(out_len), piece, err, 256)
    return rc, err.value.decode(), (bytes(out)[:out_len.value] if rc == 0 else None)
