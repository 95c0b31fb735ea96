"""Test-only helpers of the powers-of-tau preparation: the host build of csrc/zkwg_ptau_core.h (tests/native/ptautest.cpp) -- the twiddle
recoder, the transform over points on the CPU and the file operation over it -- and an unprepared toy ceremony from a known trapdoor."""
import ctypes as C

import nativelib

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def load():
    lib = nativelib.build("ptautest")
    u64p = C.POINTER(C.c_uint64)
    lib.pt_violations.restype = C.c_ulonglong
    lib.pt_table.restype = None
    lib.pt_table.argtypes = [C.c_uint32, C.c_int, C.c_void_p]
    lib.pt_ntt.restype = C.c_int
    lib.pt_ntt.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_int]
    lib.pt_prepare_size.restype = C.c_int
    lib.pt_prepare_size.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, u64p, C.c_char_p, C.c_uint64]
    lib.pt_prepare.restype = C.c_int
    lib.pt_prepare.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, u64p, C.c_char_p, C.c_uint64]
    return lib


def violations():
    return load().pt_violations()


def twiddle_digits(log2_n, inverse):
    """-> per table entry e < 2^(log2_n - 1): the digits of the recoded w^e (w^-e), least significant first, 255 positions"""
    n = max(1, (1 << log2_n) >> 1)
    out = (C.c_uint32 * (16 * n))()
    load().pt_table(log2_n, int(inverse), out)
    res = []
    for e in range(n):
        nz = sum(out[16 * e + i] << (32 * i) for i in range(8))
        neg = sum(out[16 * e + 8 + i] << (32 * i) for i in range(8))
        assert neg & ~nz == 0 and nz >> 255 == 0
        res.append([(-1 if (neg >> i) & 1 else 1) if (nz >> i) & 1 else 0 for i in range(255)])
    return res


def ntt(group, points, inverse):
    """the transform of `points` (bytes in the zkey's form, a power of two of them) on the host mirror; None when a point is refused"""
    pt = 64 if group == 1 else 128
    n = len(points) // pt
    assert n * pt == len(points) and n & (n - 1) == 0 and n
    buf = C.create_string_buffer(bytes(points), len(points))
    rc = load().pt_ntt(group, buf, n.bit_length() - 1, int(inverse))
    return buf.raw if rc == 0 else None


def prepare(data, power=0):
    """-> (rc, message, prepared file or None) by zk_ptau_prepare_host"""
    lib = load()
    size, err, out_len = C.c_uint64(), C.create_string_buffer(256), C.c_uint64()
    rc = lib.pt_prepare_size(bytes(data), len(data), power, C.byref(size), err, 256)
    if rc != 0:
        return rc, err.value.decode(), None
    out = (C.c_uint8 * size.value)()
    rc = lib.pt_prepare(bytes(data), len(data), power, out, size.value, C.byref(out_len), err, 256)
    return rc, err.value.decode(), (bytes(out)[:out_len.value] if rc == 0 else None)


def ceremony_scalars(power, tau, alpha, beta):
    """the discrete logarithms of sections 2 - 5 of an unprepared file of that power"""
    n = 1 << power
    pw = [1]
    for _ in range(2 * n - 2):
        pw.append(pw[-1] * tau % R)
    return {2: pw, 3: pw[:n], 4: [alpha * x % R for x in pw[:n]], 5: [beta * x % R for x in pw[:n]]}


def toy_ceremony(power, tau, alpha, beta, points, ceremony_power=None, contributions=b""):
    """points(group, scalars) -> bytes.  -> an UNPREPARED .ptau (sections 1 - 7) from the trapdoor"""
    from zkwg import ptau
    s = ceremony_scalars(power, tau, alpha, beta)
    secs = {2: points(1, s[2]), 3: points(2, s[3]), 4: points(1, s[4]), 5: points(1, s[5]), 6: points(2, [beta])}
    return ptau.write_ptau(power, secs, ceremony_power=ceremony_power, contributions=contributions)


def lagrange_scalars(power, scalars):
    """the logarithms of sections 12 - 15 of the prepared file: per level the scalar inverse transform (oracle/pyref/ntt.ifft_fast) of the
    prefix; the last level of section 12 over the 2 n - 1 powers and a ZERO (the top coefficient dropped)"""
    from oracle.pyref import ntt
    out = {}
    for sid, src in ((12, 2), (13, 3), (14, 4), (15, 5)):
        lv = []
        for q in range(power + 1):
            lv += ntt.ifft_fast(scalars[src][:1 << q])
        if sid == 12:
            lv += ntt.ifft_fast(scalars[2] + [0])
        out[sid] = lv
    return out
