"""Test-only helpers of per-proof groth16 verification: the host build of csrc/zkwg_fexp_core.h and csrc/zkwg_fexp_host.h
(tests/native/fexptest.cpp) -- the steps of the final exponentiation a lane pair of the zk_fexp_* kernels runs, on 384-byte values, the sum
of a proof's public-input points, and the per-proof verifier with its stage on the host -- all with the range checks of zkwg_fq29.h."""
import ctypes as C

import nativelib
import pairtest

Q = pairtest.Q
# tests/native/fexptest.cpp ft_f12_op
CONJ, FROB1, FROB2, FROB3, CYC_SQR, POW_U, NINV = range(7)
PRE = 6                    # ft_f12_op(PRE + pre): zk_fexp_pre, pre = 1 .. 6 (conj, F1, F2, F3, F2 twice, the cyclotomic square)
# csrc/zkwg_fexp_core.h: the slots and the lengths of the program
SLOT_T1, SLOT_G, SLOT_OUT = 6, 1, 8
INV_STEPS, EASY_STEPS, ALL_STEPS = 4, 6, 22


def load():
    lib = nativelib.build("fexptest")
    u64, u32, vp = C.c_uint64, C.c_uint32, C.c_void_p
    lib.ft_counters.restype = None
    lib.ft_counters.argtypes = [vp]
    lib.ft_frob_const.restype = None
    lib.ft_frob_const.argtypes = [C.c_int, C.c_int, vp]
    lib.ft_f12_op.restype = None
    lib.ft_f12_op.argtypes = [C.c_int, C.c_char_p, vp]
    lib.ft_piece.restype = None
    lib.ft_piece.argtypes = [C.c_int, C.c_char_p, vp]
    lib.ft_program.restype = None
    lib.ft_program.argtypes = [C.c_char_p, u32, u32, u32, vp]
    lib.ft_host_pow.restype = None
    lib.ft_host_pow.argtypes = [C.c_char_p, C.c_char_p, u32, vp]
    lib.ft_vkx.restype = None
    lib.ft_vkx.argtypes = [C.c_char_p, C.c_char_p, u32, vp]
    lib.ft_verify_each.restype = C.c_int
    lib.ft_verify_each.argtypes = [C.c_char_p, C.c_char_p, u32, u64, C.c_char_p, C.c_char_p, vp, vp, vp, C.c_char_p, u64]
    return lib


def counters():
    """(preconditions violated by the values, by the bounds, results above their own bounds) of csrc/zkwg_fq29.h in this library"""
    out = (C.c_ulonglong * 3)()
    load().ft_counters(out)
    return tuple(out)


def frob_const(k, j):
    """the header's constant xi^(j (q^k - 1) / 6) -> (c0, c1), standard form"""
    out = (C.c_uint8 * 64)()
    load().ft_frob_const(k, j, out)
    return int.from_bytes(bytes(out[:32]), "little"), int.from_bytes(bytes(out[32:]), "little")


def f12_op(op, f):
    out = (C.c_uint8 * 384)()
    load().ft_f12_op(op, f, out)
    return bytes(out)


def piece(op, words, n_out):
    """one small piece (ft_piece) on standard-form integers below q -> n_out integers"""
    out = (C.c_uint8 * (32 * n_out))()
    load().ft_piece(op, b"".join(int(w).to_bytes(32, "little") for w in words), out)
    return [int.from_bytes(bytes(out[32 * i:32 * i + 32]), "little") for i in range(n_out)]


def program(values, last, slot):
    """the product of the 384-byte values, then steps [0, last) of the program -> the value in `slot`"""
    out = (C.c_uint8 * 384)()
    load().ft_program(b"".join(values), len(values), last, slot, out)
    return bytes(out)


def f12_inv(f):
    return program([f], INV_STEPS, SLOT_T1)


def easy(f):
    return program([f], EASY_STEPS, SLOT_G)


def final_exp(f, *more):
    """FE(f) by the new body, or FE of the product of f and `more` as zk_fexp_fold folds them"""
    return program([f, *more], ALL_STEPS, SLOT_OUT)


def host_pow(f, e):
    """f^e by the host's square-and-multiply over fq12_mul (csrc/zkwg_pairing.h)"""
    raw = int(e).to_bytes((int(e).bit_length() + 7) // 8, "little")
    out = (C.c_uint8 * 384)()
    load().ft_host_pow(f, raw, len(raw), out)
    return bytes(out)


def vkx(ic0, terms):
    """-(ic0 + the terms): 64-byte points in the zkey's form"""
    out = (C.c_uint8 * 64)()
    load().ft_vkx(ic0, b"".join(terms), len(terms), out)
    return bytes(out)


def verify_each_host(vkey, publics, proofs256):
    """csrc/zkwg_fexp_host.h with its stage on the host, under ZKWG_FQ29_CHECK -> (rc, message, verdicts, seconds, counts)"""
    k, ic, n_public = pairtest.key_bytes(vkey)
    n = len(proofs256)
    pub = b"".join(int(x).to_bytes(32, "little") for p in publics for x in p)
    ok, sec, cnt, err = (C.c_uint8 * max(1, n))(), (C.c_double * 6)(), (C.c_ulonglong * 4)(), C.create_string_buffer(256)
    rc = load().ft_verify_each(k, ic, n_public, n, b"".join(proofs256), pub, ok, sec, cnt, err, 256)
    return rc, err.value.decode(), [bool(v) for v in ok[:n]], list(sec), list(cnt)
