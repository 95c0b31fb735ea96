"""Test-only helpers of the prover of witnesses: the host build of csrc/zkwg_zkey_core.h (tests/native/zkeytest.cpp) and a seeded random
constraint system that is not an email circuit."""
import ctypes as C
import random

import nativelib

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def load():
    lib = nativelib.build("zkeytest")
    u64p = C.POINTER(C.c_uint64)
    lib.zt_violations.restype = C.c_ulonglong
    lib.zt_zkey_check.restype = C.c_int
    lib.zt_zkey_check.argtypes = [C.c_char_p, C.c_uint64, u64p]
    lib.zt_wtns_parse.restype = C.c_int
    lib.zt_wtns_parse.argtypes = [C.c_char_p, C.c_uint64, u64p, u64p]
    lib.zt_abc.restype = C.c_int
    lib.zt_abc.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]
    lib.zt_range_ok.restype = C.c_int
    lib.zt_range_ok.argtypes = [C.c_char_p, C.c_uint64]
    lib.zt_max_row.restype = C.c_uint
    lib.zt_long_threshold.restype = C.c_uint
    return lib


def wit_bytes(w):
    return b"".join(int(x).to_bytes(32, "little") for x in w)


def section4(cons, n_public):
    """[(matrix, row, wire, coefficient)] of a zkey's section 4: the rows of A and B, then the nPublic + 1 rows snarkjs appends to A"""
    out = [(m, j, w, v % R) for j, row in enumerate(cons) for m in (0, 1) for w, v in row[m].items() if v % R]
    return out + [(0, len(cons) + s, s, 1) for s in range(n_public + 1)]


def random_system(seed, n_in=4400, n_public=5, a_lengths=(1, 2, 62, 63, 64, 65, 100, 700, 4096, 4300), n_random=260):
    """-> (n_wires, cons, w): every constraint k defines a fresh wire w_k = (A_k . w)(B_k . w) over earlier wires, so w satisfies the
    system.  Coefficients from {1, r - 1, small, uniform}, input values from {0, 1, bytes, uniform}; A rows of the given lengths (B rows
    of 1 .. 3 terms beside them) and n_random constraints of 1 .. 40 terms a side."""
    rng = random.Random(seed)
    val = lambda: rng.choice([0, 0, 1, 1, rng.randrange(256), rng.randrange(R)])
    coef = lambda: rng.choice([1, 1, 1, R - 1, R - 1, rng.randrange(2, 1000), rng.randrange(2, R - 1)])
    w = [1] + [val() for _ in range(n_in - 1)]
    cons = []
    shapes = [(la, rng.randrange(1, 4)) for la in a_lengths] + [(rng.randrange(1, 41), rng.randrange(1, 41)) for _ in range(n_random)]
    rng.shuffle(shapes)
    for la, lb in shapes:
        n = len(w)
        ra = {i: coef() for i in rng.sample(range(n), la)}
        rb = {i: coef() for i in rng.sample(range(n), lb)}
        a = sum(v * w[i] for i, v in ra.items()) % R
        b = sum(v * w[i] for i, v in rb.items()) % R
        cons.append((ra, rb, {n: 1}))
        w.append(a * b % R)
    return len(w), cons, w


def dummy_zkey(n_wires, n_public, domain, coeffs):
    """a groth16 .zkey with the given section 4 whose points are all at infinity (the readers and the row evaluation never look at them)"""
    from zkwg import zkey
    pts = {"alpha1": bytes(64), "beta1": bytes(64), "beta2": bytes(128), "gamma2": bytes(128), "delta1": bytes(64), "delta2": bytes(128)}
    return zkey.write_zkey(n_wires, n_public, domain, pts, bytes(64 * (n_public + 1)), bytes(64 * n_wires), bytes(64 * n_wires), bytes(128 * n_wires),
                           bytes(64 * (n_wires - n_public - 1)), bytes(64 * domain), coeffs)


class StubKey:
    """what oracle.pyref.groth16.abc_rows reads of a key"""

    def __init__(self, n_public, n):
        self.n_public, self.n = n_public, n


def abc_ints(raw, n_rows):
    """one record A.w | B.w | C.w of Montgomery-form values -> three lists of standard-form integers"""
    rinv = pow(1 << 256, -1, R)
    v = [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(3 * n_rows)]
    assert all(x < R for x in v), "a value is not canonical"
    v = [x * rinv % R for x in v]
    return v[:n_rows], v[n_rows:2 * n_rows], v[2 * n_rows:]
