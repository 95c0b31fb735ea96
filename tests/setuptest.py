"""Test-only helpers of the groth16 set-up: the host build of csrc/zkwg_setup_core.h (tests/native/setuptest.cpp), a seeded constraint
system with every class of coefficient in all three matrices, a toy powers-of-tau ceremony from a known (tau, alpha, beta), and the key
oracle/pyref/groth16.py makes from the same trapdoor with gamma = delta = 1 -- which a set-up from those powers must equal byte for byte."""
import ctypes as C
import random

import nativelib

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583


def load():
    from zkwg._lib import SetupSlices
    lib = nativelib.build("setuptest")
    u64p = C.POINTER(C.c_uint64)
    lib.st_violations.restype = C.c_ulonglong
    lib.st_ptau_parse.restype = C.c_int
    lib.st_ptau_parse.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, u64p, C.c_char_p, C.c_char_p, C.c_uint64]
    lib.st_zkey_new_size.restype = C.c_int
    lib.st_zkey_new_size.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_uint32), u64p, C.c_char_p, C.c_uint64]
    lib.st_zkey_new.restype = C.c_int
    lib.st_zkey_new.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(SetupSlices), C.c_void_p, C.c_uint64, u64p, u64p, C.c_char_p, C.c_uint64]
    lib.st_fixed_base.restype = None
    lib.st_fixed_base.argtypes = [C.c_int, C.c_char_p, C.c_uint64, C.c_void_p]
    lib.st_long_threshold.restype = C.c_uint
    lib.st_chunk.restype = C.c_uint
    return lib


def host_points(group, scalars):
    """[k G] for the group's generator as the zkey stores them (64 / 128 bytes a point), by the host multiply"""
    lib = load()
    out = (C.c_uint8 * ((64 if group == 1 else 128) * len(scalars)))()
    lib.st_fixed_base(group, b"".join(int(k % R).to_bytes(32, "little") for k in scalars), len(scalars), out)
    return bytes(out)


def mont1(p):
    return bytes(64) if p is None else ((p[0] << 256) % Q).to_bytes(32, "little") + ((p[1] << 256) % Q).to_bytes(32, "little")


def mont2(p):
    return bytes(128) if p is None else b"".join(((v << 256) % Q).to_bytes(32, "little") for v in (p[0][0], p[0][1], p[1][0], p[1][1]))


def host_ptau_parse(data, power):
    """-> (rc, message, offsets of the five slices, alpha1 | beta1 | beta2)"""
    lib = load()
    off, pts, err = (C.c_uint64 * 5)(), C.create_string_buffer(256), C.create_string_buffer(256)
    rc = lib.st_ptau_parse(bytes(data), len(data), power, off, pts, err, 256)
    return rc, err.value.decode(), list(off), pts.raw


def host_new_zkey(r1cs, slices):
    """the set-up on the CPU -> (rc, message, zkey bytes or None, info)"""
    from zkwg._lib import SetupSlices
    lib = load()
    power, size, err = C.c_uint32(), C.c_uint64(), C.create_string_buffer(256)
    rc = lib.st_zkey_new_size(r1cs, len(r1cs), C.byref(power), C.byref(size), err, 256)
    if rc != 0:
        return rc, err.value.decode(), None, None
    sl = SetupSlices()
    sl.power, sl.on_device = slices["power"], 0
    keep = []
    for k in ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "tau_g1_next"):
        buf = C.create_string_buffer(bytes(slices[k]), len(slices[k]))
        keep.append(buf)
        setattr(sl, k, C.addressof(buf))
    for k in ("alpha1", "beta1", "beta2"):
        C.memmove(getattr(sl, k), slices[k], len(slices[k]))
    out, out_len, info = (C.c_uint8 * size.value)(), C.c_uint64(), (C.c_uint64 * 7)()
    rc = lib.st_zkey_new(r1cs, len(r1cs), C.byref(sl), out, size.value, C.byref(out_len), info, err, 256)
    return rc, err.value.decode(), (bytes(out[:out_len.value]) if rc == 0 else None), list(info)


def coefficient(rng):
    """one of {1, r - 1, small, 2^k, r - 2^k, uniform}"""
    k = rng.randrange(1, 253)
    return rng.choice([1, 1, R - 1, R - 1, rng.randrange(2, 1000), 1 << k, R - (1 << k), rng.randrange(2, R - 1)])


def system(seed, n_in, n_public, n_cons, heavy=(), degrees=(), max_terms=4):
    """-> (n_wires, cons, w).  Constraint k defines the fresh wire n_in + k as (A.w)(B.w) / v, v its coefficient in C, so w satisfies the
    system; C rows carry further terms over earlier wires (the fresh wire's value absorbs them).  Every matrix draws coefficients from
    `coefficient`.  heavy: {wire: (count, matrices)} -- the wire is put into one of the named matrices (0 / 1 / 2, in turn) of that many constraints; degrees: [(wire, d)] --
    the wire occurs in exactly d rows of A (and nowhere else, if it is an input wire the random rows never pick: pass wires >= n_in - len)."""
    rng = random.Random(seed)
    reserved = {wr for wr, _ in degrees}
    pool = [i for i in range(n_in) if i not in reserved]
    w = [1] + [rng.choice([0, 1, rng.randrange(256), rng.randrange(R)]) for _ in range(n_in - 1)]
    rows = []
    for k in range(n_cons):
        n = n_in + k
        cand = pool + list(range(n_in, n))
        rows.append([{i: coefficient(rng) for i in rng.sample(cand, rng.randrange(1, max_terms + 1))} for _ in range(3)])
    for wr, (count, matrices) in dict(heavy).items():
        for t, k in enumerate(rng.sample(range(n_cons), count)):
            rows[k][matrices[t % len(matrices)]][wr] = coefficient(rng)
    for wr, d in degrees:
        for k in rng.sample(range(n_cons), d):
            rows[k][0][wr] = coefficient(rng)
    cons = []
    for k, (ra, rb, rc) in enumerate(rows):
        n = n_in + k
        a = sum(v * w[i] for i, v in ra.items()) % R
        b = sum(v * w[i] for i, v in rb.items()) % R
        rest = sum(v * w[i] for i, v in rc.items()) % R
        v = coefficient(rng)
        rc[n] = v
        w.append((a * b - rest) * pow(v, -1, R) % R)
        cons.append((ra, rb, rc))
    return n_in + n_cons, cons, w


def wire_degree(cons, wire):
    return sum(1 for row in cons for m in row if wire in m)


def satisfied(cons, w):
    ev = lambda d: sum(v * w[i] for i, v in d.items()) % R
    return all(ev(a) * ev(b) % R == ev(c) for a, b, c in cons)


def toy_key(n_wires, n_public, cons, seed):
    """oracle.pyref.groth16.setup with gamma = delta = 1: the key a set-up from the powers of (tau, alpha, beta) must produce"""
    from oracle.pyref import groth16 as G
    key = G.setup(n_wires, n_public, cons, seed=seed)
    key.c_key = [x * key.delta % R for x in key.c_key]
    key.h_key = [x * key.delta % R for x in key.h_key]
    key.ic = [x * key.gamma % R for x in key.ic]
    key.delta = key.gamma = 1
    return key


def toy_slice_scalars(key):
    """the discrete logarithms of the five slices of the key's trapdoor: Lagrange values of level p (times 1, alpha, beta) and p + 1"""
    from oracle.pyref import groth16 as G
    lag = key.lag
    nxt = G.lagrange_at(key.tau, key.power + 1)
    return {"tau": lag, "alpha_tau": [x * key.alpha % R for x in lag], "beta_tau": [x * key.beta % R for x in lag], "next": nxt}


def toy_slices(key, points):
    """points(group, scalars) -> bytes.  -> the dict zkwg.setup.new_zkey / host_new_zkey take"""
    s = toy_slice_scalars(key)
    return {"power": key.power, "tau_g1": points(1, s["tau"]), "tau_g2": points(2, s["tau"]), "alpha_tau_g1": points(1, s["alpha_tau"]),
            "beta_tau_g1": points(1, s["beta_tau"]), "tau_g1_next": points(1, s["next"]),
            "alpha1": points(1, [key.alpha]), "beta1": points(1, [key.beta]), "beta2": points(2, [key.beta])}


def toy_sections(key, points):
    """the point sections and header points of the key's .zkey: {3, 5, 6, 7, 8, 9: bytes, 'alpha1', 'beta1', 'beta2', 'gamma2', 'delta1', 'delta2'}"""
    np1 = key.n_public + 1
    return {3: points(1, key.ic), 5: points(1, key.a_tau), 6: points(1, key.b_tau), 7: points(2, key.b_tau), 8: points(1, key.c_key[np1:]),
            9: points(1, key.h_key), "alpha1": points(1, [key.alpha]), "beta1": points(1, [key.beta]), "beta2": points(2, [key.beta]),
            "gamma2": points(2, [1]), "delta1": points(1, [1]), "delta2": points(2, [1])}


def zkey_sections(z):
    """the same dict read from a .zkey (zkwg.zkey.read_zkey)"""
    from zkwg import zkey
    d = zkey.read_zkey(z)
    out = {3: d["ic"], 5: d["a"], 6: d["b1"], 7: d["b2"], 8: d["c"], 9: d["h"]}
    out.update({k: d[k] for k in ("alpha1", "beta1", "beta2", "gamma2", "delta1", "delta2")})
    return out, d
