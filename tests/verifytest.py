"""Test-only helpers of `powersoftau verify`: the host build of csrc/zkwg_verify_core.h and csrc/zkwg_pairing.h
(tests/native/verifytest.cpp) -- the G2 subgroup test as a lane pair of the kernel runs it and the pairing product -- and the twist points
outside the subgroup that the subgroup tests share."""
import ctypes as C

import nativelib

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
COFACTOR = 2 * Q - R                       # of the twist: 10069 x 5864401 x (a large factor)
SMALL = (10069, 5864401, 10069 * 5864401)


def load():
    lib = nativelib.build("verifytest")
    u64, u32 = C.c_uint64, C.c_uint32
    lib.vt_violations.restype = C.c_ulonglong
    lib.vt_u_digits.restype = None
    lib.vt_u_digits.argtypes = [C.POINTER(u32), C.POINTER(u32)]
    lib.vt_g2_subgroup.restype = C.c_int
    lib.vt_g2_subgroup.argtypes = [C.c_char_p, u64, C.c_void_p]
    lib.vt_pairing.restype = C.c_int
    lib.vt_pairing.argtypes = [C.c_char_p, C.c_char_p, u32, C.c_void_p, C.c_char_p, u64]
    lib.vt_pairing_check.restype = C.c_int
    lib.vt_pairing_check.argtypes = [C.c_char_p, C.c_char_p, u32, C.POINTER(C.c_int), C.c_char_p, u64]
    lib.vt_rlc.restype = C.c_int
    lib.vt_rlc.argtypes = [C.c_int, C.c_char_p, u64, C.c_char_p, u32, C.c_void_p]
    return lib


def violations():
    return load().vt_violations()


def u_digits():
    """-> (positions, non-zero digits) of the non-adjacent form of u that every lane walks"""
    a, b = C.c_uint32(), C.c_uint32()
    load().vt_u_digits(C.byref(a), C.byref(b))
    return a.value, b.value


def g2_subgroup(points):
    """128-byte points in the zkey's form -> [bool per point: inside the subgroup], or None when a point is not on the curve"""
    n = len(points) // 128
    out = (C.c_uint8 * max(1, n))()
    rc = load().vt_g2_subgroup(bytes(points), n, out)
    return [bool(v) for v in out[:n]] if rc == 0 else None


def pairing(pairs):
    """[(64-byte G1, 128-byte G2)] -> (rc, message, the product of the reduced pairings as the oracle's 6-tuple of Fq2 or None)"""
    g1, g2 = b"".join(p for p, _ in pairs), b"".join(q for _, q in pairs)
    out, err = (C.c_uint8 * 384)(), C.create_string_buffer(256)
    rc = load().vt_pairing(g1, g2, len(pairs), out, err, 256)
    b = bytes(out)
    val = tuple((int.from_bytes(b[64 * k:64 * k + 32], "little"), int.from_bytes(b[64 * k + 32:64 * k + 64], "little")) for k in range(6))
    return rc, err.value.decode(), (val if rc == 0 else None)


def pairing_check(pairs):
    """-> (rc, message, whether the product is 1)"""
    g1, g2 = b"".join(p for p, _ in pairs), b"".join(q for _, q in pairs)
    one, err = C.c_int(-1), C.create_string_buffer(256)
    rc = load().vt_pairing_check(g1, g2, len(pairs), C.byref(one), err, 256)
    return rc, err.value.decode(), (bool(one.value) if rc == 0 else None)


def rlc(group, points, scalars, scalar_bytes=16):
    """sum_i s_i P_i on the host (points and scalars as bytes) -> the point in the zkey's form, or None when a point is not on its curve"""
    pt = 64 if group == 1 else 128
    n = len(points) // pt
    assert len(points) == n * pt and len(scalars) == n * scalar_bytes
    out = (C.c_uint8 * pt)()
    rc = load().vt_rlc(group, bytes(points), n, bytes(scalars), scalar_bytes, out)
    return bytes(out) if rc == 0 else None


class HostBackend:
    """zkwg.ptau._Device on the host: bytes for tensors, the host sums and the host build of the subgroup test for the device calls"""

    def upload(self, data):
        return bytes(data)

    def g2_subgroup(self, points, n):
        from zkwg import ptau
        inside = g2_subgroup(points[:128 * n])
        if inside is None:
            raise ptau.PtauError("a point is not on its curve (or not reduced)")
        bad = [i for i, ok in enumerate(inside) if not ok]
        return len(bad), (bad[0] if bad else None)

    def rlc(self, group, points, first, n, scalars, wide=False, shifted=False, piece=0):
        from zkwg import ptau
        pt, sb = (64 if group == 1 else 128), (32 if wide else 16)
        out = [rlc(group, points[(first + k) * pt:(first + k + n) * pt], scalars[:n * sb], sb) for k in range(2 if shifted else 1)]
        if None in out:
            raise ptau.PtauError("a point is not on its curve (or not reduced)")
        return out[0], (out[1] if shifted else None)

    def ifft(self, scalars16, q):
        from oracle.pyref import ntt
        vals = [int.from_bytes(scalars16[16 * j:16 * j + 16], "little") for j in range(1 << q)]
        return b"".join(v.to_bytes(32, "little") for v in ntt.ifft_fast(vals))


# ---- twist points outside the subgroup (oracle integers) ----------------------------------------------------------------------------------
def plain_mul(k, p):
    """k p by double-and-add WITHOUT reducing k modulo r (oracle.pyref.bn254_g2.mul reduces: useless for r itself and for cofactor parts)"""
    from oracle.pyref import bn254_g2 as G2
    acc = None
    while k:
        if k & 1:
            acc = G2.add(acc, p)
        p = G2.add(p, p)
        k >>= 1
    return acc


def f2_sqrt(a):
    """a square root of a in Fq2 (q = 3 mod 4), or None"""
    from oracle.pyref.bn254_g2 import f2_mul
    from oracle.pyref.bn254_pairing import f2_pow
    if a == (0, 0):
        return a
    a1 = f2_pow(a, (Q - 3) // 4)
    alpha = f2_mul(a1, f2_mul(a1, a))
    x0 = f2_mul(a1, a)
    if alpha == (Q - 1, 0):
        r = (-x0[1] % Q, x0[0])                                 # i x0
    else:
        b = f2_pow(((1 + alpha[0]) % Q, alpha[1]), (Q - 1) // 2)
        r = f2_mul(b, x0)
    return r if f2_mul(r, r) == a else None


def twist_points(n, seed):
    """n points of the twist by try-and-increment, the cofactor NOT cleared: outside the subgroup (probability 1 - 1 / cofactor)"""
    import random
    from oracle.pyref import bn254_g2 as G2
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        x = (rng.randrange(Q), rng.randrange(Q))
        while True:
            y = f2_sqrt(G2.f2_add(G2.f2_mul(G2.f2_mul(x, x), x), G2.B2))
            if y is not None:
                break
            x = ((x[0] + 1) % Q, x[1])
        out.append((x, y))
    return out


def small_order_points(p):
    """for a raw twist point p: its multiples of order dividing 10069, 5864401 and their product"""
    return [plain_mul(R * (COFACTOR // m), p) for m in SMALL]


# ---- tampering with a .ptau (shared by the CPU and the GPU tests of zkwg.ptau.verify) ------------------------------------------------------
def _mont2(p):
    return bytes(128) if p is None else b"".join(((v << 256) % Q).to_bytes(32, "little") for v in (p[0][0], p[0][1], p[1][0], p[1][1]))


def reseal(data):
    """the last record's next_challenge recomputed over the sections as they now are"""
    from zkwg import ptau
    info = ptau.read_any(data)[0]
    recs = ptau.read_contributions(data)
    before = recs[-2]["next_challenge"] if len(recs) > 1 else ptau.new_challenge(info["ceremony_power"])
    last = dict(recs[-1])
    last["next_challenge"] = ptau._points_hash(data, info, before)
    return with_records(data, [r["raw"] for r in recs[:-1]] + [ptau.pack_record(last)])


def with_records(data, raw_records):
    from zkwg import ptau
    o, size = ptau.read_any(data)[0]["sections"][7]
    s7 = ptau.pack_section7(raw_records)
    assert len(s7) == size
    return bytes(data[:o]) + s7 + bytes(data[o + size:])


def swap_points(data, sid, i, j, first=0):
    from zkwg import ptau
    o = ptau.read_any(data)[0]["sections"][sid][0]
    pt = 128 if sid in (3, 6, 13) else 64
    b = bytearray(data)
    a, c = o + (first + i) * pt, o + (first + j) * pt
    b[a:a + pt], b[c:c + pt] = data[c:c + pt], data[a:a + pt]
    assert bytes(b) != bytes(data)
    return bytes(b)


def decode_g2(b):
    v = [int.from_bytes(b[i:i + 32], "little") * pow(1 << 256, -1, Q) % Q for i in (0, 32, 64, 96)]
    return None if not any(b) else ((v[0], v[1]), (v[2], v[3]))


def map_g2(data, sid, k, f):
    from zkwg import ptau
    o = ptau.read_any(data)[0]["sections"][sid][0] + 128 * k
    return bytes(data[:o]) + _mont2(f(decode_g2(data[o:o + 128]))) + bytes(data[o + 128:])
