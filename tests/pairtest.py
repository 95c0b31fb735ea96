"""Test-only helpers of batched groth16 verification: the host build of csrc/zkwg_pair_core.h and csrc/zkwg_pair_host.h
(tests/native/pairtest.cpp) -- the Miller loop a lane pair of zk_pair_miller runs, the host pairing's pieces on 384-byte values, the batch
verifier with its leaves made on the host -- and proofs fabricated from the trapdoor of a toy key (oracle/pyref/groth16.py)."""
import ctypes as C

import nativelib
from oracle.pyref import groth16 as G

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
ONE = ((1 << 256) % Q).to_bytes(32, "little") + bytes(352)       # the 384 bytes of 1


def load():
    lib = nativelib.build("pairtest")
    u64, u32, vp = C.c_uint64, C.c_uint32, C.c_void_p
    lib.pt_violations.restype = C.c_ulonglong
    lib.pt_core_miller.restype = C.c_int
    lib.pt_core_miller.argtypes = [C.c_char_p, C.c_char_p, vp, vp]
    lib.pt_host_miller.restype = None
    lib.pt_host_miller.argtypes = [C.c_char_p, C.c_char_p, vp]
    lib.pt_final_exp.restype = None
    lib.pt_final_exp.argtypes = [C.c_char_p, vp]
    lib.pt_f12_mul.restype = None
    lib.pt_f12_mul.argtypes = [C.c_char_p, C.c_char_p, C.c_int, vp]
    lib.pt_pair_product.restype = None
    lib.pt_pair_product.argtypes = [C.c_char_p, C.c_char_p, u32, vp]
    lib.pt_pair_piece.restype = None
    lib.pt_pair_piece.argtypes = [C.c_int, C.c_char_p, vp]
    lib.pt_counters.restype = None
    lib.pt_counters.argtypes = [vp]
    lib.pt_verify_batch.restype = C.c_int
    lib.pt_verify_batch.argtypes = [C.c_char_p, C.c_char_p, u32, u64, C.c_char_p, C.c_char_p, C.c_char_p, vp, vp, vp, C.c_char_p, u64]
    return lib


def violations():
    return load().pt_violations()


def core_miller(g1, g2):
    """points in the zkey's form -> (the 384 bytes of the core's Miller value, inside the subgroup), or None when a point is off its curve"""
    out, inside = (C.c_uint8 * 384)(), C.c_uint8(9)
    rc = load().pt_core_miller(g1, g2, out, C.byref(inside))
    return (bytes(out), bool(inside.value)) if rc == 0 else None


def host_miller(g1, g2):
    """zk_pair_miller of csrc/zkwg_pairing.h; 1 when a point is at infinity (as zk_pairing_product skips the pair)"""
    if not any(g1) or not any(g2):
        return ONE
    out = (C.c_uint8 * 384)()
    load().pt_host_miller(g1, g2, out)
    return bytes(out)


def final_exp(f):
    out = (C.c_uint8 * 384)()
    load().pt_final_exp(f, out)
    return bytes(out)


def f12_mul(a, b, core=False):
    out = (C.c_uint8 * 384)()
    load().pt_f12_mul(a, b, 1 if core else 0, out)
    return bytes(out)


def counters():
    """(preconditions violated by the values, by the bounds, results above their own bounds) of csrc/zkwg_fq29.h in this library"""
    out = (C.c_ulonglong * 3)()
    load().pt_counters(out)
    return tuple(out)


def pair_product(values, use=None):
    """one level of the product tree as zk_pair_product runs it: 384-byte values, flags or None -> ceil(n / 4) values"""
    n = len(values)
    out = (C.c_uint8 * (384 * ((n + 3) // 4)))()
    load().pt_pair_product(b"".join(values), None if use is None else bytes(use), n, out)
    return [bytes(out[384 * j:384 * j + 384]) for j in range((n + 3) // 4)]


def pair_piece(op, words, n_out):
    """one piece of the Miller loop (tests/native/pairtest.cpp pt_pair_piece) on standard-form integers below q -> n_out integers"""
    out = (C.c_uint8 * (32 * n_out))()
    load().pt_pair_piece(op, b"".join(int(w).to_bytes(32, "little") for w in words), out)
    return [int.from_bytes(bytes(out[32 * i:32 * i + 32]), "little") for i in range(n_out)]


def f12_to_oracle(b):
    """the inverse of f12_from_oracle"""
    rinv = pow(1 << 256, -1, Q)
    v = [int.from_bytes(b[o:o + 32], "little") * rinv % Q for o in range(0, 384, 32)]
    return tuple((v[2 * k], v[2 * k + 1]) for k in range(6))


def f12_edge_family(seed):
    """Fq12 values at the edges of the limb form, as 384 stored bytes (Montgomery words): every word q - 1; every word 2^232 - 1 (all
    29-bit limbs of the split word are ones); every word 1; only c5 non-zero (the hi / xi path of a product alone); only c0 non-zero; and
    two random elements -> [(name, bytes)]"""
    import random
    rng = random.Random(seed)
    word = lambda v: int(v).to_bytes(32, "little")
    rnd2 = lambda: word(rng.randrange(Q)) + word(rng.randrange(Q))
    return [("q-1", word(Q - 1) * 12), ("2^232-1", word((1 << 232) - 1) * 12), ("1", word(1) * 12), ("c5", bytes(320) + rnd2()), ("c0", rnd2() + bytes(320)),
            ("random", b"".join(rnd2() for _ in range(6))), ("random2", b"".join(rnd2() for _ in range(6)))]


def f12_from_oracle(f):
    """the oracle's 6-tuple of Fq2 -> the 384 bytes of the host's Fq12 (Montgomery words)"""
    return b"".join(((v << 256) % Q).to_bytes(32, "little") for c in f for v in c)


def mont1(p):
    return bytes(64) if p is None else b"".join(((v << 256) % Q).to_bytes(32, "little") for v in p)


def mont2(p):
    return bytes(128) if p is None else b"".join(((v << 256) % Q).to_bytes(32, "little") for v in (p[0][0], p[0][1], p[1][0], p[1][1]))


# ---- toy keys and fabricated proofs -------------------------------------------------------------------------------------------------------
def toy_key(n_public, seed):
    """a key of known trapdoor over a system of one constraint (only alpha, beta, gamma, delta and the IC logarithms matter here)"""
    n_wires = n_public + 3
    cons = [({n_public + 1: 1}, {n_public + 2: 1}, {1: 1})]
    return G.setup(n_wires, n_public, cons, seed=seed)


def fabricate(key, publics, a, b, bad=False):
    """the logarithms (a, b, c) of a valid proof for `publics` under `key`: c = (a b - alpha beta - vkx gamma) / delta; bad: c + 1"""
    vkx = (key.ic[0] + sum(x * k for x, k in zip(publics, key.ic[1:]))) % R
    c = (a * b - key.alpha * key.beta - vkx * key.gamma) % R * pow(key.delta, R - 2, R) % R
    return a, b, (c + 1) % R if bad else c


def proof_json_from_logs(logs):
    return G.proof_json({"pi_a": logs[0], "pi_b": logs[1], "pi_c": logs[2]})


def proof_bytes_from_points(a, b, c):
    """oracle points -> the 256-byte form zkwg.prover writes"""
    vals = (a[0], a[1], b[0][0], b[0][1], b[1][0], b[1][1], c[0], c[1])
    return b"".join(v.to_bytes(32, "little") for v in vals)


def proof_bytes_from_mont(a64, b128, c64):
    """points in the zkey's form (as prover.fixed_base returns them) -> the 256-byte standard form"""
    rinv = pow(1 << 256, -1, Q)
    raw = a64 + b128 + c64
    return b"".join((int.from_bytes(raw[o:o + 32], "little") * rinv % Q).to_bytes(32, "little") for o in range(0, 256, 32))


def key_bytes(vkey):
    """a snarkjs verification key dict -> (alpha | beta | gamma | delta in the zkey's form, the IC points, n_public)"""
    from oracle.pyref import bn254_pairing as P
    k = mont1(P.g1_from_json(vkey["vk_alpha_1"])) + b"".join(mont2(P.g2_from_json(vkey[n])) for n in ("vk_beta_2", "vk_gamma_2", "vk_delta_2"))
    return k, b"".join(mont1(P.g1_from_json(v)) for v in vkey["IC"]), len(vkey["IC"]) - 1


def verify_batch_host(vkey, publics, proofs256, rand16):
    """csrc/zkwg_pair_host.h with the leaves made on the host, under ZKWG_FQ29_CHECK -> (rc, message, verdicts, seconds, counts)"""
    k, ic, n_public = key_bytes(vkey)
    n = len(proofs256)
    pub = b"".join(int(x).to_bytes(32, "little") for p in publics for x in p)
    ok, sec, cnt, err = (C.c_uint8 * max(1, n))(), (C.c_double * 6)(), (C.c_ulonglong * 4)(), C.create_string_buffer(256)
    rc = load().pt_verify_batch(k, ic, n_public, n, b"".join(proofs256), pub, rand16, ok, sec, cnt, err, 256)
    return rc, err.value.decode(), [bool(v) for v in ok[:n]], list(sec), list(cnt)
