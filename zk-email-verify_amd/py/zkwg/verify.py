"""python -m zkwg.verify verification_key.json public.json proof.json [--device D] [--each]
-- `snarkjs groth16 verify` (reference: packages/helpers/src/chunked-zkey.ts:93-101, snarkjs.groth16.verify(vkey, publicSignals, proof)):
prints OK / INVALID and exits 0 / 1.  public.json and proof.json may also be JSON lists of equal length (a batch): one line per proof,
exit 1 if any is invalid.

verify_batch checks MANY proofs of one key with one Miller loop per proof on the device and one final exponentiation on the host
(zkwg_groth16_verify_batch, include/zkwg.h "checking proofs": the batch equation, the per-proof rejections and the bisection that finds
the bad proofs of a failing batch are stated there and in csrc/zkwg_pair_host.h).  device = -1 runs the same algorithm on the host alone.

verify_each (--each) gives the verdict of every proof on its own: three Miller loops and one final exponentiation per proof, all on the
device (zkwg_groth16_verify_each), no randomness and no bisection -- its work does not depend on how many proofs are bad, which is what
a verifier of proofs from strangers needs; verify_batch is the faster call while (nearly) every proof is good.

A malformed argument (wrong lengths, nPublic != len(IC) - 1, a z coordinate that is not 1, not a BN254 groth16 key) raises VerifyError; a
well-formed but wrong proof gives False.  The key's vk_alphabeta_12 is ignored: e(alpha, beta) is one of the pairs of the product."""
import argparse
import ctypes as C
import json
import sys

from . import _call
from .zkey import Q


class VerifyError(Exception):
    pass


class _Key(C.Structure):
    _fields_ = [("n_public", C.c_uint32), ("alpha1", C.c_uint8 * 64), ("beta2", C.c_uint8 * 128), ("gamma2", C.c_uint8 * 128),
                ("delta2", C.c_uint8 * 128), ("ic", C.c_void_p)]


def _int(v, what):
    try:
        x = int(v)
    except (TypeError, ValueError):
        raise VerifyError(f"{what}: not an integer") from None
    if x < 0 or x >> 256:
        raise VerifyError(f"{what}: outside 0 .. 2^256 - 1")
    return x


def _g1(v, what):
    """a snarkjs G1 point [x, y, "1"] -> (x, y) as integers"""
    if not isinstance(v, (list, tuple)) or len(v) != 3 or _int(v[2], what) != 1:
        raise VerifyError(f"{what}: expected [x, y, 1]")
    return _int(v[0], what), _int(v[1], what)


def _g2(v, what):
    """a snarkjs G2 point [[x0, x1], [y0, y1], ["1", "0"]] -> (x0, x1, y0, y1)"""
    if not isinstance(v, (list, tuple)) or len(v) != 3 or any(not isinstance(c, (list, tuple)) or len(c) != 2 for c in v) \
            or (_int(v[2][0], what), _int(v[2][1], what)) != (1, 0):
        raise VerifyError(f"{what}: expected [[x0, x1], [y0, y1], [1, 0]]")
    return tuple(_int(c, what) for c in (v[0][0], v[0][1], v[1][0], v[1][1]))


def _mont(coords, what):
    """coordinates of the KEY in the zkey's form; one at or above q is refused (a key is never turned into verdicts)"""
    if any(c >= Q for c in coords):
        raise VerifyError(f"{what}: a coordinate is not below q")
    return b"".join(_call.mont(c) for c in coords)


def _key(vkey):
    if not isinstance(vkey, dict) or any(k not in vkey for k in ("nPublic", "vk_alpha_1", "vk_beta_2", "vk_gamma_2", "vk_delta_2", "IC")):
        raise VerifyError("verification key: not a snarkjs verification_key.json")
    if vkey.get("protocol", "groth16") != "groth16" or vkey.get("curve", "bn128") not in ("bn128", "bn254"):
        raise VerifyError("verification key: not a BN254 groth16 key")
    n_public = _int(vkey["nPublic"], "nPublic")
    if not isinstance(vkey["IC"], list) or n_public != len(vkey["IC"]) - 1:
        raise VerifyError("verification key: nPublic is not len(IC) - 1")
    k = _Key()
    k.n_public = n_public
    for field, name, conv in (("alpha1", "vk_alpha_1", _g1), ("beta2", "vk_beta_2", _g2), ("gamma2", "vk_gamma_2", _g2), ("delta2", "vk_delta_2", _g2)):
        raw = _mont(conv(vkey[name], name), name)
        C.memmove(getattr(k, field), raw, len(raw))
    ic = C.create_string_buffer(b"".join(_mont(_g1(p, f"IC[{i}]"), f"IC[{i}]") for i, p in enumerate(vkey["IC"])), 64 * (n_public + 1))
    k.ic = C.cast(ic, C.c_void_p)
    return k, ic, n_public


def proof_bytes(proof):
    """a snarkjs proof.json dict (or the 256-byte form itself) -> pi_a | pi_b | pi_c, standard form, little-endian"""
    if isinstance(proof, (bytes, bytearray, memoryview)):
        if len(proof) != 256:
            raise VerifyError("proof: the byte form has 256 bytes")
        return bytes(proof)
    if not isinstance(proof, dict) or any(k not in proof for k in ("pi_a", "pi_b", "pi_c")):
        raise VerifyError("proof: not a snarkjs proof.json")
    vals = _g1(proof["pi_a"], "pi_a") + _g2(proof["pi_b"], "pi_b") + _g1(proof["pi_c"], "pi_c")
    return b"".join(v.to_bytes(32, "little") for v in vals)


def _arguments(vkey, publics, proofs):
    """-> (key, the buffer its ic points into, n, the proofs' bytes, the public inputs' bytes)"""
    key, ic, n_public = _key(vkey)
    n = len(proofs)
    if len(publics) != n:
        raise VerifyError("as many lists of public inputs as proofs are expected")
    if any(not isinstance(p, (list, tuple)) or len(p) != n_public for p in publics):
        raise VerifyError(f"every proof needs {n_public} public inputs")
    raw = b"".join(proof_bytes(p) for p in proofs)
    pub = b"".join(_int(x, "public input").to_bytes(32, "little") for p in publics for x in p)
    return key, ic, n, raw, pub


def verify_batch(vkey, publics, proofs, device=0, rand=None):
    """-> [bool per proof].  vkey: a snarkjs verification_key.json dict; publics: per proof a list of decimal strings or integers;
    proofs: snarkjs proof.json dicts or the 256-byte form zkwg.prover writes; device: the GPU, or -1 for the host alone; rand: per proof
    16 bytes, none of them all zero (tests; None draws them from the operating system inside the call)"""
    from . import _lib
    lib = _lib.load()
    key, ic, n, raw, pub = _arguments(vkey, publics, proofs)
    if rand is not None and len(rand) != 16 * n:
        raise VerifyError("rand: 16 bytes per proof")
    ok = (C.c_uint8 * max(1, n))()
    rc = lib.zkwg_groth16_verify_batch(device, C.byref(key), n, raw, pub, None if rand is None else bytes(rand), ok)
    del ic
    _call.check(lib, rc, VerifyError)
    return [bool(v) for v in ok[:n]]


def verify_each(vkey, publics, proofs, device=0):
    """-> [bool per proof], every proof checked on its own (zkwg_groth16_verify_each): the arguments of verify_batch without rand.  The
    work is three Miller loops and one final exponentiation per proof, whatever share of the proofs is bad."""
    from . import _lib
    lib = _lib.load()
    key, ic, n, raw, pub = _arguments(vkey, publics, proofs)
    ok = (C.c_uint8 * max(1, n))()
    rc = lib.zkwg_groth16_verify_each(device, C.byref(key), n, raw, pub, ok)
    del ic
    _call.check(lib, rc, VerifyError)
    return [bool(v) for v in ok[:n]]


def verify(vkey, public, proof, device=-1):
    """one proof -> bool (the host alone by default: one proof does not fill a device)"""
    return verify_batch(vkey, [public], [proof], device=device)[0]


def stats():
    """-> (seconds[6], counts[4]) of this thread's last verify_batch (zkwg_groth16_verify_stats)"""
    from . import _lib
    sec, cnt = (C.c_double * 6)(), (C.c_uint64 * 4)()
    _lib.load().zkwg_groth16_verify_stats(sec, cnt)
    return list(sec), list(cnt)


def stats_each():
    """-> (seconds[6], counts[4]) of this thread's last verify_each (zkwg_groth16_verify_each_stats)"""
    from . import _lib
    sec, cnt = (C.c_double * 6)(), (C.c_uint64 * 4)()
    _lib.load().zkwg_groth16_verify_each_stats(sec, cnt)
    return list(sec), list(cnt)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m zkwg.verify", description="snarkjs groth16 verify")
    ap.add_argument("vkey")
    ap.add_argument("public")
    ap.add_argument("proof")
    ap.add_argument("--device", type=int, default=-1, help="the GPU that runs the Miller loops; -1 (default): the host alone")
    ap.add_argument("--each", action="store_true", help="check every proof on its own (verify_each): no batch equation, no bisection")
    a = ap.parse_args(argv)
    try:
        vkey, public, proof = (json.load(open(f)) for f in (a.vkey, a.public, a.proof))
        batch = isinstance(proof, list)
        if not isinstance(public, list):
            raise VerifyError("public.json: a list is expected")
        good = (verify_each if a.each else verify_batch)(vkey, public if batch else [public], proof if batch else [proof], device=a.device)
    except (VerifyError, OSError, ValueError) as e:
        print(f"zkwg.verify: {e}", file=sys.stderr)
        return 2
    for g in good:
        print("OK" if g else "INVALID")
    return 0 if all(good) else 1


if __name__ == "__main__":
    sys.exit(main())
