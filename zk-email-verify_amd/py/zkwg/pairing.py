"""The BN254 pairing as a CHECK: is a product of pairings 1?  (zkwg_pairing_check, csrc/zkwg_pairing.h: optimal ate on the host, one
Miller loop per pair and one final exponentiation per call.)  What `python -m zkwg.ptau verify` decides its ratio checks with; the
millions of points in front of a check are folded into its four points on the device (zkwg.ptau.rlc).

Points are bytes in the zkey's form: G1 64 bytes, G2 128 bytes, little-endian Montgomery words, zeros = infinity."""
import ctypes as C

from . import _call
from .zkey import Q


class PairingError(ValueError):
    pass


def check(pairs):
    """[(G1 bytes, G2 bytes)] -> prod e(g1, g2) == 1.  A pair with a point at infinity contributes 1.  PairingError: a point is not
    reduced or not on its curve ("curve"), a G2 point is outside the subgroup of order r ("subgroup")"""
    from . import _lib
    lib = _lib.load()
    g1, g2 = b"".join(bytes(p) for p, _ in pairs), b"".join(bytes(q) for _, q in pairs)
    if len(g1) != 64 * len(pairs) or len(g2) != 128 * len(pairs):
        raise PairingError("a G1 point is 64 bytes and a G2 point 128")
    one = C.c_int(0)
    _call.check(lib, lib.zkwg_pairing_check(g1, g2, len(pairs), C.byref(one)), PairingError)
    return bool(one.value)


def neg_g1(p):
    """-p for a G1 point in the zkey's form"""
    p = bytes(p)
    y = int.from_bytes(p[32:64], "little")
    return p[:32] + ((Q - y) % Q).to_bytes(32, "little")


def same_ratio(a, b, c, d):
    """a, b in G1 and c, d in G2: is b = x a and d = x c for one x?  e(a, d) e(-b, c) == 1.  False when ANY of the four is infinity (an
    all-infinity section would otherwise pass every ratio check)"""
    if not (any(a) and any(b) and any(c) and any(d)):
        return False
    return check([(a, d), (neg_g1(b), c)])
