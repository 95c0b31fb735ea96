"""snarkjs `.ptau` (powers of tau) reader / writer: the ceremony file `groth16 setup` takes its points from (reference workflow:
docs/zk-email-docs/UsageGuide/README.md:145-180, the prepared `powersOfTau28_hez_final_NN.ptau` files).

The container is not in the reference: the layout below is restated from snarkjs' published code (src/powersoftau_utils.js,
src/powersoftau_prepare_phase2.js) [EXT] and is UNPINNED until a real file is read -- as the `.zkey` container is (zkey.py).

    "ptau" | u32 version = 1 | u32 nSections | sections: u32 id, u64 size, payload
    1        u32 n8 (32), q | u32 power | u32 ceremonyPower
    2 .. 6   tau^k G1 (2^(power + 1) - 1 points) | tau^k G2 | alpha tau^k G1 | beta tau^k G1 (2^power each) | beta G2
    7        contributions
    12 - 15  the Lagrange forms of 2 - 5 ("prepared for phase 2"): levels q = 0 .. power back to back, level q starts at point
             2^q - 1; section 12 holds one level more, q = power + 1
Points: uncompressed affine, little-endian Montgomery words, x | y (G2: x.c0 | x.c1 | y.c0 | y.c1) -- the zkey's form, so slices of the
file are uploaded as they are.  alpha1 / beta1 of a key are the first points of sections 4 / 5, beta2 is section 6.

The C side (zkwg_ptau_parse, csrc/zkwg_setup_core.h) is what the set-up uses; this module is its Python twin for tools and tests, and the
writer makes a PREPARED file from point sections the caller supplies (a test's toy ceremony; it computes nothing)."""
import struct

from .zkey import Q

# (section id, bytes per point, points as a function of n = 2^power)
SECTIONS = ((2, 64, lambda n: 2 * n - 1), (3, 128, lambda n: n), (4, 64, lambda n: n), (5, 64, lambda n: n), (6, 128, lambda n: 1),
            (12, 64, lambda n: 4 * n - 1), (13, 128, lambda n: 2 * n - 1), (14, 64, lambda n: 2 * n - 1), (15, 64, lambda n: 2 * n - 1))
LAGRANGE = {12: "tau_g1", 13: "tau_g2", 14: "alpha_tau_g1", 15: "beta_tau_g1"}


def read_ptau(data):
    """data: bytes, memoryview or mmap -> dict: power, ceremony_power, sections = {id: (offset, size)}.  Sizes are checked before any
    point is touched; a file without sections 12 - 15 is refused ("Powers of tau is not prepared")."""
    if len(data) < 12 or bytes(data[:4]) != b"ptau":
        raise ValueError("not a .ptau file")
    version, nsec = struct.unpack_from("<II", data, 4)
    if version != 1:
        raise ValueError(f".ptau version {version} is not supported")
    pos, sec = 12, {}
    for _ in range(nsec):
        if pos + 12 > len(data):
            raise ValueError(".ptau: truncated section table")
        sid, size = struct.unpack_from("<IQ", data, pos)
        if pos + 12 + size > len(data):
            raise ValueError(f".ptau: section {sid} runs past the end of the file")
        sec[sid] = (pos + 12, size)
        pos += 12 + size
    if 1 not in sec or sec[1][1] != 44:
        raise ValueError(".ptau: header section missing or of the wrong size")
    o = sec[1][0]
    n8 = struct.unpack_from("<I", data, o)[0]
    if n8 != 32 or int.from_bytes(bytes(data[o + 4:o + 36]), "little") != Q:
        raise ValueError(".ptau: the prime is not the BN254 base field")
    power, ceremony = struct.unpack_from("<II", data, o + 36)
    if not 1 <= power <= 28:
        raise ValueError(".ptau: power out of range")
    n = 1 << power
    for sid, point, count in SECTIONS:
        if sid not in sec:
            raise ValueError("Powers of tau is not prepared" if sid >= 12 else f".ptau: section {sid} is missing")
    for sid, point, count in SECTIONS:
        if sec[sid][1] != point * count(n):
            raise ValueError(f".ptau: section {sid} holds {sec[sid][1]} bytes, expected {point * count(n)}")
    return {"power": power, "ceremony_power": ceremony, "sections": sec}


def level(data, info, sid, q):
    """the 2^q points of level q of Lagrange section sid (12 - 15), as a memoryview into data"""
    point = 128 if sid == 13 else 64
    if q > info["power"] + (1 if sid == 12 else 0):
        raise ValueError(f".ptau: the file (power {info['power']}) has no level {q}")
    o = info["sections"][sid][0] + ((1 << q) - 1) * point
    return memoryview(data)[o:o + (point << q)]


def slices(data, power):
    """what the set-up of a 2^power domain reads: dict tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1 (level power), tau_g1_next (level
    power + 1), alpha1, beta1, beta2 (bytes)"""
    info = read_ptau(data)
    if power > info["power"]:
        raise ValueError(f".ptau: the power of the file ({info['power']}) is too small for the circuit ({power})")
    out = {name: level(data, info, sid, power) for sid, name in LAGRANGE.items()}
    out["tau_g1_next"] = level(data, info, 12, power + 1)
    s = info["sections"]
    out["alpha1"] = bytes(data[s[4][0]:s[4][0] + 64])
    out["beta1"] = bytes(data[s[5][0]:s[5][0] + 64])
    out["beta2"] = bytes(data[s[6][0]:s[6][0] + 128])
    return out


def write_ptau(power, sections, ceremony_power=None, contributions=b""):
    """sections: {id: bytes} for ids 2 - 6 and, for a prepared file, 12 - 15 (whole sections, every level); sizes are asserted"""
    n = 1 << power
    for sid, point, count in SECTIONS:
        if sid in sections:
            assert len(sections[sid]) == point * count(n), (sid, len(sections[sid]), point * count(n))
    hdr = struct.pack("<I", 32) + Q.to_bytes(32, "little") + struct.pack("<II", power, power if ceremony_power is None else ceremony_power)
    secs = [(1, hdr)] + [(sid, bytes(sections[sid])) for sid in (2, 3, 4, 5, 6) if sid in sections] + [(7, contributions)]
    secs += [(sid, bytes(sections[sid])) for sid in (12, 13, 14, 15) if sid in sections]
    out = [b"ptau", struct.pack("<II", 1, len(secs))]
    for sid, payload in secs:
        out.append(struct.pack("<IQ", sid, len(payload)))
        out.append(payload)
    return b"".join(out)
