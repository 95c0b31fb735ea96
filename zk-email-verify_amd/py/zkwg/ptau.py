"""python -m zkwg.ptau new POWER out.ptau
python -m zkwg.ptau contribute in.ptau out.ptau --name N [--entropy E] [--device D]
python -m zkwg.ptau beacon in.ptau out.ptau HASHHEX EXP --name N [--device D]
python -m zkwg.ptau prepare in.ptau out.ptau [--power P] [--device D]
python -m zkwg.ptau info file.ptau
-- snarkjs `.ptau` (powers of tau) reader / writer and `snarkjs powersoftau prepare phase2` on the device: the ceremony file `groth16 setup` takes its points from (reference workflow:
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

The C side (zkwg_ptau_parse, csrc/zkwg_setup_core.h) is what the set-up uses; this module is its Python twin for tools and tests.  The
writer makes a file from point sections the caller supplies (a test's toy ceremony; it computes nothing); `prepare` computes sections
12 - 15 of an unprepared file on the device (zkwg_ptau_prepare, csrc/zkwg_ptau_core.h: per level the inverse Fourier transform over the
points of the prefix; the extra level of section 12 over the 2 n - 1 powers and one point at infinity), `truncate` cuts an unprepared
file to a smaller power on the host.

THE CEREMONY ITSELF (`powersoftau new` / `contribute` / `beacon`).  `new` writes the generators (tau = alpha = beta = 1) and an empty
section 7; it needs no device.  A contribution with secrets (tau, alpha, beta) multiplies point k of sections 2 and 3 by tau^k, of
section 4 by alpha tau^k, of section 5 by beta tau^k and section 6 by beta -- every point by its own scalar, computed per lane on the
device (zkwg_ptau_apply_key, csrc/zkwg_ptau_key_core.h) -- and appends a record to section 7.  The secrets are
zkwg.phase2.derive_scalar(seed, tag) with one tag each; contribute: seed = 64 bytes of os.urandom | entropy; beacon:
zkwg.phase2.beacon_seed.

SECTION 7 (u32 count, records) [EXT: the order of the fields follows snarkjs' src/powersoftau_utils.js; restated, UNPINNED]: the
RECORD_POINTS -- the five points after the contribution, then per secret x of tau, alpha, beta a proof of knowledge
    g1_s = s G, g1_sx = (s x) G for a random s,   g2_spx = x g2_sp,   g2_sp = challenge_g2(BLAKE2b-512(previous challenge | index byte | g1_s | g1_sx))
(e(g1_s, g2_spx) = e(g1_sx, g2_sp); for tau also e(tauG1 before, g2_spx) = e(tauG1 after, g2_sp)) -- then the NEXT CHALLENGE
= BLAKE2b-512(previous challenge | sections 2 - 6 of the output as stored), a u32 length and the tagged parameters of
zkwg.phase2.PARAMS.  The first challenge of a file without contributions is BLAKE2b-512(its sections 2 - 6).
THE CHALLENGE CHAIN AND THE CHALLENGE POINT ARE ZKWG'S OWN (zkwg.phase2.challenge_g2: snarkjs' ChaCha stream cannot be restated
offline), so `snarkjs powersoftau verify` does NOT accept the file; `prepare`, `setup` and everything else that reads the points do.
Not built: powersoftau verify, import / export challenge."""
import argparse
import ctypes as C
import hashlib
import mmap
import os
import struct
import sys

from .zkey import Q, R

# (section id, bytes per point, points as a function of n = 2^power)
SECTIONS = ((2, 64, lambda n: 2 * n - 1), (3, 128, lambda n: n), (4, 64, lambda n: n), (5, 64, lambda n: n), (6, 128, lambda n: 1),
            (12, 64, lambda n: 4 * n - 1), (13, 128, lambda n: 2 * n - 1), (14, 64, lambda n: 2 * n - 1), (15, 64, lambda n: 2 * n - 1))
LAGRANGE = {12: "tau_g1", 13: "tau_g2", 14: "alpha_tau_g1", 15: "beta_tau_g1"}


class PtauError(ValueError):
    pass


def read_ptau(data, prepared=True):
    """data: bytes, memoryview or mmap -> dict: power, ceremony_power, sections = {id: (offset, size)}.  Sizes are checked before any
    point is touched; a file without sections 12 - 15 is refused ("Powers of tau is not prepared") unless prepared=False, which reads
    an UNPREPARED file and refuses one that has any of them."""
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
    if not prepared and any(sid in sec for sid in LAGRANGE):
        raise ValueError(".ptau: the file is already prepared (it has a section 12 - 15)")
    wanted = [t for t in SECTIONS if prepared or t[0] < 12]
    for sid, point, count in wanted:
        if sid not in sec:
            raise ValueError("Powers of tau is not prepared" if sid >= 12 else f".ptau: section {sid} is missing")
    for sid, point, count in wanted:
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


def truncate(data, power):
    """an UNPREPARED file cut to a smaller power (host only): the header's power set, ceremonyPower kept, sections 2 - 6 cut to
    2 n - 1 | n | n | n | 1 points, section 7 verbatim"""
    info = read_ptau(data, prepared=False)
    if not 1 <= power <= info["power"]:
        raise PtauError(f".ptau: cannot cut a file of power {info['power']} to power {power}")
    n, sec = 1 << power, info["sections"]
    cut = {sid: bytes(data[sec[sid][0]:sec[sid][0] + point * count(n)]) for sid, point, count in SECTIONS if sid < 12}
    contributions = bytes(data[sec[7][0]:sec[7][0] + sec[7][1]]) if 7 in sec else b""
    return write_ptau(power, cut, ceremony_power=info["ceremony_power"], contributions=contributions)


def prepare(data, power=None, device=0):
    """an unprepared file (bytes, or an mmap: only the prefixes are read) -> the prepared file of `power` (None: the file's own) as
    bytes, sections 12 - 15 computed on the device (zkwg_ptau_prepare)"""
    import numpy as np
    from . import _lib
    lib = _lib.load()
    a = np.frombuffer(data, dtype=np.uint8)            # (no copy; works for an mmap)
    size, out_len = C.c_uint64(), C.c_uint64()
    try:
        rc = lib.zkwg_ptau_prepare_size(a.ctypes.data, a.size, power or 0, C.byref(size))
        if rc == 0:
            out = np.empty(size.value, dtype=np.uint8)
            rc = lib.zkwg_ptau_prepare(device, a.ctypes.data, a.size, power or 0, out.ctypes.data, size.value, C.byref(out_len))
    finally:
        del a                                          # (an mmap cannot be closed while a view of it lives)
    if rc != 0:
        msg = lib.zkwg_last_error().decode() if rc == -1 else ""
        raise PtauError(f"{lib.zkwg_strerror(rc).decode()}{': ' + msg if msg else ''}")
    return out[:out_len.value].tobytes()


# ---- new / contribute / beacon --------------------------------------------------------------------------------------------------------------
TAG_TAU, TAG_ALPHA, TAG_BETA = b"zkwg ptau tau v1", b"zkwg ptau alpha v1", b"zkwg ptau beta v1"
TAG_POK = b"zkwg ptau pok v1"
KEYS = ("tau", "alpha", "beta")                   # the index byte of a proof of knowledge is the position here
RECORD_POINTS = (("tau_g1", 64), ("tau_g2", 128), ("alpha_g1", 64), ("beta_g1", 64), ("beta_g2", 128)) + \
    tuple((f"{k}_{f}", size) for k in KEYS for f, size in (("g1_s", 64), ("g1_sx", 64), ("g2_spx", 128)))
# where the five points sit in the file: (section, point index)
RECORD_AT = {"tau_g1": (2, 1), "tau_g2": (3, 1), "alpha_g1": (4, 0), "beta_g1": (5, 0), "beta_g2": (6, 0)}
_G2_GENERATOR = (0x1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed, 0x198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2,
                 0x12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa, 0x090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b)


def _mont(v):
    return ((v << 256) % Q).to_bytes(32, "little")


def generators():
    """-> (G1, G2) in the zkey's form: (1, 2) and the EIP-197 generator, the bases of zkwg_fixed_base_device"""
    return _mont(1) + _mont(2), b"".join(_mont(v) for v in _G2_GENERATOR)


def new(power):
    """snarkjs `powersoftau new`: the file of tau = alpha = beta = 1 -- every point a generator -- with an empty section 7 (host only)"""
    if not 1 <= power <= 28:
        raise PtauError(".ptau: power out of range")
    n, (g1, g2) = 1 << power, generators()
    return write_ptau(power, {2: g1 * (2 * n - 1), 3: g2 * n, 4: g1 * n, 5: g1 * n, 6: g2})


def _fail(lib, rc):
    msg = lib.zkwg_last_error().decode() if rc == -1 else ""
    raise PtauError(f"{lib.zkwg_strerror(rc).decode()}{': ' + msg if msg else ''}")


def _le32(v):
    return int(v % (1 << 256)).to_bytes(32, "little")


def point_mul(group, points, scalars, device=0):
    """scalars[i] * points[i] (bytes in the zkey's form; integers below 2^256, reduced modulo r) -> bytes (zkwg_point_mul_device)"""
    import torch
    from . import _lib
    lib = _lib.load()
    pt = 64 if group == 1 else 128
    if len(points) != pt * len(scalars):
        raise PtauError("one scalar per whole point")
    if not scalars:
        return b""
    dev = torch.device("cuda", device)
    d = torch.frombuffer(bytearray(points), dtype=torch.uint8).to(dev)
    k = torch.frombuffer(bytearray(b"".join(_le32(s) for s in scalars)), dtype=torch.uint8).to(dev)
    out = torch.empty_like(d)
    rc = lib.zkwg_point_mul_device(device, group, d.data_ptr(), len(scalars), k.data_ptr(), out.data_ptr(), 0)
    if rc != 0:
        _fail(lib, rc)
    return bytes(out.cpu().numpy())


def point_powers(group, points, c, t, first=0, device=0):
    """(c t^(first + i) mod r) * points[i] -> bytes (zkwg_point_powers_device: the scalars are computed on the device)"""
    import torch
    from . import _lib
    lib = _lib.load()
    pt = 64 if group == 1 else 128
    if len(points) % pt:
        raise PtauError("the points must be whole")
    if not points:
        return b""
    dev = torch.device("cuda", device)
    d = torch.frombuffer(bytearray(points), dtype=torch.uint8).to(dev)
    out = torch.empty_like(d)
    rc = lib.zkwg_point_powers_device(device, group, d.data_ptr(), len(points) // pt, _le32(c), _le32(t), first, out.data_ptr(), 0)
    if rc != 0:
        _fail(lib, rc)
    return bytes(out.cpu().numpy())


def apply_key(data, tau, alpha, beta, section7, device=0):
    """the unprepared file after the contribution (tau, alpha, beta), with `section7` as its section 7 (zkwg_ptau_apply_key) -> bytes"""
    import numpy as np
    from . import _lib
    lib = _lib.load()
    a = np.frombuffer(data, dtype=np.uint8)            # (no copy; works for an mmap)
    size, out_len = C.c_uint64(), C.c_uint64()
    try:
        rc = lib.zkwg_ptau_apply_key_size(a.ctypes.data, a.size, len(section7), C.byref(size))
        if rc == 0:
            out = np.empty(size.value, dtype=np.uint8)
            rc = lib.zkwg_ptau_apply_key(device, a.ctypes.data, a.size, _le32(tau), _le32(alpha), _le32(beta), bytes(section7), len(section7),
                                         out.ctypes.data, size.value, C.byref(out_len))
    finally:
        del a                                          # (an mmap cannot be closed while a view of it lives)
    if rc != 0:
        _fail(lib, rc)
    return out[:out_len.value].tobytes()


def apply_key_stats():
    """seconds and group operations of this thread's last apply_key (zkwg_ptau_apply_key_stats), per section 2 - 5"""
    from . import _lib
    sec, ops = (C.c_double * 18)(), (C.c_uint64 * 8)()
    _lib.load().zkwg_ptau_apply_key_stats(sec, ops)
    out = {sid: {"upload_check": sec[4 * i], "tables": sec[4 * i + 1], "walk": sec[4 * i + 2], "affine_download": sec[4 * i + 3], "add": ops[2 * i], "dbl": ops[2 * i + 1]}
           for i, sid in enumerate((2, 3, 4, 5))}
    out["parse_copy"], out[6] = sec[16], sec[17]
    return out


def pack_record(rec):
    from . import phase2
    out = b"".join(rec[name] for name, _ in RECORD_POINTS)
    assert len(out) == sum(size for _, size in RECORD_POINTS) and len(rec["next_challenge"]) == 64
    params = phase2.pack_params(rec)
    return out + rec["next_challenge"] + struct.pack("<I", len(params)) + params


def pack_section7(raw_records):
    return struct.pack("<I", len(raw_records)) + b"".join(raw_records) if raw_records else b""


def read_contributions(data):
    """a .ptau, or the payload of its section 7 -> [record]; a record: the RECORD_POINTS (bytes as stored), next_challenge, the fields of
    zkwg.phase2.PARAMS (None where absent) and raw, its bytes in the file.  An empty or missing section 7: []"""
    from . import phase2
    if bytes(data[:4]) == b"ptau":
        sec = read_any(data)[0]["sections"]
        data = bytes(data[sec[7][0]:sec[7][0] + sec[7][1]]) if 7 in sec else b""
    if len(data) == 0:
        return []
    if len(data) < 4:
        raise PtauError("section 7 is shorter than its count")
    n = struct.unpack_from("<I", data, 0)[0]
    pos, recs = 4, []
    fixed = sum(size for _, size in RECORD_POINTS) + 64 + 4
    for _ in range(n):
        if pos + fixed > len(data):
            raise PtauError("section 7: a record runs past the end of the section")
        rec, start = {field: None for _, field, _ in phase2.PARAMS}, pos
        for name, size in RECORD_POINTS:
            rec[name] = bytes(data[pos:pos + size])
            pos += size
        rec["next_challenge"] = bytes(data[pos:pos + 64])
        plen = struct.unpack_from("<I", data, pos + 64)[0]
        pos += 68
        if pos + plen > len(data):
            raise PtauError("section 7: the parameters of a record run past the end of the section")
        rec.update(phase2.unpack_params(data, pos, pos + plen, "section 7", PtauError))
        pos += plen
        rec["raw"] = bytes(data[start:pos])
        recs.append(rec)
    if pos != len(data):
        raise PtauError("section 7: bytes after the last record")
    return recs


def read_any(data):
    """-> (info, "prepared" | "not prepared") of a file in either state"""
    try:
        return read_ptau(data), "prepared"
    except ValueError as e:
        if "not prepared" not in str(e):
            raise
    return read_ptau(data, prepared=False), "not prepared"


def _points_hash(data, info, prefix=b""):
    h = hashlib.blake2b(prefix, digest_size=64)
    for sid in (2, 3, 4, 5, 6):
        o, size = info["sections"][sid]
        h.update(data[o:o + size])
    return h.digest()


def current_challenge(data):
    """the challenge the NEXT contribution answers: the last record's, or BLAKE2b-512(sections 2 - 6) of a file without contributions"""
    recs = read_contributions(data)
    return recs[-1]["next_challenge"] if recs else _points_hash(data, read_ptau(data, prepared=False))


def key_scalars(seed):
    """-> ((tau, alpha, beta), (s_tau, s_alpha, s_beta)): the contribution's secrets and the random scalars of their proofs of knowledge"""
    from . import phase2
    return tuple(phase2.derive_scalar(seed, tag) for tag in (TAG_TAU, TAG_ALPHA, TAG_BETA)), \
        tuple(phase2.derive_scalar(seed, TAG_POK + bytes([i])) for i in range(len(KEYS)))


def pok_challenge_point(challenge, index, g1_s, g1_sx, device=0):
    from . import phase2
    return phase2.challenge_g2(hashlib.blake2b(bytes(challenge) + bytes([index]) + g1_s + g1_sx, digest_size=64).digest(), device)


def _contribute(data, keys, esses, params, device):
    from . import phase2, prover
    info = read_ptau(data, prepared=False)
    recs = read_contributions(data)
    challenge = recs[-1]["next_challenge"] if recs else _points_hash(data, info)
    rec = dict(params)
    for i, (name, x, s) in enumerate(zip(KEYS, keys, esses)):
        g1 = bytes(prover.fixed_base(device, 1, [s, s * x % R]).cpu().numpy())
        rec[f"{name}_g1_s"], rec[f"{name}_g1_sx"] = g1[:64], g1[64:]
        rec[f"{name}_g2_spx"] = phase2.scale_points(2, pok_challenge_point(challenge, i, g1[:64], g1[64:], device), x, device)
    # the record's length is known before the file operation, its five points and the next challenge only after it: they are patched in
    for name, size in RECORD_POINTS[:5]:
        rec[name] = bytes(size)
    rec["next_challenge"] = bytes(64)
    before = [r["raw"] for r in recs]
    out = bytearray(apply_key(data, keys[0], keys[1], keys[2], pack_section7(before + [pack_record(rec)]), device))
    after = read_ptau(out, prepared=False)
    for name, size in RECORD_POINTS[:5]:
        sid, k = RECORD_AT[name]
        o = after["sections"][sid][0] + k * size
        rec[name] = bytes(out[o:o + size])
    rec["next_challenge"] = _points_hash(out, after, challenge)
    s7 = pack_section7(before + [pack_record(rec)])
    o, size = after["sections"][7]
    assert size == len(s7)
    out[o:o + size] = s7
    return bytes(out)


def contribute(data, name, entropy=None, device=0, *, urandom=os.urandom):
    """-> the unprepared file after one more contribution.  entropy: str or bytes mixed into the 64 random bytes; urandom: where those
    come from (a test that must know the secrets passes its own)"""
    e = b"" if entropy is None else entropy.encode() if isinstance(entropy, str) else bytes(entropy)
    keys, esses = key_scalars(urandom(64) + e)
    return _contribute(data, keys, esses, {"name": name}, device)


def beacon(data, name, beacon_hash, num_iterations_exp, device=0):
    """-> the file after a beacon: a contribution whose secrets everyone can recompute from the public beacon_hash (bytes or hex)"""
    from . import phase2
    bh = bytes.fromhex(beacon_hash) if isinstance(beacon_hash, str) else bytes(beacon_hash)
    if not 0 < len(bh) <= 255 or not 10 <= num_iterations_exp <= 63:
        raise PtauError("the beacon hash must be 1 .. 255 bytes and the exponent 10 .. 63")
    keys, esses = key_scalars(phase2.beacon_seed(bh, num_iterations_exp))
    return _contribute(data, keys, esses, {"name": name, "type": phase2.TYPE_BEACON, "num_iterations_exp": num_iterations_exp, "beacon_hash": bh}, device)


def last_stats():
    """seconds and group operations of this thread's last prepare (zkwg_ptau_prepare_stats), per section 12 - 15"""
    from . import _lib
    sec, ops = (C.c_double * 140)(), (C.c_uint64 * 8)()
    _lib.load().zkwg_ptau_prepare_stats(sec, ops)
    return {sid: {"upload_check": sec[3 * i], "transforms": sec[3 * i + 1], "affine_download": sec[3 * i + 2], "add": ops[2 * i], "dbl": ops[2 * i + 1],
                  "levels": list(sec[12 + 32 * i:12 + 32 * i + 32])} for i, sid in enumerate((12, 13, 14, 15))}


def group_ntt(group, points, inverse, device=0):
    """the Fourier transform over `points` (bytes in the zkey's form, a power of two of them) -> bytes (zkwg_group_ntt_device)"""
    import torch
    from . import _lib
    lib = _lib.load()
    pt = 64 if group == 1 else 128
    n = len(points) // pt
    if n * pt != len(points) or n == 0 or n & (n - 1):
        raise PtauError("the points must be whole and a power of two of them")
    d = torch.frombuffer(bytearray(points), dtype=torch.uint8).to(torch.device("cuda", device))
    rc = lib.zkwg_group_ntt_device(device, group, d.data_ptr(), n.bit_length() - 1, 1 if inverse else 0, 0)
    if rc != 0:
        msg = lib.zkwg_last_error().decode() if rc == -1 else ""
        raise PtauError(f"{lib.zkwg_strerror(rc).decode()}{': ' + msg if msg else ''}")
    return bytes(d.cpu().numpy())


def main(argv=None):
    ap = argparse.ArgumentParser(description="powers of tau: a new file, a contribution or a beacon, the preparation for phase 2, or a description")
    sub = ap.add_subparsers(dest="cmd", required=True)
    pn = sub.add_parser("new")
    pn.add_argument("power", type=int)
    pn.add_argument("ptau_out")
    pc = sub.add_parser("contribute")
    pb = sub.add_parser("beacon")
    for p in (pc, pb):
        p.add_argument("ptau_in")
        p.add_argument("ptau_out")
    pb.add_argument("beacon_hash")
    pb.add_argument("num_iterations_exp", type=int)
    pc.add_argument("--entropy")
    for p in (pc, pb):
        p.add_argument("--name", required=True)
        p.add_argument("--device", type=int, default=0)
    pp = sub.add_parser("prepare")
    pp.add_argument("ptau_in")
    pp.add_argument("ptau_out")
    pp.add_argument("--power", type=int, default=None)
    pp.add_argument("--device", type=int, default=0)
    pi = sub.add_parser("info")
    pi.add_argument("ptau")
    a = ap.parse_args(argv)
    if a.cmd == "new":
        try:
            open(a.ptau_out, "wb").write(new(a.power))
        except ValueError as e:
            print(f"no file: {e}", file=sys.stderr)
            return 1
        return 0
    path = a.ptau if a.cmd == "info" else a.ptau_in
    out, why = None, ""
    with open(path, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as mm:
        try:
            if a.cmd == "prepare":
                out = prepare(mm, a.power, a.device)
            elif a.cmd == "contribute":
                out = contribute(mm, a.name, a.entropy, a.device)
            elif a.cmd == "beacon":
                out = beacon(mm, a.name, a.beacon_hash, a.num_iterations_exp, a.device)
            else:
                info, state = read_any(mm)
                out = f"power {info['power']}, ceremony power {info['ceremony_power']}, {state}; sections " + \
                      ", ".join(f"{sid}: {size} bytes" for sid, (_, size) in sorted(info["sections"].items()))
                for i, r in enumerate(read_contributions(mm)):
                    kind = f"beacon {r['beacon_hash'].hex()} 2^{r['num_iterations_exp']}" if r["type"] == 1 else "contribution"
                    out += f"\ncontribution {i + 1}: {kind}, name {r['name']!r}, next challenge {r['next_challenge'].hex()[:16]}..."
        except ValueError as e:
            why = str(e)
    if out is None:
        print(f"no file: {why}", file=sys.stderr)
        return 1
    if a.cmd == "info":
        print(out)
    else:
        open(a.ptau_out, "wb").write(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
