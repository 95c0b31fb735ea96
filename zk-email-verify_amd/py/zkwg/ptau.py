"""python -m zkwg.ptau new POWER out.ptau
python -m zkwg.ptau contribute in.ptau out.ptau --name N [--entropy E] [--device D]
python -m zkwg.ptau beacon in.ptau out.ptau HASHHEX EXP --name N [--device D]
python -m zkwg.ptau prepare in.ptau out.ptau [--power P] [--device D]
python -m zkwg.ptau info file.ptau
python -m zkwg.ptau verify file.ptau [--device D]
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

`verify` CHECKS A FILE END TO END, in either state and at any point of the workflow: every point reduced and on its curve, every G2 point
of sections 3, 6, 13 in the subgroup of order r (zkwg_g2_subgroup_device), the sections powers of ONE tau (and alpha, beta times them),
every record's proofs of knowledge and its link to the record before, the challenge chain's last link, and the Lagrange sections against
the powers.  A section of 2^21 points becomes the four points of one pairing check by a random linear combination on the device
(zkwg_point_rlc_device); the pairings themselves, a few dozen, run on the host (zkwg.pairing).  See `verify` below for the checks.  (`zkey verify`, the check of a phase-2 key, is zkwg.phase2.verify; it folds
with `rlc`'s two-array form.)  Not built: snarkjs-compatible challenge hashes, import / export challenge."""
import argparse
import ctypes as C
import hashlib
import mmap
import os
import struct
import sys

from . import _call
from .zkey import Q, R

# (section id, bytes per point, points as a function of n = 2^power)
SECTIONS = ((2, 64, lambda n: 2 * n - 1), (3, 128, lambda n: n), (4, 64, lambda n: n), (5, 64, lambda n: n), (6, 128, lambda n: 1),
            (12, 64, lambda n: 4 * n - 1), (13, 128, lambda n: 2 * n - 1), (14, 64, lambda n: 2 * n - 1), (15, 64, lambda n: 2 * n - 1))
LAGRANGE = {12: "tau_g1", 13: "tau_g2", 14: "alpha_tau_g1", 15: "beta_tau_g1"}


class PtauError(ValueError):
    pass


class PointRefused(PtauError):
    """zkwg_point_rlc_device refused its points: ZKWG_RC_BAD_CONFIG, which that call returns for one reason only -- a point of either
    array is not reduced or not on its curve"""


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
    from . import _lib
    lib = _lib.load()
    rc, out = _call.sized_call(lambda p, n, size: lib.zkwg_ptau_prepare_size(p, n, power or 0, size),
                               lambda p, n, o, cap, out_len: lib.zkwg_ptau_prepare(device, p, n, power or 0, o, cap, out_len), data)
    _call.check(lib, rc, PtauError)
    return out


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


def generators():
    """-> (G1, G2) in the zkey's form: (1, 2) and the EIP-197 generator, the bases of zkwg_fixed_base_device"""
    return _call.mont(1) + _call.mont(2), b"".join(_call.mont(v) for v in _G2_GENERATOR)


def new(power):
    """snarkjs `powersoftau new`: the file of tau = alpha = beta = 1 -- every point a generator -- with an empty section 7 (host only)"""
    if not 1 <= power <= 28:
        raise PtauError(".ptau: power out of range")
    n, (g1, g2) = 1 << power, generators()
    return write_ptau(power, {2: g1 * (2 * n - 1), 3: g2 * n, 4: g1 * n, 5: g1 * n, 6: g2})


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
    d, k = _call.upload(points, device), _call.upload(b"".join(_call.le32(s) for s in scalars), device)
    out = torch.empty_like(d)
    _call.check(lib, lib.zkwg_point_mul_device(device, group, d.data_ptr(), len(scalars), k.data_ptr(), out.data_ptr(), 0), PtauError)
    return _call.download(out)


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
    d = _call.upload(points, device)
    out = torch.empty_like(d)
    _call.check(lib, lib.zkwg_point_powers_device(device, group, d.data_ptr(), len(points) // pt, _call.le32(c), _call.le32(t), first, out.data_ptr(), 0), PtauError)
    return _call.download(out)


def apply_key(data, tau, alpha, beta, section7, device=0):
    """the unprepared file after the contribution (tau, alpha, beta), with `section7` as its section 7 (zkwg_ptau_apply_key) -> bytes"""
    from . import _lib
    lib = _lib.load()
    keys = [_call.le32(v) for v in (tau, alpha, beta)]
    rc, out = _call.sized_call(lambda p, n, size: lib.zkwg_ptau_apply_key_size(p, n, len(section7), size),
                               lambda p, n, o, cap, out_len: lib.zkwg_ptau_apply_key(device, p, n, *keys, bytes(section7), len(section7), o, cap, out_len), data)
    _call.check(lib, rc, PtauError)
    return out


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
    from . import _lib
    lib = _lib.load()
    pt = 64 if group == 1 else 128
    n = len(points) // pt
    if n * pt != len(points) or n == 0 or n & (n - 1):
        raise PtauError("the points must be whole and a power of two of them")
    d = _call.upload(points, device)
    _call.check(lib, lib.zkwg_group_ntt_device(device, group, d.data_ptr(), n.bit_length() - 1, 1 if inverse else 0, 0), PtauError)
    return _call.download(d)


# ---- verify ---------------------------------------------------------------------------------------------------------------------------------------
POWERS = {2: 1, 3: 2, 4: 1, 5: 1}                  # section -> group
LAGRANGE_OF = {12: 2, 13: 3, 14: 4, 15: 5}         # Lagrange section -> the section of its powers
_W28 = pow(5, (R - 1) >> 28, R)                    # ffjavascript's Fr.w[28]; w[q] = w[q + 1]^2
NTT_MIN_LOG2 = 2                                   # the smallest domain of zkwg_ntt_create


class _Device:
    """the device calls of `verify` over torch tensors (the CPU tests put host mirrors in its place)"""

    def __init__(self, device):
        import torch
        from . import _lib
        self.device, self.torch, self.lib = device, torch, _lib.load()
        self.dev = torch.device("cuda", device)

    def upload(self, data):
        return _call.upload(data, self.device)

    def g2_subgroup(self, points, n):
        """-> (points outside the subgroup, the lowest index of one or None)"""
        n_bad, first = C.c_uint64(), C.c_uint64()
        _call.check(self.lib, self.lib.zkwg_g2_subgroup_device(self.device, points.data_ptr(), n, C.byref(n_bad), C.byref(first), 0), PtauError)
        return n_bad.value, (first.value if n_bad.value else None)

    def rlc(self, group, points, first, n, scalars, wide=False, shifted=False, piece=0, other=None):
        """sum_i s_i P[first + i], i < n -> (sum, None); shifted: also sum_i s_i P[first + i + 1] from the same upload; other (a second
        array of the same group on the device): also sum_i s_i other[first + i], from the same call.  scalars: n x 16 bytes on the device
        (wide: n x 32, below r)"""
        pt = 64 if group == 1 else 128
        a = points.data_ptr() + first * pt
        b = a + pt if shifted else other.data_ptr() + first * pt if other is not None else None
        out_a, out_b = (C.c_uint8 * pt)(), (C.c_uint8 * pt)()
        fn = self.lib.zkwg_point_rlc32_device if wide else self.lib.zkwg_point_rlc_device
        rc = fn(self.device, group, a, b, n, scalars.data_ptr(), piece, out_a, out_b if b is not None else None, 0)
        if rc == _call.BAD_CONFIG:
            raise PointRefused(f"{self.lib.zkwg_strerror(rc).decode()}: {self.lib.zkwg_last_error().decode()}")
        _call.check(self.lib, rc, PtauError)
        return bytes(out_a), (bytes(out_b) if b is not None else None)

    def ifft(self, scalars16, q):
        """2^q 16-byte values (bytes) -> their inverse field transform over the 2^q-th roots, 32-byte values on the device"""
        import numpy as np
        n = 1 << q
        wide = np.zeros((n, 32), dtype=np.uint8)
        wide[:, :16] = np.frombuffer(scalars16, dtype=np.uint8).reshape(n, 16)
        d = self.torch.from_numpy(wide.reshape(-1)).to(self.dev)
        plan = C.c_void_p()
        rc = self.lib.zkwg_ntt_create(self.device, q, C.byref(plan))
        if rc == 0:
            # (the transform is linear and its tables carry the Montgomery factor: standard-form values in, standard-form values out)
            rc = self.lib.zkwg_ntt_transform_device(plan, d.data_ptr(), 1, 1, 0)
            self.lib.zkwg_ntt_destroy(plan)
        _call.check(self.lib, rc, PtauError)
        return d


def _backend(device):
    return _Device(device)


def g2_subgroup(points, device=0):
    """128-byte G2 points (bytes in the zkey's form) -> (how many are outside the subgroup of order r, the lowest index of one or None)
    (zkwg_g2_subgroup_device)"""
    if len(points) % 128:
        raise PtauError("the points must be whole")
    B = _backend(device)
    return B.g2_subgroup(B.upload(points), len(points) // 128) if points else (0, None)


def rlc(group, points, scalars, shifted=False, wide=False, piece=0, device=0, other=None):
    """sum_i s_i P_i for points and 16-byte scalars as bytes (wide: 32-byte scalars below r) -> the point in the zkey's form
    (zkwg_point_rlc_device).  shifted: one point more than scalars; -> (sum_i s_i P_i, sum_i s_i P_(i+1)) from ONE array on the device.
    other: as many points of the same group in an array of their own; -> (sum_i s_i P_i, sum_i s_i other_i) from ONE call, the two
    arrays under the same scalars (what zkwg.phase2.verify folds sections 8 / 9 of two keys with)"""
    pt, sb = (64 if group == 1 else 128), (32 if wide else 16)
    n = len(scalars) // sb
    if len(scalars) != n * sb or len(points) != (n + (1 if shifted else 0)) * pt or n == 0:
        raise PtauError("one scalar per whole point (and one point more in the shifted form)")
    if other is not None and (shifted or len(other) != len(points)):
        raise PtauError("the other array holds as many points of the same group, and there is no shifted form of two arrays")
    B = _backend(device)
    if other is not None:
        return B.rlc(group, B.upload(points), 0, n, B.upload(scalars), wide=wide, piece=piece, other=B.upload(other))
    out = B.rlc(group, B.upload(points), 0, n, B.upload(scalars), wide=wide, shifted=shifted, piece=piece)
    return out if shifted else out[0]


def ifft_host(values, q):
    """the inverse transform of 2^q integers by the definition: out[k] = 2^-q sum_j values[j] w^(-j k), w = Fr.w[q]"""
    n = 1 << q
    w_inv = pow(pow(_W28, 1 << (28 - q), R), -1, R)
    n_inv = pow(n, -1, R)
    return [n_inv * sum(v * pow(w_inv, j * k, R) for j, v in enumerate(values)) % R for k in range(n)]


def new_challenge(power):
    """BLAKE2b-512 of sections 2 - 6 of new(power), streamed (the file itself is 2^power x 384 bytes)"""
    n, (g1, g2) = 1 << power, generators()
    h = hashlib.blake2b(digest_size=64)
    for point, count in ((g1, 2 * n - 1), (g2, n), (g1, n), (g1, n), (g2, 1)):
        block = point * min(count, 1 << 14)
        for _ in range(count // (1 << 14)):
            h.update(block)
        h.update(point * (count % (1 << 14)))
    return h.digest()


def _has_infinity(view, pt):
    import numpy as np
    a = np.frombuffer(view, dtype=np.uint8).reshape(-1, pt)
    return bool((~a.any(axis=1)).any())


def _verify_record(rec, prev, challenge, device):
    """one record against the five points before it and the challenge it answers -> (ok, detail)"""
    from . import pairing, phase2
    g1, g2 = generators()
    failed = []

    def ratio(what, a, b, c, d):
        try:
            if not pairing.same_ratio(a, b, c, d):
                failed.append(what)
        except pairing.PairingError as e:
            failed.append(f"{what} ({e})")
    for i, name in enumerate(KEYS):
        s, sx, spx = rec[f"{name}_g1_s"], rec[f"{name}_g1_sx"], rec[f"{name}_g2_spx"]
        sp = pok_challenge_point(challenge, i, s, sx, device)
        ratio(f"{name}: proof of knowledge", s, sx, sp, spx)
        ratio(f"{name}: link to the points before", prev[f"{name}_g1"], rec[f"{name}_g1"], sp, spx)
    ratio("tau_g1 / tau_g2", g1, rec["tau_g1"], g2, rec["tau_g2"])
    ratio("beta_g1 / beta_g2", g1, rec["beta_g1"], g2, rec["beta_g2"])
    kind = "contribution"
    if rec["type"] == phase2.TYPE_BEACON:
        kind = "beacon"
        if not rec["beacon_hash"] or not rec["num_iterations_exp"] or not 10 <= rec["num_iterations_exp"] <= 63:
            failed.append("beacon parameters")
        else:
            (tau, _, _), _ = key_scalars(phase2.beacon_seed(rec["beacon_hash"], rec["num_iterations_exp"]))
            if phase2.scale_points(1, prev["tau_g1"], tau, device) != rec["tau_g1"]:
                failed.append("tau_g1 is not the beacon's tau times the tau_g1 before")
    who = f"{kind} {rec['name']!r}"
    return (not failed), (who if not failed else f"{who}: " + "; ".join(failed))


def verify(data, device=0, *, urandom=os.urandom):
    """-> {"ok": bool, "checks": [(name, ok, detail)]} for a .ptau in either state (bytes, or an mmap).  ok of a check: True, False, or
    None = skipped (does not fail).  urandom supplies the 16-byte scalars of the random linear combinations.  The checks, in order:

      structure       what read_any / read_contributions refuse
      points          every point of sections 2 - 6 (and 12 - 15) reduced and on its curve (the device's check); none of 2 - 6 infinity
      subgroup        every point of sections 3, 6, 13 in the subgroup of order r (zkwg_g2_subgroup_device)
      anchors         point 0 of sections 2 and 3 are the generators
      powers_2 .. 5   S_a = sum s_i P_i, S_b = sum s_i P_(i+1) have the ratio tau: same_ratio(S_a, S_b, G2, tau G2); section 3:
                      same_ratio(G1, tau G1, S_a, S_b).  Skipped when a G2 point of the check is outside the subgroup (`subgroup` says so)
      beta            same_ratio(G1, beta G1, G2, beta G2)
      record_k        record k: three proofs of knowledge, their links to the points of record k - 1, tau and beta in both groups;
                      a beacon's tau recomputed
      last_record     the last record's five points are the file's
      last_challenge  its next_challenge = BLAKE2b-512(previous challenge | sections 2 - 6); skipped for a truncated file
      lagrange_12 .. 15   per level q: sum_j s_j Lag_q[j] == sum_k ifft(s)_k P_k, two points compared directly
    A failure of `structure` or `points` ends the run: nothing after it would mean anything."""
    from . import pairing
    checks = []

    def done():
        return {"ok": all(ok is not False for _, ok, _ in checks), "checks": checks}
    try:
        info, state = read_any(data)
        recs = read_contributions(data)
    except ValueError as e:
        checks.append(("structure", False, str(e)))
        return done()
    power, sec = info["power"], info["sections"]
    n = 1 << power
    checks.append(("structure", True, f"power {power}, ceremony power {info['ceremony_power']}, {state}, " +
                   (f"{len(recs)} contribution{'s' if len(recs) != 1 else ''}" if recs else "no contributions")))
    view = memoryview(data)
    part = lambda sid: view[sec[sid][0]:sec[sid][0] + sec[sid][1]]
    pt_of = lambda sid: 128 if sid in (3, 6, 13) else 64
    point = lambda sid, k: bytes(view[sec[sid][0] + k * pt_of(sid):sec[sid][0] + (k + 1) * pt_of(sid)])
    sids = [2, 3, 4, 5, 6] + ([12, 13, 14, 15] if state == "prepared" else [])
    # ---- everything the device computes, first: its curve check is the `points` check
    inf = [sid for sid in (2, 3, 4, 5, 6) if _has_infinity(part(sid), pt_of(sid))]
    if inf:
        checks.append(("points", False, f"section {inf[0]} holds a point at infinity"))
        return done()
    B = _backend(device)
    outside, sums, lag = {}, {}, {}
    sid = 0
    try:
        for sid in sids:
            group, count = (2 if pt_of(sid) == 128 else 1), sec[sid][1] // pt_of(sid)
            d = B.upload(part(sid))
            if group == 2:
                outside[sid] = B.g2_subgroup(d, count)
            if sid in POWERS and count > 1:
                sums[sid] = B.rlc(group, d, 0, count - 1, B.upload(urandom(16 * (count - 1))), shifted=True)
            if sid in LAGRANGE_OF:
                src = B.upload(part(LAGRANGE_OF[sid]))
                lag[sid] = []
                for q in range(power + (2 if sid == 12 else 1)):
                    m = 1 << q
                    s = urandom(16 * m)
                    left = B.rlc(group, d, m - 1, m, B.upload(s))[0]
                    if q < NTT_MIN_LOG2:
                        hat = B.upload(b"".join(v.to_bytes(32, "little") for v in ifft_host([int.from_bytes(s[16 * j:16 * j + 16], "little") for j in range(m)], q)))
                    else:
                        hat = B.ifft(s, q)
                    right = B.rlc(group, src, 0, min(m, 2 * n - 1), hat, wide=True)[0]      # (level power + 1: the pad's scalar meets no point)
                    lag[sid].append(left == right)
                    del hat
                del src
            del d
    except PtauError as e:
        if "curve" not in str(e):
            raise
        checks.append(("points", False, f"section {sid}: {e}"))
        return done()
    checks.append(("points", True, f"sections {', '.join(str(s) for s in sids)}"))
    bad = {s: v for s, v in outside.items() if v[0]}
    checks.append(("subgroup", not bad, "; ".join(f"section {s}: {v[0]} point{'s' if v[0] != 1 else ''} outside the subgroup, the first at {v[1]}" for s, v in bad.items())
                   or f"sections {', '.join(str(s) for s in outside)}"))
    g1, g2 = generators()
    checks.append(("anchors", point(2, 0) == g1 and point(3, 0) == g2, "point 0 of sections 2 and 3"))
    tau_g1, tau_g2 = point(2, 1), point(3, 1)

    def ratio(name, a, b, c, d, detail):
        try:
            checks.append((name, pairing.same_ratio(a, b, c, d), detail))
        except pairing.PairingError as e:
            if bad and "subgroup" in str(e):             # no pairing is defined there, and `subgroup` has reported why
                checks.append((name, None, "skipped (a G2 point of the check is outside the subgroup)"))
            else:
                checks.append((name, False, str(e)))
    for s in (2, 3, 4, 5):
        count = sec[s][1] // pt_of(s)
        if s == 3:
            ratio("powers_3", g1, tau_g1, sums[3][0], sums[3][1], f"{count} points")
        else:
            ratio(f"powers_{s}", sums[s][0], sums[s][1], g2, tau_g2, f"{count} points")
    ratio("beta", g1, point(5, 0), g2, point(6, 0), "sections 5 and 6")
    # ---- the records
    if recs:
        prev = {"tau_g1": g1, "tau_g2": g2, "alpha_g1": g1, "beta_g1": g1, "beta_g2": g2}
        challenge = new_challenge(info["ceremony_power"])
        for k, rec in enumerate(recs):
            ok, detail = _verify_record(rec, prev, challenge, device)
            checks.append((f"record_{k + 1}", ok, detail))
            prev, before, challenge = rec, challenge, rec["next_challenge"]
        same = all(rec[name] == point(*RECORD_AT[name]) for name in RECORD_AT)
        checks.append(("last_record", same, "the last record's five points are the file's" if same else "the last record's five points are not the file's"))
        if power < info["ceremony_power"]:
            checks.append(("last_challenge", None, "skipped (truncated)"))
        else:
            checks.append(("last_challenge", recs[-1]["next_challenge"] == _points_hash(view, info, before), "the last next_challenge against sections 2 - 6"))
    for sid in lag:
        wrong = [q for q, ok in enumerate(lag[sid]) if not ok]
        checks.append((f"lagrange_{sid}", not wrong, f"level{'s' if len(wrong) != 1 else ''} {', '.join(str(q) for q in wrong)} differ from the powers" if wrong else f"{len(lag[sid])} levels"))
    return done()


def main(argv=None):
    ap = argparse.ArgumentParser(description="powers of tau: a new file, a contribution or a beacon, the preparation for phase 2, a description, or the verification of a file")
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
    pv = sub.add_parser("verify")
    pv.add_argument("ptau")
    pv.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.cmd == "new":
        try:
            open(a.ptau_out, "wb").write(new(a.power))
        except ValueError as e:
            print(f"no file: {e}", file=sys.stderr)
            return 1
        return 0
    if a.cmd == "verify":
        with open(a.ptau, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as mm:
            res = verify(mm, a.device)
        for name, ok, detail in res["checks"]:
            print(f"{name}: {'ok' if ok else 'skipped' if ok is None else 'FAILED'}  {detail}")
        print("the file verifies" if res["ok"] else "the file does NOT verify")
        return 0 if res["ok"] else 1
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
