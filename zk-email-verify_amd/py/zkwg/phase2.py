"""python -m zkwg.phase2 contribute in.zkey out.zkey --name N [--entropy E]
python -m zkwg.phase2 beacon in.zkey out.zkey HASHHEX EXP --name N
python -m zkwg.phase2 verify circuit.r1cs pot.ptau circuit.zkey [--device D]
python -m zkwg.phase2 verify circuit.zkey --init init.zkey [--device D]
-- "Phase 2" of the reference's workflow on the device (docs/zk-email-docs/UsageGuide/README.md:149,178-180: `snarkjs zkey contribute` /
`zkey beacon`; the guide's next command reads circuit_0001.zkey, the key AFTER a contribution, :206).  The key python -m zkwg.setup writes
has delta = 1: anyone can forge proofs under it.  A contribution with secret k turns delta into k delta (delta1, delta2 times k, the C and
H bases times 1 / k: zkwg_zkey_apply_delta, csrc/zkwg_phase2_core.h, csrc/zkwg_kernels_phase2.hip) and appends a record to section 10.

THE SCALAR.  k = BLAKE2b-512(tag | seed) mod r, hashed again while it is 0.  contribute: seed = 64 bytes of os.urandom | entropy;
beacon: seed = SHA-256 iterated 2^EXP times over the beacon hash (a sequential chain: host).  hashlib only.

THE RECORD (section 10: 64-byte circuit hash, u32 count, records), as snarkjs writes it -- restated from its published
src/zkey_utils.js [EXT], UNPINNED like the container itself (zkwg/zkey.py): RECORD_POINTS, then a 64-byte transcript, u32 length of the
parameters, and the parameters as (tag byte, value) in the order of PARAMS.
    deltaAfter  delta1 after this contribution            g1_s = s G, g1_sx = (s k) G for a random s
    g2_spx = k g2_sp, g2_sp = challenge_g2(transcript)    transcript = BLAKE2b-512(circuit hash | earlier records | g1_s | g1_sx)
Knowledge of k: e(g1_s, g2_spx) = e(g1_sx, g2_sp) and e(delta1 before, g2_spx) = e(deltaAfter, g2_sp).

THE CHALLENGE POINT IS ZKWG'S OWN.  snarkjs derives g2_sp from a ChaCha stream seeded with the transcript, which cannot be restated
offline; here it is try-and-increment: x in Fq2 from BLAKE2b(tag | transcript | counter | half), y = sqrt(x^3 + 3 / (9 + i)) in Python
integers (q = 3 mod 4; Fq2 roots through the norm), then times the twist's cofactor 2 q - r on the device (zkwg_point_scale_device:
the one scalar here above r).  Nobody knows its discrete logarithm -- a multiple of the generator would let the first contribution be
forged.  `snarkjs zkey verify` therefore does NOT accept the record (nor the circuit hash, which stays as the file holds it: 64 zero
bytes after zkwg.setup); every prover and verifier reads the key.

`verify` (`snarkjs zkey verify` / `zkey verifyfrominit`) CHECKS A KEY against its circuit and ceremony file: the initial key is made again
(zkwg.setup.new_zkey) and everything a contribution must not touch is compared with it byte for byte; delta1 / delta2 are one delta; every
record's transcript, proof of knowledge and link to the delta1 before it (a beacon's scalar recomputed); and sections 8 and 9 are the
initial key's divided by that delta -- each folded, together with the initial key's, into one point per key by a random linear
combination on the device (zkwg.ptau.rlc, the two-array form of zkwg_point_rlc_device) and compared under delta2 by ONE pairing check on
the host (zkwg.pairing).  See `verify_from_init` below for the checks.  The records are zkwg's, so this is the command that reads them."""
import argparse
import contextlib
import ctypes as C
import hashlib
import mmap
import os
import struct
import sys

from . import _call, _lib, zkey

R, Q = zkey.R, zkey.Q
COFACTOR_G2 = 2 * Q - R
TAG_SCALAR, TAG_POK, TAG_G2 = b"zkwg phase2 scalar v1", b"zkwg phase2 pok v1", b"zkwg phase2 challenge v1"
RECORD_POINTS = (("delta_after", 64), ("g1_s", 64), ("g1_sx", 64), ("g2_spx", 128))
# (tag, field, kind): u8 = one byte; bytes / str = a length byte and that many bytes.  A field that is None / 0 / empty is not written.
PARAMS = ((1, "type", "u8"), (2, "num_iterations_exp", "u8"), (3, "beacon_hash", "bytes"), (4, "name", "str"))
TYPE_BEACON = 1


class Phase2Error(ValueError):
    pass


def derive_scalar(seed_bytes, tag=TAG_SCALAR):
    """-> k in [1, r): BLAKE2b-512(tag | seed) mod r, hashed again while 0"""
    h = hashlib.blake2b(tag + bytes(seed_bytes), digest_size=64).digest()
    while int.from_bytes(h, "little") % R == 0:
        h = hashlib.blake2b(tag + h, digest_size=64).digest()
    return int.from_bytes(h, "little") % R


def beacon_seed(beacon_hash, num_iterations_exp):
    h = bytes(beacon_hash)
    for _ in range(1 << num_iterations_exp):
        h = hashlib.sha256(h).digest()
    return h


# ---- section 10 -------------------------------------------------------------------------------------------------------------------------------
def _pack_params(rec):
    out = b""
    for tag, field, kind in PARAMS:
        v = rec.get(field)
        if not v:
            continue
        if kind == "u8":
            out += bytes([tag, v])
        else:
            b = v.encode()[:64] if kind == "str" else bytes(v)
            if len(b) > 255:
                raise Phase2Error(f"{field} is longer than 255 bytes")
            out += bytes([tag, len(b)]) + b
    return out


def unpack_params(data, p, end, where, error=None):
    """the tagged parameters at data[p:end] -> {field: value} (what _pack_params wrote); `where` names the section in a refusal"""
    error = error or Phase2Error
    by_tag = {tag: (field, kind) for tag, field, kind in PARAMS}
    out = {}
    while p < end:
        if data[p] not in by_tag or p + 2 > end:
            raise error(f"{where}: unknown or truncated parameter")
        field, kind = by_tag[data[p]]
        if kind == "u8":
            out[field] = data[p + 1]
            p += 2
        else:
            ln = data[p + 1]
            if p + 2 + ln > end:
                raise error(f"{where}: truncated parameter")
            v = bytes(data[p + 2:p + 2 + ln])
            out[field] = v.decode() if kind == "str" else v
            p += 2 + ln
    return out


pack_params = _pack_params      # (zkwg/ptau.py writes the same tagged parameters)


def pack_record(rec):
    out = b"".join(rec[name] for name, _ in RECORD_POINTS)
    assert len(out) == sum(size for _, size in RECORD_POINTS) and len(rec["transcript"]) == 64
    params = _pack_params(rec)
    return out + rec["transcript"] + struct.pack("<I", len(params)) + params


def read_contributions(zkey_or_section10):
    """a .zkey, or the payload of its section 10 -> (circuit hash, [record]); a record: the RECORD_POINTS (bytes as stored), transcript,
    the PARAMS fields (None where absent) and raw, its bytes in the file.  A key without section 10: (64 zero bytes, [])"""
    data = zkey_or_section10
    if data[:4] == b"zkey":
        sec = zkey.sections(data)
        data = bytes(data[sec[10][0]:sec[10][0] + sec[10][1]]) if 10 in sec else b""
    if len(data) == 0:
        return bytes(64), []
    if len(data) < 68:
        raise Phase2Error("section 10 is shorter than its hash and count")
    n = struct.unpack_from("<I", data, 64)[0]
    pos, recs = 68, []
    fixed = sum(size for _, size in RECORD_POINTS) + 64 + 4
    for _ in range(n):
        if pos + fixed > len(data):
            raise Phase2Error("section 10: a record runs past the end of the section")
        rec, start = {field: None for _, field, _ in PARAMS}, pos
        for name, size in RECORD_POINTS:
            rec[name] = bytes(data[pos:pos + size])
            pos += size
        rec["transcript"] = bytes(data[pos:pos + 64])
        plen = struct.unpack_from("<I", data, pos + 64)[0]
        pos += 68
        if pos + plen > len(data):
            raise Phase2Error("section 10: the parameters of a record run past the end of the section")
        end = pos + plen
        rec.update(unpack_params(data, pos, end, "section 10"))
        pos = end
        rec["raw"] = bytes(data[start:pos])
        recs.append(rec)
    if pos != len(data):
        raise Phase2Error("section 10: bytes after the last record")
    return bytes(data[:64]), recs


def pack_section10(circuit_hash, raw_records):
    return bytes(circuit_hash) + struct.pack("<I", len(raw_records)) + b"".join(raw_records)


# ---- the device ---------------------------------------------------------------------------------------------------------------------------------
def scale_points(group, points, scalar, device=0):
    """scalar * every point of `points` (bytes in the zkey's form; scalar: any integer below 2^256) -> bytes (zkwg_point_scale_device)"""
    import torch
    lib = _lib.load()
    pt = 64 if group == 1 else 128
    if len(points) % pt or not 0 <= scalar < 1 << 256:
        raise Phase2Error("points must be whole and the scalar below 2^256")
    if not points:
        return b""
    d = _call.upload(points, device)
    out = torch.empty_like(d)
    _call.check(lib, lib.zkwg_point_scale_device(device, group, d.data_ptr(), len(points) // pt, _call.le32(scalar), out.data_ptr(), 0), Phase2Error)
    return _call.download(out)


def apply_delta(zkey_bytes, k, section10, device=0):
    """the key with delta times k and `section10` as its section 10 (zkwg_zkey_apply_delta) -> bytes"""
    lib = _lib.load()
    rc, out = _call.sized_call(lambda p, n, size: lib.zkwg_zkey_apply_delta_size(p, n, len(section10), size),
                               lambda p, n, o, cap, out_len: lib.zkwg_zkey_apply_delta(device, p, n, _call.le32(k), bytes(section10), len(section10), o, cap, out_len),
                               zkey_bytes)
    _call.check(lib, rc, Phase2Error)
    return out


def last_stats():
    """seconds and group operations of this thread's last apply_delta (zkwg_zkey_apply_delta_stats)"""
    lib = _lib.load()
    sec, ops = (C.c_double * 5)(), (C.c_uint64 * 4)()
    lib.zkwg_zkey_apply_delta_stats(sec, ops)
    names = ("parse_copy", "upload_check", "scale_c", "scale_h", "affine_download")
    return {"seconds": dict(zip(names, sec)), "ops": {"c": {"add": ops[0], "dbl": ops[1]}, "h": {"add": ops[2], "dbl": ops[3]}}}


# ---- the challenge point ------------------------------------------------------------------------------------------------------------------------
def _f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)


def _fq_sqrt(a):
    s = pow(a, (Q + 1) // 4, Q)                      # q = 3 mod 4
    return s if s * s % Q == a % Q else None


def _f2_sqrt(a):
    """a root of a in Fq2 = Fq[i] / (i^2 + 1), or None: through the norm a0^2 + a1^2, whose root exists in Fq when a is a square"""
    a0, a1 = a
    if a1 == 0:
        s = _fq_sqrt(a0)
        if s is not None:
            return (s, 0)
        return (0, _fq_sqrt(-a0 % Q))                # a0 is not a square, so -a0 is (-1 is not): (t i)^2 = -t^2 = a0
    n = _fq_sqrt((a0 * a0 + a1 * a1) % Q)
    if n is None:
        return None
    half = pow(2, -1, Q)
    x0 = _fq_sqrt((a0 + n) * half % Q)
    if x0 is None:
        x0 = _fq_sqrt((a0 - n) * half % Q)
    if x0 is None or x0 == 0:
        return None
    x = (x0, a1 * pow(2 * x0, -1, Q) % Q)
    return x if _f2_mul(x, x) == (a0 % Q, a1 % Q) else None


_B2 = _f2_mul((3, 0), (9 * pow(82, -1, Q) % Q, -pow(82, -1, Q) % Q))      # 3 / (9 + i) = 3 (9 - i) / 82


def challenge_g2(transcript, device=0):
    """-> a point of G2 (128 bytes in the zkey's form) that only the transcript determines"""
    for counter in range(1 << 16):
        h = [hashlib.blake2b(TAG_G2 + bytes(transcript) + struct.pack("<IB", counter, half), digest_size=64).digest() for half in (0, 1)]
        x = (int.from_bytes(h[0], "little") % Q, int.from_bytes(h[1], "little") % Q)
        x3 = _f2_mul(_f2_mul(x, x), x)
        y = _f2_sqrt(((x3[0] + _B2[0]) % Q, (x3[1] + _B2[1]) % Q))
        if y is None:
            continue
        y = min(y, ((-y[0]) % Q, (-y[1]) % Q))       # (which root: the smaller pair)
        p = scale_points(2, b"".join(_call.mont(v) for v in x + y), COFACTOR_G2, device)
        if any(p):
            return p
    raise Phase2Error("no challenge point found")


# ---- contributions --------------------------------------------------------------------------------------------------------------------------------
def _contribute(zkey_bytes, k, s, params, device):
    from .prover import fixed_base
    sec = zkey.sections(zkey_bytes)
    if 2 not in sec or sec[2][1] < 84 + 576:
        raise Phase2Error("not a groth16 .zkey (header)")
    d1 = sec[2][0] + 84 + 384
    delta1 = bytes(zkey_bytes[d1:d1 + 64])
    circuit_hash, recs = read_contributions(zkey_bytes)
    rec = dict(params)
    rec["delta_after"] = scale_points(1, delta1, k, device)
    g1 = bytes(fixed_base(device, 1, [s, s * k % R]).cpu().numpy())
    rec["g1_s"], rec["g1_sx"] = g1[:64], g1[64:]
    rec["transcript"] = hashlib.blake2b(circuit_hash + b"".join(r["raw"] for r in recs) + g1, digest_size=64).digest()
    rec["g2_spx"] = scale_points(2, challenge_g2(rec["transcript"], device), k, device)
    return apply_delta(zkey_bytes, k, pack_section10(circuit_hash, [r["raw"] for r in recs] + [pack_record(rec)]), device)


def contribution_scalars(seed):
    """-> (k, s): the contribution's secret and the random scalar of its proof of knowledge"""
    return derive_scalar(seed), derive_scalar(seed, TAG_POK)


def contribute(zkey_bytes, name, entropy=None, device=0, *, urandom=os.urandom):
    """-> the key after one more contribution.  entropy: str or bytes mixed into the 64 random bytes; urandom: where those come from
    (a test that must know k passes its own)"""
    e = b"" if entropy is None else entropy.encode() if isinstance(entropy, str) else bytes(entropy)
    k, s = contribution_scalars(urandom(64) + e)
    return _contribute(zkey_bytes, k, s, {"name": name}, device)


def beacon(zkey_bytes, name, beacon_hash, num_iterations_exp, device=0):
    """-> the key after a beacon: a contribution whose scalar everyone can recompute from the public beacon_hash (bytes or hex)"""
    bh = bytes.fromhex(beacon_hash) if isinstance(beacon_hash, str) else bytes(beacon_hash)
    if not 0 < len(bh) <= 255 or not 10 <= num_iterations_exp <= 63:
        raise Phase2Error("the beacon hash must be 1 .. 255 bytes and the exponent 10 .. 63")
    k, s = contribution_scalars(beacon_seed(bh, num_iterations_exp))
    return _contribute(zkey_bytes, k, s, {"name": name, "type": TYPE_BEACON, "num_iterations_exp": num_iterations_exp, "beacon_hash": bh}, device)


# ---- verify ---------------------------------------------------------------------------------------------------------------------------------------
HEADER_POINTS = (("alpha1", 64), ("beta1", 64), ("beta2", 128), ("gamma2", 128), ("delta1", 64), ("delta2", 128))      # after the 84 bytes of section 2
SECTION_ENTRY = {3: 64, 5: 64, 6: 64, 7: 128}     # bytes per point of the sections a contribution copies (section 4: a u32 count, 44 bytes a coefficient)
FOLD_PIECE = 0                                    # points per multi-exponentiation plan of a fold (0: zkwg_point_rlc_device's own 2^22)


def _first_difference(a, b):
    """the lowest index at which two buffers of one length differ, or None"""
    import numpy as np
    x, y = np.frombuffer(a, dtype=np.uint8), np.frombuffer(b, dtype=np.uint8)
    for at in range(0, len(x), 1 << 24):
        d = np.flatnonzero(x[at:at + (1 << 24)] != y[at:at + (1 << 24)])
        if len(d):
            return at + int(d[0])


def _zkey_check(data):
    """zkwg_zkey_check (host only): the header, every section's size against it, the coefficients of section 4"""
    import numpy as np
    lib = _lib.load()
    a = np.frombuffer(data, dtype=np.uint8)            # (no copy; works for an mmap)
    try:
        rc = lib.zkwg_zkey_check(a.ctypes.data, a.size, None, None, None)
    finally:
        del a
    _call.check(lib, rc, Phase2Error)


def _verify_record(rec, circuit_hash, earlier, before, device):
    """one record against the circuit hash, the records before it and the delta1 before it -> (ok, detail)"""
    from . import pairing
    failed = []

    def ratio(what, a, b, c, d):
        try:
            if not pairing.same_ratio(a, b, c, d):
                failed.append(what)
        except pairing.PairingError as e:
            failed.append(f"{what} ({e})")
    transcript = hashlib.blake2b(circuit_hash + b"".join(r["raw"] for r in earlier) + rec["g1_s"] + rec["g1_sx"], digest_size=64).digest()
    if transcript != rec["transcript"]:
        failed.append("transcript")
    sp = challenge_g2(rec["transcript"], device)      # (of the STORED transcript: a wrong one has failed above, and the ratios still say what else holds)
    ratio("proof of knowledge", rec["g1_s"], rec["g1_sx"], sp, rec["g2_spx"])
    ratio("link to the delta1 before", before, rec["delta_after"], sp, rec["g2_spx"])
    kind = "contribution"
    if rec["type"] == TYPE_BEACON:
        kind = "beacon"
        if not rec["beacon_hash"] or not rec["num_iterations_exp"] or not 10 <= rec["num_iterations_exp"] <= 63:
            failed.append("beacon parameters")
        else:
            k, _ = contribution_scalars(beacon_seed(rec["beacon_hash"], rec["num_iterations_exp"]))
            if scale_points(1, before, k, device) != rec["delta_after"]:
                failed.append("delta_after is not the beacon's scalar times the delta1 before")
    who = f"{kind} {rec['name']!r}"
    return (not failed), (who if not failed else f"{who}: " + "; ".join(failed))


def verify_from_init(init_zkey_bytes, zkey_bytes, device=0, *, urandom=os.urandom):
    """-> {"ok": bool, "checks": [(name, ok, detail)]} for a key against the INITIAL key of its circuit (both bytes, or an mmap).  ok of a
    check: True, False, or None = skipped (does not fail).  urandom supplies the 16-byte scalars of the folds.  The checks, in order:

      structure       zkwg_zkey_check accepts both files, section 10 parses, nVars, nPublic, the domain and the sizes of sections 1 - 9 are
                      the initial key's
      header          alpha1, beta1, beta2, gamma2 and the 64 bytes of the circuit hash are the initial key's
      section_3 .. 7  byte-equal to the initial key's; the detail names the first entry that differs
      delta           delta1 is not infinity and same_ratio(G1, delta1, G2, delta2); a delta2 the pairing refuses fails here
      record_k        record k: its transcript recomputed; g2_sp = challenge_g2(transcript), same_ratio(g1_s, g1_sx, g2_sp, g2_spx) and
                      same_ratio(delta1 before, delta_after, g2_sp, g2_spx); a beacon's scalar recomputed and applied
      last_record     the last record's delta_after is the key's delta1; without records delta1, delta2 are the initial key's
      section_8, 9    S' = sum s_i P'_i over the key and S = sum s_i P_i over the initial key, random 16-byte s_i, from ONE two-array fold
                      (zkwg.ptau.rlc's `other`); the key's points are the initial ones divided by delta, so e(S', delta2') = e(S, delta2):
                      pairing.same_ratio(S', S, delta2 of the initial key, delta2 of the key) -- its arguments (a, b, c, d) mean
                      e(a, d) = e(b, c).  A point off its curve is the device's refusal and fails the check
    A failure of `structure` ends the run.  An initial key that holds records itself (the key before this contribution, for a coordinator
    who checks one contribution at a time) is trusted as it is: the key must repeat its records, and the first new one links to its delta1."""
    from . import pairing, ptau
    checks = []

    def done():
        return {"ok": all(ok is not False for _, ok, _ in checks), "checks": checks}
    init, key = init_zkey_bytes, zkey_bytes
    try:
        walked = []
        for name, data in (("the initial key", init), ("the key", key)):
            try:
                s = zkey.sections(data)
                missing = [sid for sid in range(1, 10) if sid not in s]
                if missing or s[2][1] != 84 + sum(size for _, size in HEADER_POINTS):
                    raise Phase2Error(f"section {missing[0]} is missing" if missing else "section 2 is not a groth16 header")
                _zkey_check(data)
                walked.append((s,) + read_contributions(data))
            except ValueError as e:                    # (Phase2Error, and what the section walk of zkwg.zkey raises)
                raise Phase2Error(f"{name}: {e}")
        (sec0, hash0, recs0), (sec, circuit_hash, recs) = walked
        shape0, shape = (struct.unpack_from("<III", d, s[2][0] + 72) for d, s in ((init, sec0), (key, sec)))
        if shape != shape0:
            raise Phase2Error(f"nVars, nPublic, domain are {shape}, the initial key's {shape0}")
        for sid in range(1, 10):
            if sec[sid][1] != sec0[sid][1]:
                raise Phase2Error(f"section {sid} holds {sec[sid][1]} bytes, the initial key's {sec0[sid][1]}")
    except Phase2Error as e:
        checks.append(("structure", False, str(e)))
        return done()
    checks.append(("structure", True, f"{shape[0]} wires, {shape[1]} public, domain {shape[2]}, " +
                   (f"{len(recs)} contribution{'s' if len(recs) != 1 else ''}" if recs else "no contributions")))
    view0, view = memoryview(init), memoryview(key)
    part0 = lambda sid: view0[sec0[sid][0]:sec0[sid][0] + sec0[sid][1]]
    part = lambda sid: view[sec[sid][0]:sec[sid][0] + sec[sid][1]]
    hdr0, hdr, at = {}, {}, 84
    for name, size in HEADER_POINTS:
        hdr0[name], hdr[name] = bytes(part0(2)[at:at + size]), bytes(part(2)[at:at + size])
        at += size
    differ = [name for name in ("alpha1", "beta1", "beta2", "gamma2") if hdr[name] != hdr0[name]] + (["the circuit hash"] if circuit_hash != hash0 else [])
    checks.append(("header", not differ, f"{', '.join(differ)} differ{'s' if len(differ) == 1 else ''} from the initial key's" if differ else "alpha1, beta1, beta2, gamma2, the circuit hash"))
    for sid in (3, 4, 5, 6, 7):
        d = _first_difference(part(sid), part0(sid))
        if d is None:
            checks.append((f"section_{sid}", True, f"{sec[sid][1]} bytes"))
        elif sid == 4:
            checks.append(("section_4", False, "the count differs" if d < 4 else f"coefficient {(d - 4) // 44} differs (byte {d} of the section)"))
        else:
            checks.append((f"section_{sid}", False, f"point {d // SECTION_ENTRY[sid]} differs"))
    g1, g2 = ptau.generators()

    def ratio(name, a, b, c, d, detail):
        try:
            checks.append((name, pairing.same_ratio(a, b, c, d), detail))
        except pairing.PairingError as e:
            checks.append((name, False, str(e)))
    if not any(hdr["delta1"]):
        checks.append(("delta", False, "delta1 is the point at infinity"))
    else:
        ratio("delta", g1, hdr["delta1"], g2, hdr["delta2"], "delta1 and delta2 are one delta")
    # ---- the records
    before = hdr0["delta1"]
    for k, rec in enumerate(recs):
        if k < len(recs0):
            same = rec["raw"] == recs0[k]["raw"]
            checks.append((f"record_{k + 1}", same, "as in the initial key" if same else "differs from the initial key's record"))
            continue
        ok, detail = _verify_record(rec, circuit_hash, recs[:k], before, device)
        checks.append((f"record_{k + 1}", ok, detail))
        before = rec["delta_after"]
    if len(recs) < len(recs0):
        checks.append(("last_record", False, f"the key holds {len(recs)} records, the initial key {len(recs0)}"))
    elif len(recs) > len(recs0):
        same = recs[-1]["delta_after"] == hdr["delta1"]
        checks.append(("last_record", same, "the last record's delta_after is the key's delta1" if same else "the last record's delta_after is not the key's delta1"))
    else:
        same = hdr["delta1"] == hdr0["delta1"] and hdr["delta2"] == hdr0["delta2"]
        checks.append(("last_record", same, "no contribution: delta is the initial key's" if same else "no contribution, but delta is not the initial key's"))
    # ---- sections 8 and 9: one fold of both keys, one pairing check
    B = ptau._backend(device)
    for sid in (8, 9):
        name, n = f"section_{sid}", sec[sid][1] // 64
        if n == 0:
            checks.append((name, True, "no points"))
            continue
        try:
            s_key, s_init = B.rlc(1, B.upload(part(sid)), 0, n, B.upload(urandom(16 * n)), piece=FOLD_PIECE, other=B.upload(part0(sid)))
        except ptau.PointRefused as e:                 # (the device's curve check, by its return code)
            checks.append((name, False, str(e)))
            continue
        if not any(s_key) or not any(s_init):          # (every point at infinity on both sides is a key without such wires; on one side only, a difference)
            both = not any(s_key) and not any(s_init)
            checks.append((name, both, f"{n} points, all at infinity" if both else "one fold is the point at infinity, the other is not"))
        else:
            ratio(name, s_key, s_init, hdr0["delta2"], hdr["delta2"], f"{n} points")
    return done()


def verify(r1cs_bytes, ptau_bytes, zkey_bytes, device=0, *, urandom=os.urandom):
    """`snarkjs zkey verify`: the initial key is made again from the circuit and the PREPARED powers of tau (zkwg.setup.new_zkey, which
    raises what it refuses there), the rest is verify_from_init.  -> {"ok": bool, "checks": [(name, ok, detail)]}"""
    from . import setup
    return verify_from_init(setup.new_zkey(r1cs_bytes, ptau_bytes, device), zkey_bytes, device, urandom=urandom)


def main(argv=None):
    ap = argparse.ArgumentParser(description="phase 2 of the groth16 set-up: a contribution or a beacon on a .zkey, or the verification of a key")
    sub = ap.add_subparsers(dest="cmd", required=True)
    pc = sub.add_parser("contribute")
    pb = sub.add_parser("beacon")
    for p in (pc, pb):
        p.add_argument("zkey_in")
        p.add_argument("zkey_out")
    pb.add_argument("beacon_hash")
    pb.add_argument("num_iterations_exp", type=int)
    pc.add_argument("--entropy")
    for p in (pc, pb):
        p.add_argument("--name", required=True)
        p.add_argument("--device", type=int, default=0)
    pv = sub.add_parser("verify", description="circuit.r1cs pot.ptau circuit.zkey: the initial key is made again from the circuit and the prepared "
                        "powers of tau; circuit.zkey --init init.zkey: it is read from a file (a coordinator makes it once)")
    pv.add_argument("files", nargs="+", metavar="FILE", help="circuit.r1cs pot.ptau circuit.zkey, or with --init: circuit.zkey")
    pv.add_argument("--init", metavar="INIT_ZKEY")
    pv.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.cmd == "verify":
        return _main_verify(a, pv)
    z, why = None, ""
    with open(a.zkey_in, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as mm:
        try:
            z = contribute(mm, a.name, a.entropy, a.device) if a.cmd == "contribute" else beacon(mm, a.name, a.beacon_hash, a.num_iterations_exp, a.device)
        except ValueError as e:                        # (Phase2Error, and what the section walk of zkwg.zkey raises)
            why = str(e)
    if z is None:
        print(f"no key: {why}", file=sys.stderr)
        return 1
    open(a.zkey_out, "wb").write(z)
    return 0


def _main_verify(a, parser):
    if len(a.files) != (1 if a.init else 3):
        parser.error("verify takes circuit.r1cs pot.ptau circuit.zkey, or circuit.zkey --init init.zkey")
    res, why = None, ""
    try:
        with contextlib.ExitStack() as stack:
            def mapped(path):                          # (an empty file cannot be mapped: ValueError)
                f = stack.enter_context(open(path, "rb"))
                return stack.enter_context(mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ))
            key = mapped(a.files[-1])
            if a.init:
                res = verify_from_init(mapped(a.init), key, a.device)
            else:
                with open(a.files[0], "rb") as f:
                    r1cs = f.read()
                res = verify(r1cs, mapped(a.files[1]), key, a.device)
    except (ValueError, OSError) as e:                 # (a file that is missing or empty, and what the set-up refuses in the .r1cs or the .ptau)
        why = str(e)
    if res is None:
        print(f"no verdict: {why}", file=sys.stderr)
        return 1
    for name, ok, detail in res["checks"]:
        print(f"{name}: {'ok' if ok else 'skipped' if ok is None else 'FAILED'}  {detail}")
    print("the key verifies" if res["ok"] else "the key does NOT verify")
    return 0 if res["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
