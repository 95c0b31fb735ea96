"""A powers-of-tau contribution on the CPU: the host build of csrc/zkwg_ptau_key_core.h (tests/native/ptaukeytest.cpp -- the regular
recoding, the per-lane scalars c t^k, the table and the walk a lane of zk_ptau_key_walk runs, the set-up's conversion to affine points and
the file operation over them) against the oracle's group arithmetic (oracle/pyref/bn254_g1.py, bn254_g2.py), against the toy ceremony of
a known trapdoor (tests/ptautest.py) and, for the records of section 7, the oracle pairing.  All comparisons are exact, and no limb-form
bound is violated."""
import hashlib
import random
import struct

import pytest

import phase2test
import ptaukeytest
import ptautest
import setuptest
from oracle.pyref import bn254_g1 as G1
from oracle.pyref import bn254_g2 as G2
from oracle.pyref import bn254_pairing as P

R, Q = setuptest.R, setuptest.Q
EDGES = ptaukeytest.EDGES


def test_recoding_is_regular_and_reassembles_to_the_scalar():
    rng = random.Random(51)
    assert ptaukeytest.load().pk_window() == 4
    assert {0, 1, 2, 3, 4, R - 2, R - 1, 1 << 253} <= set(EDGES)         # (r is odd: r - 1 is the largest even, r - 2 the largest odd value)
    allowed = {d for d in range(-15, 16) if d % 2}
    for k in EDGES + [rng.randrange(R) for _ in range(300)] + [rng.randrange(1 << b) for b in (8, 64, 130, 200) for _ in range(20)]:
        digits, minus_p = ptaukeytest.recode(k)
        assert len(digits) == 64 and set(digits) <= allowed, k            # every window non-zero: no lane ever skips an addition
        assert digits[63] == (3 if k >> 253 else 1), k                    # the walk starts from P or 3 P, never from a negative row
        assert sum(d << (4 * i) for i, d in enumerate(digits)) - (1 if minus_p else 0) == k, k
        assert minus_p == (k % 2 == 0)


def test_the_p_equals_q_cases_of_the_header():
    """before window i the accumulator is 16 M P and the addend d_i P: 16 M = +-d_i mod r only for k = r - 1, at the last window"""
    rng = random.Random(52)
    for k in EDGES + [R - 5, R - 16, R - 17, R - 31, R - 33] + [rng.randrange(R) for _ in range(100)]:
        digits, _ = ptaukeytest.recode(k)
        m = digits[63]
        for i in range(62, -1, -1):
            hit = (16 * m - digits[i]) % R == 0, (16 * m + digits[i]) % R == 0
            assert hit == (False, k == R - 1 and i == 0), (k, i)
            m = 16 * m + digits[i]
        assert m == k | 1


def test_per_lane_scalars_equal_pow():
    rng = random.Random(53)
    before = ptaukeytest.violations()
    for first in (0, 1, (1 << 20) - 100, (1 << 32) + 12345, (1 << 64) - 200):
        for c, t in ((1, rng.randrange(1, R)), (rng.randrange(1, R), rng.randrange(1, R)), (R - 1, R - 1), (rng.randrange(1, R), 1), (5 + R, 3 + 2 * R)):
            got = ptaukeytest.powers(c, t, first, 200)
            assert got == [c * pow(t, first + k, R) % R for k in range(200)], (first, c, t)
    assert ptaukeytest.powers(0, 5, 0, 4) is None and ptaukeytest.powers(5, R, 0, 4) is None
    assert ptaukeytest.violations() == before == 0


def test_host_multiplication_of_g1_points_equals_the_oracle():
    rng = random.Random(54)
    logs = [rng.randrange(1, R) for _ in range(70)]
    logs[5] = logs[40] = logs[69] = 0                                     # infinity among them, the last point included
    logs[6], logs[7] = 1, R - 1
    scalars = EDGES + [rng.randrange(R) for _ in range(70 - len(EDGES))]
    scalars[40] = R - 1                                                   # r - 1 and 0 on infinity
    pts = setuptest.host_points(1, logs)
    assert pts[64 * 5:64 * 6] == bytes(64)
    before = ptaukeytest.violations()
    got = ptaukeytest.mul(1, pts, scalars, piece=16)                      # five pieces, the last one short
    for i, (a, s) in enumerate(zip(logs, scalars)):
        assert got[64 * i:64 * i + 64] == setuptest.mont1(G1.mul(a * s % R, G1.G) if a * s % R else None), (i, s)
    assert got == ptaukeytest.mul(1, pts, scalars) == ptaukeytest.mul(1, pts, [s + R for s in scalars[:-1]] + [scalars[-1]])    # one piece; reduced modulo r
    # every edge on one point
    one = setuptest.host_points(1, [logs[0]])
    got = ptaukeytest.mul(1, one * len(EDGES), EDGES)
    for i, s in enumerate(EDGES):
        assert got[64 * i:64 * i + 64] == setuptest.mont1(G1.mul(logs[0] * s % R, G1.G) if s else None), s
    assert ptaukeytest.violations() == before == 0
    bad = bytearray(pts)
    bad[64 * 33 + 3] ^= 1
    assert ptaukeytest.mul(1, bytes(bad), scalars, piece=16) is None


def test_host_multiplication_of_g2_points_equals_the_oracle():
    rng = random.Random(55)
    logs = [rng.randrange(1, R) for _ in range(35)]
    logs[3] = logs[34] = 0
    logs[4] = R - 1
    scalars = EDGES + [rng.randrange(R) for _ in range(35 - len(EDGES))]
    pts = setuptest.host_points(2, logs)
    before = ptaukeytest.violations()
    got = ptaukeytest.mul(2, pts, scalars, piece=8)
    for i, (a, s) in enumerate(zip(logs, scalars)):
        assert got[128 * i:128 * i + 128] == setuptest.mont2(G2.mul(a * s % R, G2.G2) if a * s % R else None), (i, s)
    assert got == ptaukeytest.mul(2, pts, scalars)
    assert ptaukeytest.violations() == before == 0
    bad = bytearray(pts)
    bad[128 * 20 + 70] ^= 1
    assert ptaukeytest.mul(2, bytes(bad), scalars) is None


def _sections(data):
    from zkwg import ptau
    sec = ptau.read_ptau(data, prepared=False)["sections"]
    return {sid: bytes(data[o:o + size]) for sid, (o, size) in sec.items()}


@pytest.fixture(scope="module")
def keys():
    rng = random.Random(56)
    return [tuple(rng.randrange(1, R) for _ in range(3)) for _ in range(2)]


@pytest.fixture(scope="module")
def chain(keys):
    """new(4) and two contributions on the host mirror, piece size 16"""
    from zkwg import ptau
    p0 = ptau.new(4)
    rc, msg, p1 = ptaukeytest.apply_key(p0, *keys[0], b"", piece=16)
    assert rc == 0, msg
    rc, msg, p2 = ptaukeytest.apply_key(p1, keys[1][0] + R, keys[1][1], keys[1][2], b"record", piece=16)       # (a key above r is reduced)
    assert rc == 0, msg
    return p0, p1, p2


def test_new_is_the_ceremony_of_ones():
    from zkwg import ptau
    p0 = ptau.new(4)
    assert p0 == ptautest.toy_ceremony(4, 1, 1, 1, setuptest.host_points)
    assert ptau.generators() == (setuptest.mont1(G1.G), setuptest.mont2(G2.G2))
    info = ptau.read_ptau(p0, prepared=False)
    assert (info["power"], info["ceremony_power"], info["sections"][7][1]) == (4, 4, 0)
    assert ptau.read_contributions(p0) == []
    assert ptau.current_challenge(p0) == hashlib.blake2b(b"".join(_sections(p0)[s] for s in (2, 3, 4, 5, 6)), digest_size=64).digest()
    with pytest.raises(ptau.PtauError):
        ptau.new(0)


def test_one_contribution_and_a_second_equal_the_toy_ceremony(chain, keys):
    p0, p1, p2 = chain
    assert ptaukeytest.violations() == 0
    (t1, a1, b1), (t2, a2, b2) = keys
    want1 = _sections(ptautest.toy_ceremony(4, t1, a1, b1, setuptest.host_points))
    want2 = _sections(ptautest.toy_ceremony(4, t1 * t2 % R, a1 * a2 % R, b1 * b2 % R, setuptest.host_points))
    got1, got2 = _sections(p1), _sections(p2)
    for sid in (1, 2, 3, 4, 5, 6):
        assert got1[sid] == want1[sid], sid
        assert got2[sid] == want2[sid], sid
    assert got1[7] == b"" and got2[7] == b"record"
    assert sorted(got2) == [1, 2, 3, 4, 5, 6, 7]
    # the sections are written in the order 1 .. 7, and the piece size does not show
    from zkwg import ptau
    assert list(ptau.read_ptau(p2, prepared=False)["sections"]) == [1, 2, 3, 4, 5, 6, 7] and struct.unpack_from("<I", p2, 8)[0] == 7
    assert ptaukeytest.apply_key(p0, *keys[0], b"", piece=1 << 20)[2] == p1 == ptaukeytest.apply_key(p0, *keys[0], b"", piece=5)[2]


def test_refusals(chain, keys):
    p0, p1, _ = chain
    k = keys[0]
    for bad in ((0, k[1], k[2]), (k[0], R, k[2]), (k[0], k[1], 2 * R)):
        rc, msg, _ = ptaukeytest.apply_key(p1, *bad)
        assert rc == -1 and "0 modulo" in msg, bad
    prepared = ptautest.prepare(p1)[2]
    rc, msg, _ = ptaukeytest.apply_key(prepared, *k)
    assert rc == -1 and "already prepared" in msg
    rc, msg, _ = ptaukeytest.apply_key(p1[:-9], *k)                       # (the empty section 7 is 12 bytes of table)
    assert rc == -1 and "truncated section table" in msg
    rc, msg, _ = ptaukeytest.apply_key(p1[:-30], *k)
    assert rc == -1 and "past the end" in msg
    rc, msg, _ = ptaukeytest.apply_key(p1[:40], *k)
    assert rc == -1 and "past the end" in msg
    rc, msg, _ = ptaukeytest.apply_key(b"ptbu" + p1[4:], *k)
    assert rc == -1 and "magic" in msg
    from zkwg import ptau
    sec = ptau.read_ptau(p1, prepared=False)["sections"]
    for sid in (2, 3, 4, 5, 6):
        b = bytearray(p1)
        b[sec[sid][0] + sec[sid][1] - 40] ^= 4
        rc, msg, _ = ptaukeytest.apply_key(bytes(b), *k)
        assert rc == -1 and "curve" in msg, sid
    assert ptaukeytest.violations() == 0


def _host_backend(monkeypatch):
    """zkwg.ptau's contribution with the device calls replaced by the host mirrors"""
    import torch
    from zkwg import phase2, prover, ptau
    monkeypatch.setattr(phase2, "scale_points", lambda group, pts, s, device=0: phase2test.scale(group, pts, s))
    monkeypatch.setattr(prover, "fixed_base", lambda device, group, scalars: torch.frombuffer(bytearray(setuptest.host_points(group, scalars)), dtype=torch.uint8))

    def apply_key(data, tau, alpha, beta, s7, device=0):
        rc, msg, out = ptaukeytest.apply_key(data, tau, alpha, beta, s7, piece=16)
        if rc != 0:
            raise ptau.PtauError(msg)
        return out
    monkeypatch.setattr(ptau, "apply_key", apply_key)


def _g1(b):
    v = [int.from_bytes(b[i:i + 32], "little") * pow(1 << 256, -1, Q) % Q for i in (0, 32)]
    return None if not any(b) else (v[0], v[1])


def _g2(b):
    v = [int.from_bytes(b[i:i + 32], "little") * pow(1 << 256, -1, Q) % Q for i in (0, 32, 64, 96)]
    return None if not any(b) else ((v[0], v[1]), (v[2], v[3]))


def test_records_round_trip_and_the_proofs_of_knowledge_hold_under_the_oracle_pairing(monkeypatch):
    from zkwg import phase2, ptau
    _host_backend(monkeypatch)
    rng = random.Random(57)
    blob = lambda n: bytes(rng.randrange(256) for _ in range(n))
    # the layout, byte for byte: the five points, three proofs, the next challenge, u32 length, tagged parameters
    names = ["tau_g1", "tau_g2", "alpha_g1", "beta_g1", "beta_g2", "tau_g1_s", "tau_g1_sx", "tau_g2_spx", "alpha_g1_s", "alpha_g1_sx", "alpha_g2_spx",
             "beta_g1_s", "beta_g1_sx", "beta_g2_spx"]
    assert [n for n, _ in ptau.RECORD_POINTS] == names
    r1 = {n: blob(size) for n, size in ptau.RECORD_POINTS}
    r1.update(next_challenge=blob(64), name="first")
    raw1 = ptau.pack_record(r1)
    assert raw1 == b"".join(r1[n] for n in names) + r1["next_challenge"] + (7).to_bytes(4, "little") + b"\x04\x05first" and len(raw1) == 3 * 64 + 2 * 128 + 3 * 256 + 64 + 4 + 7
    assert ptau.pack_section7([]) == b"" and ptau.pack_section7([raw1])[:4] == (1).to_bytes(4, "little")
    for cut in (ptau.pack_section7([raw1])[:-1], ptau.pack_section7([raw1]) + b"x", b"\x01\x00"):
        with pytest.raises(ptau.PtauError):
            ptau.read_contributions(cut)
    # a contribution and a beacon through zkwg.ptau itself
    p0 = ptau.new(3)
    seed = bytes(range(64))
    p1 = ptau.contribute(p0, "alice", "entropy", urandom=lambda n: seed[:n])
    p2 = ptau.beacon(p1, "the beacon", "0102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f20", 10)
    (t1, a1, b1), esses = ptau.key_scalars(seed + b"entropy")
    (t2, a2, b2), _ = ptau.key_scalars(phase2.beacon_seed(bytes(range(1, 33)), 10))
    assert len({t1, a1, b1, *esses}) == 6 and t1 == phase2.derive_scalar(seed + b"entropy", ptau.TAG_TAU)
    want1 = _sections(ptautest.toy_ceremony(3, t1, a1, b1, setuptest.host_points))
    want2 = _sections(ptautest.toy_ceremony(3, t1 * t2 % R, a1 * a2 % R, b1 * b2 % R, setuptest.host_points))
    for sid in (1, 2, 3, 4, 5, 6):
        assert _sections(p1)[sid] == want1[sid] and _sections(p2)[sid] == want2[sid], sid
    recs = ptau.read_contributions(p2)
    assert len(recs) == 2 and ptau.read_contributions(p1) == recs[:1] and ptau.read_contributions(_sections(p2)[7]) == recs
    assert (recs[0]["name"], recs[0]["type"], recs[1]["name"], recs[1]["type"], recs[1]["num_iterations_exp"]) == ("alice", None, "the beacon", 1, 10)
    assert recs[1]["beacon_hash"] == bytes(range(1, 33))
    assert ptau.pack_section7([r["raw"] for r in recs]) == _sections(p2)[7]
    # the five points are the file's, and the challenges chain over the points as stored
    challenge = ptau.current_challenge(p0)
    for before, after, rec, key in ((p0, p1, recs[0], (t1, a1, b1)), (p1, p2, recs[1], (t2, a2, b2))):
        s = _sections(after)
        assert (rec["tau_g1"], rec["tau_g2"], rec["alpha_g1"], rec["beta_g1"], rec["beta_g2"]) == (s[2][64:128], s[3][128:256], s[4][:64], s[5][:64], s[6])
        nxt = hashlib.blake2b(challenge + s[2] + s[3] + s[4] + s[5] + s[6], digest_size=64).digest()
        assert rec["next_challenge"] == nxt == ptau.current_challenge(after)
        neg = lambda p: None if p is None else (p[0], -p[1] % Q)
        for i, name in enumerate(ptau.KEYS):
            g1_s, g1_sx, spx = rec[f"{name}_g1_s"], rec[f"{name}_g1_sx"], _g2(rec[f"{name}_g2_spx"])
            sp = _g2(ptau.pok_challenge_point(challenge, i, g1_s, g1_sx))
            assert G2.on_curve(sp) and G2.mul(R, sp) is None and spx == G2.mul(key[i], sp)
            assert P.pairing_product_is_one([(_g1(g1_s), spx), (neg(_g1(g1_sx)), sp)]), name
            if name == "tau":                                             # the same tau moved the file: tauG1 before / after
                b1_, a1_ = _g1(_sections(before)[2][64:128]), _g1(rec["tau_g1"])
                assert P.pairing_product_is_one([(b1_, spx), (neg(a1_), sp)])
                assert not P.pairing_product_is_one([(b1_, spx), (neg(_g1(g1_s)), sp)])
        challenge = nxt
