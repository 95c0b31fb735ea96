"""Phase 2 on the CPU: the host build of csrc/zkwg_phase2_core.h (tests/native/phase2test.cpp -- the recoder, the digit walk a lane of
zk_phase2_scale runs, the set-up's conversion to affine points and the file operation over them) against the oracle's group arithmetic
(oracle/pyref/bn254_g1.py, bn254_g2.py) and against the toy key of a known trapdoor (tests/setuptest.py); the record of section 10 and
the scalar derivation of zkwg/phase2.py.  Reference workflow: docs/zk-email-docs/UsageGuide/README.md:149,178-180 ("Phase 2").  All
comparisons are exact, and no limb-form bound is violated."""
import copy
import hashlib
import random

import pytest

import phase2test
import setuptest
import zkeytest
from oracle.pyref import bn254_g1 as G1
from oracle.pyref import bn254_g2 as G2

R, Q = setuptest.R, setuptest.Q
COFACTOR = 2 * Q - R
EDGES = [1, 2, 3, R - 1, 1 << 253, (1 << 255) + 1, COFACTOR]


def test_recoding_is_the_non_adjacent_form():
    rng = random.Random(11)
    scalars = EDGES + [0, R, R + 1, (1 << 256) - 1, (1 << 256) - 2, int("aa" * 32, 16), int("55" * 32, 16)] + \
        [rng.randrange(1 << rng.choice([8, 64, 200, 254, 256])) for _ in range(300)]
    for s in scalars:
        d = phase2test.recode(s)
        assert sum(x << i for i, x in enumerate(d)) == s, s
        assert set(d) <= {-1, 0, 1}
        assert all(d[i] == 0 or d[i + 1] == 0 for i in range(len(d) - 1)), s
        assert len(d) <= 257 and (not d or d[-1] == 1)
    # a third of the positions on average
    dens = [sum(1 for x in phase2test.recode(rng.randrange(R)) if x) for _ in range(200)]
    assert 75 < sum(dens) / len(dens) < 95


def _dbl_add(add, k, p):
    """k p for the INTEGER k over the oracle's addition (oracle mul reduces k modulo r, which is wrong outside the subgroup)"""
    acc = None
    for bit in bin(k)[2:]:
        acc = add(acc, acc)
        if bit == "1":
            acc = add(acc, p)
    return acc


def test_host_scaling_of_g1_points_equals_the_oracle():
    rng = random.Random(12)
    logs = [rng.randrange(1, R) for _ in range(203)]
    logs[7] = logs[100] = logs[202] = 0                       # infinity among them, the last point included
    logs[8], logs[9] = 1, R - 1
    pts = setuptest.host_points(1, logs)
    assert pts[64 * 7:64 * 8] == bytes(64)
    before = phase2test.violations()
    for s in (R - 1, rng.randrange(R), 3):
        got = phase2test.scale(1, pts, s)
        for i, a in enumerate(logs):
            assert got[64 * i:64 * i + 64] == setuptest.mont1(G1.mul(a * s % R, G1.G) if a * s % R else None), (s, i)
    # scalars at and above the group order (the chain meets P = +-Q at its last steps), 0, and the 256-bit edges: sampled points
    few = pts[64 * 5:64 * 12]
    for s in (0, R, R + 1, R - 2, (1 << 255) + 1, (1 << 256) - 1, COFACTOR):
        got = phase2test.scale(1, few, s)
        for i, a in enumerate(logs[5:12]):
            assert got[64 * i:64 * i + 64] == setuptest.mont1(G1.mul(a * s % R, G1.G) if a * s % R else None), (s, i)
    assert phase2test.violations() == before == 0
    # a point off the curve, a word that is not reduced: refused
    bad = bytearray(pts)
    bad[64 * 50 + 3] ^= 1
    assert phase2test.scale(1, bytes(bad), 5) is None
    assert phase2test.scale(1, Q.to_bytes(32, "little") + bytes(32), 5) is None


def _twist_point(rng):
    """a point of the twist y^2 = x^3 + 3 / (9 + i) that is NOT in the subgroup of order r"""
    from zkwg import phase2
    while True:
        x = (rng.randrange(Q), rng.randrange(Q))
        y = phase2._f2_sqrt(G2.f2_add(G2.f2_mul(G2.f2_mul(x, x), x), G2.B2))
        if y is None:
            continue
        p = (x, y)
        assert G2.on_curve(p)
        if _dbl_add(G2.add, R, p) is not None:
            return p


def test_host_scaling_of_g2_points_equals_the_oracle_and_clears_the_cofactor():
    rng = random.Random(13)
    logs = [rng.randrange(1, R) for _ in range(52)]
    logs[3] = logs[51] = 0
    logs[4] = R - 1
    pts = setuptest.host_points(2, logs)
    before = phase2test.violations()
    for s in (R - 1, rng.randrange(R)):
        got = phase2test.scale(2, pts, s)
        for i, a in enumerate(logs):
            assert got[128 * i:128 * i + 128] == setuptest.mont2(G2.mul(a * s % R, G2.G2) if a * s % R else None), (s, i)
    got = phase2test.scale(2, pts[:128 * 6], R)
    assert got == bytes(128 * 6)
    # the cofactor on points outside the subgroup: the integer multiple, which then has order r
    outside = [_twist_point(rng) for _ in range(5)]
    raw = b"".join(setuptest.mont2(p) for p in outside) + bytes(128)
    got = phase2test.scale(2, raw, COFACTOR)
    for i, p in enumerate(outside):
        want = _dbl_add(G2.add, COFACTOR, p)
        assert want is not None and _dbl_add(G2.add, R, want) is None
        assert got[128 * i:128 * i + 128] == setuptest.mont2(want), i
    assert got[128 * 5:] == bytes(128)
    got3 = phase2test.scale(2, raw, 3)                               # a small integer multiple outside the subgroup
    assert got3[:128] == setuptest.mont2(G2.add(G2.add(outside[0], outside[0]), outside[0]))
    assert phase2test.violations() == before == 0
    bad = bytearray(pts)
    bad[128 * 20 + 70] ^= 2
    assert phase2test.scale(2, bytes(bad), 5) is None


@pytest.fixture(scope="module")
def toy():
    from zkwg import zkey
    n_public = 3
    n_wires, cons, w = setuptest.system(seed=6, n_in=12, n_public=n_public, n_cons=40)
    key = setuptest.toy_key(n_wires, n_public, cons, seed=78)
    sec = setuptest.toy_sections(key, setuptest.host_points)
    z = zkey.write_zkey(n_wires, n_public, key.n, {k: sec[k] for k in ("alpha1", "beta1", "beta2", "gamma2", "delta1", "delta2")},
                        sec[3], sec[5], sec[6], sec[7], sec[8], sec[9], zkeytest.section4(cons, n_public))
    return key, z


def _expected(key, delta):
    """the sections of the toy key after contributions whose scalars multiply to delta"""
    k2 = copy.copy(key)
    inv = pow(delta, -1, R)
    k2.c_key = [x * inv % R for x in key.c_key]
    k2.h_key = [x * inv % R for x in key.h_key]
    want = setuptest.toy_sections(k2, setuptest.host_points)
    want["delta1"], want["delta2"] = setuptest.host_points(1, [delta]), setuptest.host_points(2, [delta])
    return want


def test_host_apply_delta_equals_the_trapdoor_key_section_by_section(toy):
    from zkwg import zkey
    key, z = toy
    rng = random.Random(14)
    k1, k2 = rng.randrange(1, R), rng.randrange(1, R)
    s10 = bytes(range(64)) + b"\x00\x00\x00\x00"
    before = phase2test.violations()
    rc, msg, z1 = phase2test.apply_delta(z, k1, s10)
    assert rc == 0, msg
    rc, msg, z2 = phase2test.apply_delta(z1, k2 + R, s10 + b"tail")          # (a scalar above r is reduced)
    assert rc == 0, msg
    assert phase2test.violations() == before == 0
    d0 = zkey.read_zkey(z)
    for zz, delta, tail in ((z1, k1, s10), (z2, k1 * k2 % R, s10 + b"tail")):
        got, d = setuptest.zkey_sections(zz)
        want = _expected(key, delta)
        for name in (3, 5, 6, 7, 8, 9, "alpha1", "beta1", "beta2", "gamma2", "delta1", "delta2"):
            assert got[name] == want[name], name
        for name in ("ic", "a", "b1", "b2", "coeffs", "n_vars", "n_public", "domain_size"):
            assert d[name] == d0[name], name                   # sections 3 - 7 bit for bit
        assert d["section10"] == tail
        assert got[8] != setuptest.zkey_sections(z)[0][8] and got[9] != setuptest.zkey_sections(z)[0][9]
        sec_in, sec_out = zkey.sections(z), zkey.sections(zz)
        assert z[sec_in[4][0]:sec_in[4][0] + sec_in[4][1]] == zz[sec_out[4][0]:sec_out[4][0] + sec_out[4][1]]
        assert zkey.verification_key(zz)["vk_delta_2"] == [[str(v) for v in c] for c in G2.mul(delta, G2.G2)] + [["1", "0"]]
    # refusals: k = 0 mod r, a truncated key, a corrupted point of section 8 and of section 9
    for k in (0, R):
        rc, msg, _ = phase2test.apply_delta(z, k, s10)
        assert rc == -1 and "0 modulo" in msg
    rc, msg, _ = phase2test.apply_delta(z[:-9], k1, s10)
    assert rc == -1 and "truncated" in msg
    sec = zkey.sections(z)
    for sid in (8, 9):
        b = bytearray(z)
        b[sec[sid][0] + sec[sid][1] - 40] ^= 4
        rc, msg, _ = phase2test.apply_delta(bytes(b), k1, s10)
        assert rc == -1 and "curve" in msg, sid
    assert phase2test.apply_delta(z, k1, s10)[2] == z1


def test_section10_round_trip_and_the_beacon_record(toy):
    from zkwg import phase2, zkey
    key, z = toy
    assert phase2.read_contributions(z) == (bytes(64), [])
    rng = random.Random(15)
    blob = lambda n: bytes(rng.randrange(256) for _ in range(n))
    r1 = {"delta_after": blob(64), "g1_s": blob(64), "g1_sx": blob(64), "g2_spx": blob(128), "transcript": blob(64), "name": "first"}
    r2 = dict(r1, delta_after=blob(64), name="the beacon", type=phase2.TYPE_BEACON, num_iterations_exp=10, beacon_hash=blob(32))
    raw1, raw2 = phase2.pack_record(r1), phase2.pack_record(r2)
    # the layout, byte for byte: points, transcript, u32 length, tagged parameters
    assert raw1 == r1["delta_after"] + r1["g1_s"] + r1["g1_sx"] + r1["g2_spx"] + r1["transcript"] + (7).to_bytes(4, "little") + b"\x04\x05first"
    assert raw2[384:] == (4 + 34 + 12).to_bytes(4, "little") + b"\x01\x01\x02\x0a\x03\x20" + r2["beacon_hash"] + b"\x04\x0athe beacon"
    chash = blob(64)
    s10 = phase2.pack_section10(chash, [raw1, raw2])
    assert s10[:68] == chash + (2).to_bytes(4, "little")
    d = zkey.read_zkey(z)
    z2 = zkey.write_zkey(d["n_vars"], d["n_public"], d["domain_size"], d, d["ic"], d["a"], d["b1"], d["b2"], d["c"], d["h"], d["coeffs"], section10=s10)
    assert zkey.write_zkey(d["n_vars"], d["n_public"], d["domain_size"], d, d["ic"], d["a"], d["b1"], d["b2"], d["c"], d["h"], d["coeffs"]) == z
    got_hash, recs = phase2.read_contributions(z2)
    assert got_hash == chash and len(recs) == 2 and phase2.read_contributions(s10) == (got_hash, recs)
    for want, got, raw in ((r1, recs[0], raw1), (r2, recs[1], raw2)):
        assert got["raw"] == raw
        for f in ("delta_after", "g1_s", "g1_sx", "g2_spx", "transcript"):
            assert got[f] == want[f]
        for _, f, _ in phase2.PARAMS:
            assert got[f] == want.get(f), f
    assert (recs[1]["type"], recs[1]["num_iterations_exp"], recs[1]["beacon_hash"]) == (1, 10, r2["beacon_hash"])
    assert recs[0]["type"] is None and recs[0]["beacon_hash"] is None
    for cut in (s10[:-1], s10[:70], s10 + b"x"):
        with pytest.raises(phase2.Phase2Error):
            phase2.read_contributions(cut)


def test_derive_scalar_and_the_beacon_chain():
    from zkwg import phase2
    a = phase2.derive_scalar(b"seed")
    assert a == phase2.derive_scalar(b"seed") and 0 < a < R
    assert a == int.from_bytes(hashlib.blake2b(phase2.TAG_SCALAR + b"seed", digest_size=64).digest(), "little") % R
    seen = {phase2.derive_scalar(bytes([i])) for i in range(64)}
    assert len(seen) == 64 and all(0 < k < R for k in seen)
    assert phase2.contribution_scalars(b"seed")[0] == a and phase2.contribution_scalars(b"seed")[1] not in (a, 0)
    h = b"\x01" * 32
    for _ in range(1 << 10):
        h = hashlib.sha256(h).digest()
    assert phase2.beacon_seed(b"\x01" * 32, 10) == h
    # Fq2 roots through the norm: squares have one, and the root squares back
    rng = random.Random(16)
    for _ in range(20):
        x = (rng.randrange(Q), rng.choice([0, rng.randrange(Q)]))
        sq = G2.f2_mul(x, x)
        y = phase2._f2_sqrt(sq)
        assert y is not None and G2.f2_mul(y, y) == sq
    assert phase2._B2 == G2.B2
