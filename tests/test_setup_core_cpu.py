"""The groth16 set-up on the CPU: the host build of csrc/zkwg_setup_core.h (tests/native/setuptest.cpp -- the plans, the per-lane sums
and the conversion to affine points that the kernels of csrc/zkwg_kernels_setup.hip compile) makes, from the toy powers of a known
(tau, alpha, beta), the key oracle/pyref/groth16.py makes from the same trapdoor with gamma = delta = 1: every byte of sections 3, 5 - 9
and of the header points, section 4 as a sorted list, and no violated limb-form bound.  Reference workflow:
docs/zk-email-docs/UsageGuide/README.md:145-180 (`snarkjs groth16 setup`).  All comparisons are exact."""
import random

import pytest

import setuptest
import zkeytest
from oracle.pyref import bn254_g1 as G1
from oracle.pyref import bn254_g2 as G2

R = setuptest.R


@pytest.fixture(scope="module")
def small():
    """102 wires, 90 constraints, 3 public wires: a 2^7 domain.  Wire 0 is in A of 80 constraints, wire 5 in B of 70, wire 6 in A / B / C
    of 72: the wavefront path of every sum runs (more than ZK_SETUP_LONG = 64 terms)."""
    n_public = 3
    n_wires, cons, w = setuptest.system(seed=5, n_in=12, n_public=n_public, n_cons=90, heavy={0: (80, (0,)), 5: (70, (1,)), 6: (72, (0, 1, 2))})
    key = setuptest.toy_key(n_wires, n_public, cons, seed=77)
    return n_public, n_wires, cons, w, key


def test_the_system_is_what_the_docstring_says(small):
    n_public, n_wires, cons, w, key = small
    lib = setuptest.load()
    assert n_wires == 102 and key.power == 7 and setuptest.satisfied(cons, w)
    assert lib.st_long_threshold() == 64
    assert setuptest.wire_degree(cons, 0) > 64 and setuptest.wire_degree(cons, 5) > 64 and setuptest.wire_degree(cons, 6) > 64
    assert sum(1 for a, _, _ in cons if 0 in a) > 64 and sum(1 for _, b, _ in cons if 5 in b) > 64
    # every class of coefficient in every matrix
    classes = lambda v: "one" if v == 1 else "minus" if v == R - 1 else "small" if v < 1000 else "pow2" if v & (v - 1) == 0 else \
        "negpow2" if (R - v) & (R - v - 1) == 0 else "uniform"
    for m in range(3):
        assert {classes(v) for row in cons for v in row[m].values()} == {"one", "minus", "small", "pow2", "negpow2", "uniform"}, m


def test_host_multiply_is_pinned_to_the_oracle():
    rng = random.Random(3)
    ks = [1, 2, R - 1, rng.randrange(R), rng.randrange(R), 0]
    got = setuptest.host_points(1, ks)
    for i, k in enumerate(ks):
        assert got[64 * i:64 * i + 64] == setuptest.mont1(G1.mul(k, G1.G)), k
    ks2 = [1, R - 1, rng.randrange(R), 0]
    got = setuptest.host_points(2, ks2)
    for i, k in enumerate(ks2):
        assert got[128 * i:128 * i + 128] == setuptest.mont2(G2.mul(k, G2.G2)), k


def test_host_setup_equals_the_oracle_key_byte_for_byte(small):
    from zkwg import r1cs as zr
    n_public, n_wires, cons, w, key = small
    lib = setuptest.load()
    slices = setuptest.toy_slices(key, setuptest.host_points)
    # the toy ceremony itself: slice points against the oracle's multiplication
    s = setuptest.toy_slice_scalars(key)
    for j in (0, 1, 93, 127):
        assert slices["tau_g1"][64 * j:64 * j + 64] == setuptest.mont1(G1.mul(s["tau"][j], G1.G))
    assert slices["beta_tau_g1"][64 * 5:64 * 6] == setuptest.mont1(G1.mul(s["beta_tau"][5], G1.G))
    assert slices["alpha_tau_g1"][64 * 6:64 * 7] == setuptest.mont1(G1.mul(s["alpha_tau"][6], G1.G))
    assert slices["tau_g1_next"][64 * 255:64 * 256] == setuptest.mont1(G1.mul(s["next"][255], G1.G))
    assert slices["tau_g2"][128 * 9:128 * 10] == setuptest.mont2(G2.mul(s["tau"][9], G2.G2))
    r1cs = zr.write_r1cs(n_wires, cons, n_pub_out=1, n_pub_in=n_public - 1, n_prv_in=12 - n_public)
    before = lib.st_violations()
    rc, msg, z, info = setuptest.host_new_zkey(r1cs, slices)
    assert rc == 0, msg
    assert lib.st_violations() == before == 0
    assert info[4] >= 1 and info[5] >= 1 and info[6] >= 3, info            # wavefront work items in A, B and K
    got, d = setuptest.zkey_sections(z)
    want = setuptest.toy_sections(key, setuptest.host_points)
    assert (d["n_vars"], d["n_public"], d["domain_size"]) == (n_wires, n_public, 128)
    for name in (5, 6, 7, 3, 8, 9, "alpha1", "beta1", "beta2", "gamma2", "delta1", "delta2"):
        assert got[name] == want[name], name
    assert want[6].count(bytes(64)) > 0 and all((want[6][64 * i:64 * i + 64] == bytes(64)) == (want[7][128 * i:128 * i + 128] == bytes(128)) for i in range(n_wires))
    assert sorted(d["coeffs"]) == sorted(zkeytest.section4(cons, n_public))
    # spot checks of the key's points by the oracle's own multiplication
    assert got[5][:64] == setuptest.mont1(G1.mul(key.a_tau[0], G1.G)) and got[7][128 * 5:128 * 6] == setuptest.mont2(G2.mul(key.b_tau[5], G2.G2))
    assert got[3][64:128] == setuptest.mont1(G1.mul(key.ic[1], G1.G)) and got[9][64 * 17:64 * 18] == setuptest.mont1(G1.mul(key.h_key[17], G1.G))
    # the zkey readers of the prover accept the file
    zt = zkeytest.load()
    import ctypes as C
    zinfo = (C.c_uint64 * 4)()
    assert zt.zt_zkey_check(z, len(z), zinfo) == 0 and list(zinfo)[:3] == [n_wires, n_public, len(cons) + n_public + 1]


def test_verification_key_and_a_proof_from_the_new_key_verify(small):
    """zkey.verification_key(new key) is the oracle's vkey_json, and a proof assembled from the oracle's scalars under this key is accepted"""
    from zkwg import r1cs as zr, zkey
    from oracle.pyref import bn254_pairing as P
    from oracle.pyref import groth16 as G
    n_public, n_wires, cons, w, key = small
    r1cs = zr.write_r1cs(n_wires, cons, n_pub_out=1, n_pub_in=n_public - 1, n_prv_in=12 - n_public)
    rc, msg, z, _ = setuptest.host_new_zkey(r1cs, setuptest.toy_slices(key, setuptest.host_points))
    assert rc == 0, msg
    vk = zkey.verification_key(z)
    assert vk == G.vkey_json(key)
    sc = G.prove_scalars(key, cons, w, 1234567, 7654321)
    pub = [str(w[i]) for i in range(1, n_public + 1)]
    assert P.groth16_verify(vk, pub, G.proof_json(sc))
    bad = list(pub)
    bad[0] = str((int(bad[0]) + 1) % R)
    assert not P.groth16_verify(vk, bad, G.proof_json(sc))


def test_r1cs_refusals():
    from zkwg import r1cs as zr
    n_wires, cons, w = setuptest.system(seed=1, n_in=4, n_public=1, n_cons=3)
    key = setuptest.toy_key(n_wires, 1, cons, seed=2)
    slices = setuptest.toy_slices(key, setuptest.host_points)
    good = zr.write_r1cs(n_wires, cons, n_pub_out=1, n_prv_in=2)
    assert setuptest.host_new_zkey(good, slices)[0] == 0
    # nPublic + 1 >= nVars
    rc, msg, z, _ = setuptest.host_new_zkey(zr.write_r1cs(n_wires, cons, n_pub_out=n_wires - 1), slices)
    assert rc == -1 and "nPublic" in msg
    # what the .r1cs reader refuses
    rc, msg, z, _ = setuptest.host_new_zkey(good[:len(good) - 5], slices)
    assert rc == -1 and z is None
    rc, msg, z, _ = setuptest.host_new_zkey(b"r1cx" + good[4:], slices)
    assert rc == -1 and "magic" in msg
    # slices of another power
    other = dict(slices, power=slices["power"] + 1)
    assert setuptest.host_new_zkey(good, other)[0] == -1
    # a slice point off its curve / not reduced
    for name in ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "tau_g1_next"):
        b = bytearray(slices[name])
        b[70] ^= 1
        rc, msg, z, _ = setuptest.host_new_zkey(good, dict(slices, **{name: bytes(b)}))
        assert rc == -1 and "curve" in msg, name
    b = bytearray(slices["tau_g1"])
    b[:32] = (int.from_bytes(b[:32], "little") + setuptest.Q).to_bytes(32, "little")       # the same x mod q, not reduced
    rc, msg, z, _ = setuptest.host_new_zkey(good, dict(slices, tau_g1=bytes(b)))
    assert rc == -1 and "curve" in msg
