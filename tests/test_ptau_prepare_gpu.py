"""`powersoftau prepare phase2` on the device (zkwg.ptau.prepare -> zkwg_ptau_prepare / zkwg_group_ntt_device ->
csrc/zkwg_kernels_ptau.hip): the transform over points against known logarithms and the host mirror, a power-9 file against the host
mirror in every byte, and the workflow an unprepared ceremony starts:  prepare -> setup.new_zkey -> phase 2 -> prove.

Two facts shape the end-to-end tests.  Level q <= power of a prepared file is the inverse transform of
(tau^k G), which IS (L_j(tau) G) of groth16.lagrange_at -- so with the circuit's power BELOW the file's, the new key equals the trapdoor
key of tests/setuptest.py in every byte.  Level power + 1 of section 12 is computed without tau^(2 n - 1), which a file of that power
does not hold: with the circuit's power EQUAL to the file's, section 9 differs from the trapdoor key (entry j by
tau^(2 n - 1) w^(2 j + 1) / (2 n) times G) and the key is still a valid one, because the quotient's degree is at most 2 n - 2: its proofs
are accepted by the PINNED verifier (oracle/pyref/bn254_pairing.py).  All comparisons are exact.

GPU time of this file: 20 s (5 passed; profiles/r09/README.md) -- budget 120 s like tests/test_phase2_gpu.py; the longest test is the
host mirror's side of the power-9 comparison (12 s of CPU)."""
import json
import random

import pytest

import ptautest
import setuptest
import zkeytest
from oracle.pyref import bn254_pairing as P
from oracle.pyref import groth16 as G
from oracle.pyref import ntt

R = G.R


def _gpu_points(group, scalars):
    from zkwg import prover
    return bytes(prover.fixed_base(0, group, scalars).cpu().numpy())


@pytest.fixture(scope="module")
def world():
    """the seeded system (power 8), its trapdoor key, and unprepared ceremonies of power 9 and 8 from the key's own (tau, alpha, beta)"""
    from zkwg import r1cs as zr
    n_public = 4
    n_wires, cons, w = setuptest.system(seed=33, n_in=24, n_public=n_public, n_cons=220, degrees=[(20, 70)])
    assert setuptest.satisfied(cons, w)
    key = setuptest.toy_key(n_wires, n_public, cons, seed=9)
    assert key.power == 8
    r1cs = zr.write_r1cs(n_wires, cons, n_pub_out=2, n_pub_in=2, n_prv_in=20)
    pot9 = ptautest.toy_ceremony(9, key.tau, key.alpha, key.beta, _gpu_points, ceremony_power=12, contributions=b"seven")
    pot8 = ptautest.toy_ceremony(8, key.tau, key.alpha, key.beta, _gpu_points)
    return {"n_public": n_public, "n_wires": n_wires, "cons": cons, "w": w, "key": key, "r1cs": r1cs, "pot9": pot9, "pot8": pot8}


@pytest.mark.gpu
def test_gpu_group_ntt_equals_the_known_logarithms_and_the_host_mirror():
    from zkwg import ptau
    rng = random.Random(41)
    for group, L, pt in ((1, 12, 64), (2, 10, 128)):
        n = 1 << L
        logs = [rng.randrange(1, R) for _ in range(n)]
        logs[0] = logs[77] = logs[n - 1] = 0                                    # infinity, the first and the last point included
        logs[5] = logs[4]                                                       # equal and opposite points
        logs[7] = R - logs[6]
        pts = _gpu_points(group, logs)
        inv = ptau.group_ntt(group, pts, True)
        assert inv == _gpu_points(group, ntt.ifft_fast(logs)), group           # every byte
        assert ptau.group_ntt(group, pts, False) == _gpu_points(group, ntt.fft_fast(logs)), group
        assert ptau.group_ntt(group, inv, False) == pts, group                  # forward o inverse
        sub = pts[:pt << 8]
        for inverse in (True, False):
            assert ptau.group_ntt(group, sub, inverse) == ptautest.ntt(group, sub, inverse), (group, inverse)
        # tau = 1: all inputs equal, every output but the first is infinity; and a root of unity: one other output is not
        ones = _gpu_points(group, [1] * n)
        assert ptau.group_ntt(group, ones, True) == ones[:pt] + bytes(pt * (n - 1))
        w = ntt.root(L)
        got = ptau.group_ntt(group, _gpu_points(group, [pow(w, 3 * k, R) for k in range(n)]), True)
        assert got == bytes(pt * 3) + ones[:pt] + bytes(pt * (n - 4))
        assert ptau.group_ntt(group, pts[:pt], True) == pts[:pt] and ptau.group_ntt(group, pts[pt:2 * pt], False) == pts[pt:2 * pt]
        bad = bytearray(pts)
        bad[pt * (n - 2) + 5] ^= 1
        with pytest.raises(ptau.PtauError, match="curve"):
            ptau.group_ntt(group, bytes(bad), True)
    assert ptautest.violations() == 0


@pytest.mark.gpu
def test_gpu_prepare_of_a_power_9_file_equals_the_host_mirror(world):
    from zkwg import ptau
    got = ptau.prepare(world["pot9"])
    rc, msg, want = ptautest.prepare(world["pot9"])
    assert rc == 0, msg
    assert got == want                                                          # every byte of the file
    info = ptau.read_ptau(got)
    assert (info["power"], info["ceremony_power"]) == (9, 12) and sorted(info["sections"]) == [1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15]
    src = ptau.read_ptau(world["pot9"], prepared=False)
    for sid in range(1, 8):
        (o, n), (o2, n2) = info["sections"][sid], src["sections"][sid]
        assert got[o:o + n] == world["pot9"][o2:o2 + n2], sid
    st = ptau.last_stats()
    assert all(v["add"] > 0 and v["dbl"] > v["add"] and v["transforms"] > 0 for v in st.values())
    assert ptau.prepare(world["pot9"], 8) == ptau.prepare(ptau.truncate(world["pot9"], 8))
    bad = bytearray(world["pot9"])
    bad[src["sections"][3][0] + 128 * 511 + 70] ^= 2                           # the last point of section 3
    with pytest.raises(ptau.PtauError, match="curve"):
        ptau.prepare(bytes(bad))
    with pytest.raises(ptau.PtauError, match="already prepared"):
        ptau.prepare(got)
    with pytest.raises(ptau.PtauError, match="above"):
        ptau.prepare(world["pot9"], 10)
    assert ptautest.violations() == 0


def _prove_and_verify(z, world, vk=None):
    from zkwg import prover, zkey
    w, n_public = world["w"], world["n_public"]
    vk = vk or zkey.verification_key(z)
    wp = prover.WitnessProver(z, device=0, slots=2)
    st, proofs = wp.prove(zkeytest.wit_bytes(w), [(12345, 67890)])
    assert st == [0]
    pub = wp.public_signals(zkeytest.wit_bytes(w))
    assert pub == [str(w[i]) for i in range(1, n_public + 1)]
    pj = prover.Prover.proof_json(proofs[0])
    assert P.groth16_verify(vk, pub, pj)
    bad = list(pub)
    bad[1] = str((int(bad[1]) + 1) % R)
    assert not P.groth16_verify(vk, bad, pj)
    del wp


@pytest.mark.gpu
def test_gpu_prepare_then_setup_equals_the_trapdoor_key_when_the_file_is_larger_than_the_circuit(world):
    from zkwg import ptau, setup
    z = setup.new_zkey(world["r1cs"], ptau.prepare(world["pot9"]))
    got, d = setuptest.zkey_sections(z)
    want = setuptest.toy_sections(world["key"], _gpu_points)
    assert (d["n_vars"], d["n_public"], d["domain_size"]) == (world["n_wires"], world["n_public"], 256)
    for name in (3, 5, 6, 7, 8, 9, "alpha1", "beta1", "beta2", "gamma2", "delta1", "delta2"):
        assert got[name] == want[name], name


@pytest.mark.gpu
def test_gpu_prepare_then_setup_at_the_files_own_power_gives_another_valid_key(world):
    from zkwg import ptau, setup
    key = world["key"]
    z = setup.new_zkey(world["r1cs"], ptau.prepare(world["pot8"]))
    got, d = setuptest.zkey_sections(z)
    want = setuptest.toy_sections(key, _gpu_points)
    for name in (3, 5, 6, 7, 8, "alpha1", "beta1", "beta2", "gamma2", "delta1", "delta2"):
        assert got[name] == want[name], name
    assert got[9] != want[9]
    # section 9 is what the derivation says: H_j = L'_(2 j + 1)(tau) - tau^(2 n - 1) w^(2 j + 1) / (2 n), w the 2 n-th root of unity
    n, w = key.n, ntt.root(key.power + 1)
    top = pow(key.tau, 2 * n - 1, R) * pow(2 * n, -1, R) % R
    assert got[9] == _gpu_points(1, [(key.h_key[j] - top * pow(w, 2 * j + 1, R)) % R for j in range(n)])
    _prove_and_verify(z, world, G.vkey_json(key))


@pytest.mark.gpu
def test_gpu_the_command_lines_in_a_row(world, tmp_path, capsys):
    from zkwg import phase2, prove, ptau, setup, wtns, zkey
    f = lambda name: str(tmp_path / name)
    open(f("c.r1cs"), "wb").write(world["r1cs"])
    open(f("pot.ptau"), "wb").write(world["pot9"])
    open(f("w.wtns"), "wb").write(wtns.write_wtns(zkeytest.wit_bytes(world["w"])))
    assert setup.main([f("c.r1cs"), f("pot.ptau"), f("no.zkey")]) == 1          # unprepared: refused as before, now with the way out
    err = capsys.readouterr().err
    assert "Powers of tau is not prepared" in err and "zkwg.ptau prepare" in err
    assert ptau.main(["prepare", f("pot.ptau"), f("pot_final.ptau"), "--power", "8"]) == 0
    assert ptau.main(["info", f("pot_final.ptau")]) == 0
    assert "power 8, ceremony power 12, prepared" in capsys.readouterr().out
    assert ptau.main(["prepare", f("pot_final.ptau"), f("x.ptau")]) == 1
    assert ptau.main(["prepare", f("w.wtns"), f("x.ptau")]) == 1
    assert setup.main([f("c.r1cs"), f("pot_final.ptau"), f("c_0000.zkey")]) == 0
    assert phase2.main(["contribute", f("c_0000.zkey"), f("c_0001.zkey"), "--name", "cli", "--entropy", "some text"]) == 0
    assert prove.main([f("c_0001.zkey"), f("w.wtns"), f("proof.json"), f("public.json")]) == 0
    proof, public = json.load(open(f("proof.json"))), json.load(open(f("public.json")))
    z1 = open(f("c_0001.zkey"), "rb").read()
    assert P.groth16_verify(zkey.verification_key(z1), public, proof)
    assert not P.groth16_verify(zkey.verification_key(open(f("c_0000.zkey"), "rb").read()), public, proof)
