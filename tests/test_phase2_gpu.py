"""Phase 2 on the device (zkwg.phase2 -> zkwg_zkey_apply_delta / zkwg_point_scale_device -> csrc/zkwg_kernels_phase2.hip): the seeded
5,200-constraint system of tests/test_setup_gpu.py goes through  setup.new_zkey -> phase2.contribute -> phase2.beacon;  after each step
EVERY byte of sections 8 and 9 and of delta1, delta2 equals the key of the same trapdoor with delta = the product of the derived scalars
(bases through prover.fixed_base), sections 3 - 7 are untouched, and a proof under the contributed key is accepted by the PINNED verifier
(oracle/pyref/bn254_pairing.py) with the new verification key and rejected with the initial one.  The record of section 10 checks out
under the oracle pairing.  Reference workflow: docs/zk-email-docs/UsageGuide/README.md:149,178-180,206.  All comparisons are exact.

GPU time of this file: 18 s (4 passed; profiles/r08/README.md) -- budget 120 s like tests/test_setup_gpu.py; one G.setup of the
5,200-constraint system, shared by every test through the module fixture; the longest test is the host mirror's side of the
zkwg_point_scale_device comparison (12 s of CPU)."""
import copy
import json
import random

import pytest

import phase2test
import setuptest
import zkeytest
from oracle.pyref import bn254_g1 as G1
from oracle.pyref import bn254_g2 as G2
from oracle.pyref import bn254_pairing as P
from oracle.pyref import groth16 as G

R, Q = G.R, setuptest.Q
COFACTOR = 2 * Q - R
URANDOM = lambda n: bytes(range(n))
ENTROPY = "fixed entropy"
BEACON_HASH, BEACON_EXP = "0102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f20", 10


def _gpu_points(group, scalars):
    from zkwg import prover
    return bytes(prover.fixed_base(0, group, scalars).cpu().numpy())


def _expected(key, delta):
    """the sections of the trapdoor key with delta in place of 1: C and H times 1 / delta"""
    k2 = copy.copy(key)
    inv = pow(delta, -1, R)
    k2.c_key = [x * inv % R for x in key.c_key]
    k2.h_key = [x * inv % R for x in key.h_key]
    k2.delta = delta
    want = setuptest.toy_sections(k2, _gpu_points)
    want["delta1"], want["delta2"] = _gpu_points(1, [delta]), _gpu_points(2, [delta])
    return want, k2


@pytest.fixture(scope="module")
def chain():
    """the seeded system, its trapdoor key (ONE G.setup), the initial key and the keys after a contribution and a beacon"""
    from zkwg import phase2, prover, r1cs as zr, setup
    n_public = 4
    heavy = {0: (4500, (0, 1, 2)), 3: (4300, (0,)), 4: (4200, (1,)), 5: (4100, (2,))}
    degrees = [(30, 1), (31, 2), (32, 63), (33, 64), (34, 65)]
    n_wires, cons, w = setuptest.system(seed=21, n_in=40, n_public=n_public, n_cons=5200, heavy=heavy, degrees=degrees)
    key = setuptest.toy_key(n_wires, n_public, cons, seed=8)
    r1cs = zr.write_r1cs(n_wires, cons, n_pub_out=2, n_pub_in=2, n_prv_in=36)
    s = setuptest.toy_slice_scalars(key)
    slices = {"power": key.power, "tau_g1": prover.fixed_base(0, 1, s["tau"]), "tau_g2": prover.fixed_base(0, 2, s["tau"]),
              "alpha_tau_g1": prover.fixed_base(0, 1, s["alpha_tau"]), "beta_tau_g1": prover.fixed_base(0, 1, s["beta_tau"]),
              "tau_g1_next": prover.fixed_base(0, 1, s["next"]),
              "alpha1": _gpu_points(1, [key.alpha]), "beta1": _gpu_points(1, [key.beta]), "beta2": _gpu_points(2, [key.beta])}
    z0 = setup.new_zkey(r1cs, slices)
    z1 = phase2.contribute(z0, "first", entropy=ENTROPY, urandom=URANDOM)
    z2 = phase2.beacon(z1, "the beacon", BEACON_HASH, BEACON_EXP)
    k1 = phase2.contribution_scalars(URANDOM(64) + ENTROPY.encode())
    k2 = phase2.contribution_scalars(phase2.beacon_seed(bytes.fromhex(BEACON_HASH), BEACON_EXP))
    return {"n_public": n_public, "n_wires": n_wires, "cons": cons, "w": w, "key": key, "r1cs": r1cs, "slices": slices, "z": (z0, z1, z2), "k": (k1, k2)}


@pytest.mark.gpu
def test_gpu_contribute_then_beacon_equal_the_trapdoor_key_and_prove(chain):
    import torch
    from zkwg import prover, zkey
    key, (z0, z1, z2), ((k1, _), (k2, _)) = chain["key"], chain["z"], chain["k"]
    n_public, w = chain["n_public"], chain["w"]
    got0, d0 = setuptest.zkey_sections(z0)
    keys = []
    for z, delta in ((z1, k1), (z2, k1 * k2 % R)):
        got, d = setuptest.zkey_sections(z)
        want, kd = _expected(key, delta)
        for name in (8, 9, "delta1", "delta2", 3, 5, 6, 7, "alpha1", "beta1", "beta2", "gamma2"):
            assert got[name] == want[name], name
        for name in (3, 5, 6, 7, "alpha1", "beta1", "beta2", "gamma2"):
            assert got[name] == got0[name], name                               # sections 3 - 7 and alpha, beta, gamma: as they were
        assert d["coeffs"] == d0["coeffs"] and (d["n_vars"], d["n_public"], d["domain_size"]) == (d0["n_vars"], d0["n_public"], d0["domain_size"])
        assert got[8] != got0[8] and got[9] != got0[9] and got["delta1"] != got0["delta1"]
        assert zkey.verification_key(z) == G.vkey_json(kd)
        keys.append(kd)
    vk0, vk1, vk2 = zkey.verification_key(z0), zkey.verification_key(z1), zkey.verification_key(z2)
    assert vk0 != vk1 != vk2 and vk0["vk_delta_2"] == G.g2_json(G2.G2)
    # a proof under the contributed key: accepted with the NEW verification key only
    rng = random.Random(5)
    for z, vk, kd in ((z1, vk1, keys[0]), (z2, vk2, keys[1])):
        wp = prover.WitnessProver(z, device=0, slots=2)
        bl = [(rng.randrange(R), rng.randrange(R))]
        st, proofs = wp.prove(zkeytest.wit_bytes(w), bl)
        assert st == [0]
        pub = wp.public_signals(zkeytest.wit_bytes(w))
        assert pub == [str(w[i]) for i in range(1, n_public + 1)]
        pj = prover.Prover.proof_json(proofs[0])
        assert P.groth16_verify(vk, pub, pj)
        assert not P.groth16_verify(vk0, pub, pj)
        bad = list(pub)
        bad[1] = str((int(bad[1]) + 1) % R)
        assert not P.groth16_verify(vk, bad, pj)
        sc = G.prove_scalars(kd, chain["cons"], w, *bl[0])
        assert proofs[0]["pi_a"] == G1.mul(sc["pi_a"], G1.G) and proofs[0]["pi_c"] == G1.mul(sc["pi_c"], G1.G)
        del wp
    assert not P.groth16_verify(vk1, pub, pj)                                   # (the beacon's proof under the key before the beacon)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_contribution_records_check_out_under_the_oracle_pairing(chain):
    from zkwg import phase2, prover, zkey
    (z0, z1, z2), ((k1, s1), (k2, s2)) = chain["z"], chain["k"]
    pt = prover.point_from_montgomery
    assert phase2.read_contributions(z0) == (bytes(64), [])
    h1, recs1 = phase2.read_contributions(z1)
    h2, recs2 = phase2.read_contributions(z2)
    assert h1 == h2 == bytes(64) and len(recs1) == 1 and len(recs2) == 2 and recs2[0] == recs1[0]
    assert (recs2[0]["name"], recs2[0]["type"], recs2[0]["beacon_hash"]) == ("first", None, None)
    assert (recs2[1]["name"], recs2[1]["type"], recs2[1]["num_iterations_exp"], recs2[1]["beacon_hash"]) == ("the beacon", 1, BEACON_EXP, bytes.fromhex(BEACON_HASH))
    before = zkey.read_zkey(z0, coeffs=False)["delta1"]
    neg = lambda p: (p[0], (-p[1]) % Q)
    for i, (rec, z, k, s) in enumerate(((recs2[0], z1, k1, s1), (recs2[1], z2, k2, s2))):
        after = zkey.read_zkey(z, coeffs=False)["delta1"]
        assert rec["delta_after"] == after
        assert rec["g1_s"] == _gpu_points(1, [s]) and rec["g1_sx"] == _gpu_points(1, [s * k % R])
        import hashlib
        assert rec["transcript"] == hashlib.blake2b(bytes(64) + b"".join(r["raw"] for r in recs2[:i]) + rec["g1_s"] + rec["g1_sx"], digest_size=64).digest()
        sp_raw = phase2.challenge_g2(rec["transcript"])
        assert sp_raw == phase2.challenge_g2(rec["transcript"]) and any(sp_raw)
        sp, spx = pt(sp_raw), pt(rec["g2_spx"])
        # g2_sp is on the twist, of order r, and not a multiple anyone chose: it differs between transcripts
        assert G2.on_curve(sp) and G2.on_curve(spx)
        acc = None
        for bit in bin(R)[2:]:
            acc = G2.add(acc, acc)
            if bit == "1":
                acc = G2.add(acc, sp)
        assert acc is None
        assert spx == G2.mul(k, sp)
        # knowledge of k: e(g1_s, g2_spx) = e(g1_sx, g2_sp), and the same k moved delta1: e(before, g2_spx) = e(after, g2_sp)
        assert P.pairing_product_is_one([(pt(rec["g1_s"]), spx), (neg(pt(rec["g1_sx"])), sp)])
        assert P.pairing_product_is_one([(pt(before), spx), (neg(pt(after)), sp)])
        assert not P.pairing_product_is_one([(pt(before), spx), (neg(pt(rec["g1_s"])), sp)])
        before = after
    assert phase2.challenge_g2(recs2[0]["transcript"]) != phase2.challenge_g2(recs2[1]["transcript"])


@pytest.mark.gpu
def test_gpu_point_scale_device_equals_the_known_logarithms_and_the_host_mirror():
    from zkwg import phase2
    rng = random.Random(31)
    for group, n, pt in ((1, 4099, 64), (2, 2051, 128)):
        logs = [rng.randrange(1, R) for _ in range(n)]
        logs[0] = logs[77] = logs[n - 1] = 0                                    # infinity, the last point included
        logs[1], logs[2] = 1, R - 1
        pts = _gpu_points(group, logs)
        assert pts[:pt] == bytes(pt)
        for s in (rng.randrange(R), R - 1) + ((COFACTOR, (1 << 256) - 1) if group == 2 else ((1 << 255) + 1,)):
            got = phase2.scale_points(group, pts, s)
            assert got == _gpu_points(group, [a * s % R for a in logs]), (group, s)          # every byte
            assert got == phase2test.scale(group, pts, s), (group, s)                      # and the host mirror's
        assert phase2.scale_points(group, pts, 0) == bytes(len(pts))
        assert phase2.scale_points(group, pts, R) == bytes(len(pts))
        assert phase2.scale_points(group, b"", 5) == b""
        bad = bytearray(pts)
        bad[pt * (n - 2) + 5] ^= 1
        with pytest.raises(phase2.Phase2Error, match="curve"):
            phase2.scale_points(group, bytes(bad), 5)
    assert phase2test.violations() == 0


PIECE = 1 << 20                                   # ZK_PHASE2_PIECE (csrc/zkwg_phase2_core.h): the points of one launch series


@pytest.mark.gpu
def test_gpu_point_scale_device_over_two_pieces_equals_its_single_piece_halves():
    """piece + 1 points: the smallest call whose piece loop comes round again (its buffers reused, a last piece of one point)"""
    from zkwg import phase2, ptau
    rng = random.Random(32)
    n = PIECE + 1
    for group, pt in ((1, 64), (2, 128)):
        t, s = rng.randrange(2, R), rng.randrange(1, R)
        pts = ptau.point_powers(group, ptau.generators()[group - 1] * n, 1, t)       # t^i G: distinct points, made on the device
        got = phase2.scale_points(group, pts, s)
        assert got == phase2.scale_points(group, pts[:pt * PIECE], s) + phase2.scale_points(group, pts[pt * PIECE:], s), group
        pick = lambda b: b"".join(b[pt * i:pt * i + pt] for i in (0, PIECE - 1, PIECE))
        assert pick(got) == phase2test.scale(group, pick(pts), s), group
        del pts, got
    assert phase2test.violations() == 0


@pytest.mark.gpu
def test_gpu_refusals_and_the_command_line(chain, tmp_path):
    from zkwg import phase2, prove, ptau, setup, wtns, zkey
    z0, z1, _ = chain["z"]
    sec = zkey.sections(z0)
    s10 = bytes(68)
    for sid in (8, 9):
        for at in (sec[sid][0] + 9, sec[sid][0] + sec[sid][1] - 40):            # the first and the last point of the section
            b = bytearray(z0)
            b[at] ^= 4
            with pytest.raises(phase2.Phase2Error, match="curve"):
                phase2.contribute(bytes(b), "first", entropy=ENTROPY, urandom=URANDOM)
    b = bytearray(z0)
    b[sec[2][0] + 84 + 448 + 3] ^= 1                                            # delta2
    with pytest.raises(phase2.Phase2Error, match="curve"):
        phase2.apply_delta(bytes(b), 7, s10)
    for k in (0, R):
        with pytest.raises(phase2.Phase2Error, match="0 modulo"):
            phase2.apply_delta(z0, k, s10)
    with pytest.raises(phase2.Phase2Error, match="truncated"):
        phase2.apply_delta(z0[:-7], 7, s10)
    with pytest.raises(ValueError):
        phase2.contribute(z0[:-7], "first", entropy=ENTROPY, urandom=URANDOM)
    with pytest.raises(phase2.Phase2Error):
        phase2.beacon(z0, "b", BEACON_HASH, 5)
    assert phase2.contribute(z0, "first", entropy=ENTROPY, urandom=URANDOM) == z1       # and nothing of that is remembered
    st = phase2.last_stats()
    n8, n9 = sec[8][1] // 64, sec[9][1] // 64
    assert st["ops"]["c"]["dbl"] in (252 * n8, 253 * n8, 254 * n8) and st["ops"]["h"]["dbl"] * n8 == st["ops"]["c"]["dbl"] * n9
    assert 60 * n8 < st["ops"]["c"]["add"] < 110 * n8 and all(v >= 0 for v in st["seconds"].values())
    # setup -> phase2 contribute -> prove from the command line; the proof verifies under the contributed key's exported verification key
    sl = {k: (bytes(v.cpu().numpy()) if hasattr(v, "cpu") else v) for k, v in chain["slices"].items()}
    n = chain["key"].n
    lag = lambda name, point, extra=b"": bytes(point * (n - 1)) + sl[name] + extra
    secs = {2: bytes(64 * (2 * n - 1)), 3: bytes(128 * n), 4: sl["alpha1"] + bytes(64 * (n - 1)), 5: sl["beta1"] + bytes(64 * (n - 1)), 6: sl["beta2"],
            12: lag("tau_g1", 64, sl["tau_g1_next"]), 13: lag("tau_g2", 128), 14: lag("alpha_tau_g1", 64), 15: lag("beta_tau_g1", 64)}
    f = lambda name: str(tmp_path / name)
    open(f("c.r1cs"), "wb").write(chain["r1cs"])
    open(f("pot.ptau"), "wb").write(ptau.write_ptau(chain["key"].power, secs))
    open(f("w.wtns"), "wb").write(wtns.write_wtns(zkeytest.wit_bytes(chain["w"])))
    assert setup.main([f("c.r1cs"), f("pot.ptau"), f("c_0000.zkey"), f("vk0.json")]) == 0
    assert open(f("c_0000.zkey"), "rb").read() == z0
    assert phase2.main(["contribute", f("c_0000.zkey"), f("c_0001.zkey"), "--name", "cli", "--entropy", "some text"]) == 0
    assert phase2.main(["beacon", f("c_0001.zkey"), f("c_final.zkey"), BEACON_HASH, "10", "--name", "final"]) == 0
    assert phase2.main(["contribute", f("w.wtns"), f("x.zkey"), "--name", "cli"]) == 1
    zf = open(f("c_final.zkey"), "rb").read()
    assert [r["name"] for r in phase2.read_contributions(zf)[1]] == ["cli", "final"]
    assert prove.main([f("c_final.zkey"), f("w.wtns"), f("proof.json"), f("public.json")]) == 0
    proof, public = json.load(open(f("proof.json"))), json.load(open(f("public.json")))
    assert P.groth16_verify(zkey.verification_key(zf), public, proof)
    assert not P.groth16_verify(json.load(open(f("vk0.json"))), public, proof)
