"""`groth16 setup` on the device (zkwg.setup.new_zkey -> zkwg_zkey_new -> csrc/zkwg_kernels_setup.hip): from the toy powers of a known
(tau, alpha, beta) the new key equals, in EVERY byte of sections 3, 5 - 9 and of the header points, the key oracle/pyref/groth16.py makes
from the same trapdoor with gamma = delta = 1 (bases through prover.fixed_base, as tests/test_prove_wtns.py makes its keys); proofs
under the new key are accepted by the PINNED verifier (oracle/pyref/bn254_pairing.py) with zkey.verification_key(new key).  A seeded
system whose long wires need several wavefronts each, and EmailVerifier(576,192).  Reference workflow:
docs/zk-email-docs/UsageGuide/README.md:145-180.  All comparisons are exact.

GPU time of this file: NOT MEASURED YET -- no MI355X run of it is on record (budget: 120 s; the fixture's G.setup of (576,192) was 11.6 s
and its two Lagrange vectors are estimated at 17 s in tests/test_prove_wtns.py's terms)."""
import random

import pytest

import setuptest
import zkeytest
from oracle.pyref import bn254_pairing as P
from oracle.pyref import groth16 as G

R = G.R


def _gpu_points(group, scalars):
    from zkwg import prover
    return bytes(prover.fixed_base(0, group, scalars).cpu().numpy())


def _assert_key(z, key, n_wires, n_public, sections=(3, 5, 6, 7, 8, 9)):
    got, d = setuptest.zkey_sections(z)
    want = setuptest.toy_sections(key, _gpu_points)
    assert (d["n_vars"], d["n_public"], d["domain_size"]) == (n_wires, n_public, key.n)
    for name in tuple(sections) + ("alpha1", "beta1", "beta2", "gamma2", "delta1", "delta2"):
        assert got[name] == want[name], name
    return d


@pytest.mark.gpu
def test_gpu_new_zkey_of_a_system_with_long_wires_equals_the_trapdoor_key():
    import torch
    from zkwg import prover, ptau, r1cs as zr, setup, zkey
    n_public = 4
    heavy = {0: (4500, (0, 1, 2)), 3: (4300, (0,)), 4: (4200, (1,)), 5: (4100, (2,))}
    degrees = [(30, 1), (31, 2), (32, 63), (33, 64), (34, 65)]
    n_wires, cons, w = setuptest.system(seed=21, n_in=40, n_public=n_public, n_cons=5200, heavy=heavy, degrees=degrees)
    assert len(cons) >= 5000 and setuptest.satisfied(cons, w)
    assert sum(1 for wr in (0, 3, 4, 5) if setuptest.wire_degree(cons, wr) > 4096) >= 3 and setuptest.wire_degree(cons, 0) > 4096
    assert [setuptest.wire_degree(cons, wr) for wr, _ in degrees] == [1, 2, 63, 64, 65]
    assert sum(1 for a, _, _ in cons if 3 in a) > 4096 and sum(1 for _, b, _ in cons if 4 in b) > 4096        # several wavefronts per wire in A and in B
    classes = lambda v: "one" if v == 1 else "minus" if v == R - 1 else "small" if v < 1000 else "pow2" if v & (v - 1) == 0 else \
        "negpow2" if (R - v) & (R - v - 1) == 0 else "uniform"
    for m in range(3):
        assert {classes(v) for row in cons for v in row[m].values()} == {"one", "minus", "small", "pow2", "negpow2", "uniform"}, m
    key = setuptest.toy_key(n_wires, n_public, cons, seed=8)
    assert key.power == 13
    r1cs = zr.write_r1cs(n_wires, cons, n_pub_out=2, n_pub_in=2, n_prv_in=36)
    assert setup.key_shape(r1cs)[0] == 13
    # the toy ceremony, resident on the device
    s = setuptest.toy_slice_scalars(key)
    dev_slices = {"power": key.power, "tau_g1": prover.fixed_base(0, 1, s["tau"]), "tau_g2": prover.fixed_base(0, 2, s["tau"]),
                  "alpha_tau_g1": prover.fixed_base(0, 1, s["alpha_tau"]), "beta_tau_g1": prover.fixed_base(0, 1, s["beta_tau"]),
                  "tau_g1_next": prover.fixed_base(0, 1, s["next"]),
                  "alpha1": _gpu_points(1, [key.alpha]), "beta1": _gpu_points(1, [key.beta]), "beta2": _gpu_points(2, [key.beta])}
    z = setup.new_zkey(r1cs, dev_slices)
    d = _assert_key(z, key, n_wires, n_public)
    assert sorted(d["coeffs"]) == sorted(zkeytest.section4(cons, n_public))
    host_slices = {k: (bytes(v.cpu().numpy()) if hasattr(v, "cpu") else v) for k, v in dev_slices.items()}
    # host buffers instead of device tensors: the same bytes
    assert setup.new_zkey(r1cs, host_slices) == z
    # the same slices through a .ptau file + zkwg_ptau_parse: the same bytes.  The file is of power 13; the levels below 13 and the
    # monomial sections, which the set-up never reads, are zeros
    n = key.n
    lag = lambda name, point, extra=b"": bytes(point * (n - 1)) + host_slices[name] + extra
    secs = {2: bytes(64 * (2 * n - 1)), 3: bytes(128 * n), 4: host_slices["alpha1"] + bytes(64 * (n - 1)), 5: host_slices["beta1"] + bytes(64 * (n - 1)),
            6: host_slices["beta2"], 12: lag("tau_g1", 64, host_slices["tau_g1_next"]), 13: lag("tau_g2", 128), 14: lag("alpha_tau_g1", 64),
            15: lag("beta_tau_g1", 64)}
    blob = ptau.write_ptau(key.power, secs)
    assert setup.new_zkey(r1cs, blob) == z
    assert setup.new_zkey(r1cs, memoryview(blob)) == z
    # a proof under the new key
    wp = prover.WitnessProver(z, device=0, slots=2)
    assert (wp.n_vars, wp.n_public, wp.n_rows) == (n_wires, n_public, len(cons) + n_public + 1)
    rng = random.Random(5)
    bl = [(rng.randrange(R), rng.randrange(R))]
    st, proofs = wp.prove(zkeytest.wit_bytes(w), bl)
    assert st == [0]
    vk = zkey.verification_key(z)
    assert vk == G.vkey_json(key)
    pub = wp.public_signals(zkeytest.wit_bytes(w))
    assert pub == [str(w[i]) for i in range(1, n_public + 1)]
    assert P.groth16_verify(vk, pub, prover.Prover.proof_json(proofs[0]))
    sc = G.prove_scalars(key, cons, w, *bl[0])
    from oracle.pyref import bn254_g1 as G1
    assert proofs[0]["pi_a"] == G1.mul(sc["pi_a"], G1.G) and proofs[0]["pi_c"] == G1.mul(sc["pi_c"], G1.G)
    bad = list(pub)
    bad[1] = str((int(bad[1]) + 1) % R)
    assert not P.groth16_verify(vk, bad, prover.Prover.proof_json(proofs[0]))
    # refusals: one corrupted point in a slice (each slice in turn; host and device), slices of another power, nPublic + 1 >= nVars
    for name in ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "tau_g1_next"):
        b = bytearray(host_slices[name])
        b[len(b) - 40] ^= 4
        with pytest.raises(setup.SetupError, match="curve"):
            setup.new_zkey(r1cs, dict(host_slices, **{name: bytes(b)}))
    t = dev_slices["tau_g1"].clone()
    t[64 * 777 + 3] ^= 1
    with pytest.raises(setup.SetupError, match="curve"):
        setup.new_zkey(r1cs, dict(dev_slices, tau_g1=t))
    with pytest.raises(setup.SetupError, match="too small"):
        setup.new_zkey(r1cs, ptau.write_ptau(3, {sid: bytes(point * count(8)) for sid, point, count in ptau.SECTIONS}))
    with pytest.raises(setup.SetupError, match="not prepared"):
        setup.new_zkey(r1cs, ptau.write_ptau(key.power, {k: v for k, v in secs.items() if k < 12}))
    with pytest.raises(setup.SetupError, match="nPublic"):
        setup.new_zkey(zr.write_r1cs(n_wires, cons, n_pub_out=n_wires - 1), dev_slices)
    with pytest.raises(setup.SetupError):
        setup.new_zkey(r1cs[:-7], dev_slices)
    assert setup.new_zkey(r1cs, dev_slices) == z                 # and nothing of that is remembered
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def ev_576_192():
    """EmailVerifier(576,192): handle, constraints, ONE trapdoor key with gamma = delta = 1 (G.setup is the expensive part) and the
    Lagrange scalars of its two domains"""
    import zkwg
    from zkwg import r1cs as zr
    N, M, n_public = 576, 192, 20
    c = zkwg.Circuit(zkwg.MAIN_EMAIL_VERIFIER, max_header=N, max_body=M, device=0)
    cons = zr.email_verifier_constraints(c.symbols(), N, M)
    key = setuptest.toy_key(c.W, n_public, cons, seed=31)
    return c, cons, key, setuptest.toy_slice_scalars(key)


@pytest.mark.gpu
def test_gpu_new_zkey_of_email_verifier_equals_the_trapdoor_key_and_proves_the_same(ev_576_192):
    import torch
    from zkwg import prover, r1cs as zr, setup, synth, zkey
    c, cons, key, s = ev_576_192
    n_public = 20
    r1cs = zr.write_r1cs(c.W, cons, n_pub_out=3, n_pub_in=17)
    assert setup.key_shape(r1cs)[0] == key.power
    dev_slices = {"power": key.power, "tau_g1": prover.fixed_base(0, 1, s["tau"]), "tau_g2": prover.fixed_base(0, 2, s["tau"]),
                  "alpha_tau_g1": prover.fixed_base(0, 1, s["alpha_tau"]), "beta_tau_g1": prover.fixed_base(0, 1, s["beta_tau"]),
                  "tau_g1_next": prover.fixed_base(0, 1, s["next"]),
                  "alpha1": _gpu_points(1, [key.alpha]), "beta1": _gpu_points(1, [key.beta]), "beta2": _gpu_points(2, [key.beta])}
    z = setup.new_zkey(r1cs, dev_slices)
    del dev_slices
    torch.cuda.empty_cache()
    # the old route: the same key (gamma = delta = 1) written from its discrete logarithms
    full = zr.append_public_rows(cons, n_public)
    coeffs = [(m, j, w, v % R) for j, row in enumerate(full) for m in (0, 1) for w, v in row[m].items() if v % R]
    want = setuptest.toy_sections(key, _gpu_points)
    got, d = setuptest.zkey_sections(z)
    for name in (5, 6, 7, 8, 9, 3, "alpha1", "beta1", "beta2", "gamma2", "delta1", "delta2"):
        assert got[name] == want[name], name
    assert sorted(d["coeffs"]) == sorted(coeffs)
    z_old = zkey.write_zkey(c.W, n_public, key.n, {k: want[k] for k in ("alpha1", "beta1", "beta2", "gamma2", "delta1", "delta2")},
                            want[3], want[5], want[6], want[7], want[8], want[9], coeffs)
    del want, got, d, coeffs
    n = 2
    recs, _ = synth.packed_batch(c, seed=8, n=n, body_len=100)
    rng = random.Random(4)
    bl = [(rng.randrange(R), rng.randrange(R)) for _ in range(n)]
    st_new, p_new = prover.Prover.from_zkey(c, z, slots=2).prove_records(recs, bl, slots=2)
    torch.cuda.empty_cache()
    st_old, p_old = prover.Prover.from_zkey(c, z_old, slots=2).prove_records(recs, bl, slots=2)
    assert st_new == st_old == [0] * n and p_new == p_old
    wit, st0 = c.calculate_batch_host(recs)
    pub = [str(int.from_bytes(wit[32 * i:32 * i + 32], "little")) for i in range(1, n_public + 1)]
    assert P.groth16_verify(zkey.verification_key(z), pub, prover.Prover.proof_json(p_new[0]))
