"""`groth16.prove(zkey, wtns)` on the device for a key of ANY circuit (zkwg.prover.WitnessProver -> zkwg_prover_create_wtns /
zkwg_prover_prove_witnesses -> zk_zkey_abc, csrc/zkwg_kernels_zkey.hip): a seeded random system that is not an email circuit, judged by
the discrete logarithms of a toy key (oracle/pyref/groth16.py) and by the PINNED verifier (oracle/pyref/bn254_pairing.py), and
EmailVerifier(576,192) against the handle path, byte for byte.  Reference call site: packages/helpers/src/chunked-zkey.ts:80-84.
All comparisons are exact.

GPU time of this file (pytest --durations=0 on an MI355X): 21 s in all -- 11.6 s for the one G.setup of (576,192), 3.6 + 3.3 + 2.2 s for
the three tests."""
import ctypes as C
import random

import pytest

import zkeytest
from oracle.pyref import bn254_g1 as G1
from oracle.pyref import bn254_g2 as G2
from oracle.pyref import bn254_pairing as P
from oracle.pyref import groth16 as G

R = G.R
Q = G1.Q


def _mont1(p):
    return bytes(64) if p is None else ((p[0] << 256) % Q).to_bytes(32, "little") + ((p[1] << 256) % Q).to_bytes(32, "little")


def _mont2(p):
    return bytes(128) if p is None else b"".join(((v << 256) % Q).to_bytes(32, "little") for v in (p[0][0], p[0][1], p[1][0], p[1][1]))


def _toy_zkey(n_wires, n_public, cons, key, coeffs):
    """the key `key` (known trapdoor) as a .zkey: bases through prover.fixed_base, section 4 = coeffs"""
    from zkwg import prover, zkey
    pk = prover.ProvingKey.from_scalars(0, n_public, key.power, key.a_tau, key.b_tau, key.c_key[n_public + 1:], key.h_key, key.alpha, key.beta, key.delta)
    down = lambda t: bytes(t.cpu().numpy())
    pts = {"alpha1": pk.alpha1, "beta1": pk.beta1, "beta2": pk.beta2, "gamma2": _mont2(G2.mul(key.gamma, G2.G2)), "delta1": pk.delta1, "delta2": pk.delta2}
    ic = b"".join(_mont1(G1.mul(x, G1.G)) for x in key.ic)
    return pk, zkey.write_zkey(n_wires, n_public, key.n, pts, ic, down(pk.d_a), down(pk.d_b1), down(pk.d_b2), down(pk.d_c), down(pk.d_h), coeffs)


def _resolve(cons, w, n_in):
    """the satisfying witness of zkeytest.random_system's constraints for the input wires w[:n_in]"""
    w = list(w[:n_in])
    for ra, rb, _ in cons:
        w.append(sum(v * w[i] for i, v in ra.items()) % R * (sum(v * w[i] for i, v in rb.items()) % R) % R)
    return w


@pytest.mark.gpu
def test_gpu_witnesses_of_a_random_system_prove_under_the_pinned_verifier():
    import torch
    import zkwg
    from zkwg import prover
    dev = torch.device("cuda", 0)
    n_public = 5
    n_wires, cons, w = zkeytest.random_system(seed=7, n_public=n_public)
    n_in = n_wires - len(cons)
    rng = random.Random(12)
    w_b = _resolve(cons, [1] + [rng.choice([0, 1, rng.randrange(R)]) for _ in range(n_in - 1)], n_in)      # a second satisfying witness
    w_bad = list(w)
    w_bad[n_in + 3] = (w_bad[n_in + 3] + 1) % R                      # constraint 3 fails
    w_big = list(w)
    w_big[n_in // 2] += R                                             # the same value mod r, not reduced (w[n_in // 2] + r < 2^256)
    assert w_big[n_in // 2] < 1 << 256
    key = G.setup(n_wires, n_public, cons, seed=41)
    n_rows = len(cons) + n_public + 1
    pk, z = _toy_zkey(n_wires, n_public, cons, key, zkeytest.section4(cons, n_public))
    wp = prover.WitnessProver(z, device=0, slots=4)
    E = wp.lib.zkwg_prover_emails_per_series(wp._h)
    assert (wp.n_vars, wp.n_public, wp.n_rows) == (n_wires, n_public, n_rows) and wp.lib.zkwg_prover_contexts(wp._h) == 2 and E == 2
    # more witnesses than the contexts hold at once (they roll), repeated ones, a failing constraint, a value that is not reduced
    ws = [w, w_b, w, w_bad, w_big, w_b, w]
    bl = [(rng.randrange(R), rng.randrange(R)) for _ in ws]
    raw = b"".join(zkeytest.wit_bytes(x) for x in ws)
    st, proofs = wp.prove(raw, bl)
    assert st == [0, 0, 0, 0, prover.STATUS_WITNESS_NOT_REDUCED, 0, 0] and proofs[4] is None
    st_b, raw_proofs = wp.prove_bytes(raw, bl)
    assert raw_proofs[256 * 4:256 * 5] == bytes(256)
    # zk_zkey_abc alone, every value against the oracle's buildABC1 (the flagged witness too: its terms are reduced mod r, never dropped)
    d_w = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    abc = bytes(wp.abc_device(d_w, len(ws)).cpu().numpy())
    for e, x in enumerate(ws):
        a, b, c = zkeytest.abc_ints(abc[96 * n_rows * e:96 * n_rows * (e + 1)], n_rows)
        A, B, Cc = G.abc_rows(key, cons, x)
        assert a == A[:n_rows] and b == B[:n_rows] and c == Cc[:n_rows], e
    # the five sums of two witnesses, stage by stage over the same buffers, against their discrete logarithms
    ntt = zkwg.Ntt(key.power, device=0)
    d_h = torch.empty(32 << key.power, dtype=torch.uint8, device=dev)
    d_nw = torch.empty(ntt.work_bytes(1), dtype=torch.uint8, device=dev)
    plans = {"a": prover._DeviceMsm(pk.d_a, 1, 0), "b1": prover._DeviceMsm(pk.d_b1, 1, 0), "b2": prover._DeviceMsm(pk.d_b2, 2, 0),
             "c": prover._DeviceMsm(pk.d_c, 1, 0), "h": prover._DeviceMsm(pk.d_h, 1, 0)}
    d_mw = torch.empty(max(m.work_bytes() for m in plans.values()) + 256, dtype=torch.uint8, device=dev)
    d_mw = d_mw[(-d_mw.data_ptr()) % 256:]
    d_abc = wp.abc_device(d_w, len(ws))
    for e in (0, 3):
        sc = G.prove_scalars(key, cons, ws[e], *bl[e])
        ntt.h_evaluations_device(d_abc[96 * n_rows * e:], 96 * n_rows, n_rows, 1, d_nw, d_h)
        wit = d_w.data_ptr() + 32 * n_wires * e
        got = {"a": plans["a"].run(wit, False, True, d_mw), "b1": plans["b1"].run(wit, False, True, d_mw), "b2": plans["b2"].run(wit, False, True, d_mw),
               "c": plans["c"].run(wit + 32 * (n_public + 1), False, True, d_mw), "h": plans["h"].run(d_h.data_ptr(), True, False, d_mw)}
        for name, k_ in (("a", "a"), ("b1", "b"), ("c", "c"), ("h", "h")):
            assert prover.point_from_montgomery(got[name]) == G1.mul(sc[k_], G1.G), (e, name)
        assert prover.point_from_montgomery(got["b2"]) == G2.mul(sc["b"], G2.G2), e
    # every proof: the group elements of its discrete logarithms, and the verifier's verdict
    vk = G.vkey_json(key)
    for e, x in enumerate(ws):
        if e == 4:
            continue
        sc = G.prove_scalars(key, cons, x, *bl[e])
        p = proofs[e]
        assert p["pi_a"] == G1.mul(sc["pi_a"], G1.G) and p["pi_c"] == G1.mul(sc["pi_c"], G1.G) and p["pi_b"] == G2.mul(sc["pi_b"], G2.G2), e
        if e in (0, 1, 3):
            pub = wp.public_signals(zkeytest.wit_bytes(x))
            assert pub == [str(x[i]) for i in range(1, n_public + 1)]
            ok = P.groth16_verify(vk, pub, prover.Prover.proof_json(p))
            assert ok == (e != 3), e                                 # a proof of the witness that fails a constraint is returned and REJECTED
            if e == 0:
                bad = list(pub)
                bad[2] = str((int(bad[2]) + 1) % R)
                assert not P.groth16_verify(vk, bad, prover.Prover.proof_json(p))
    # device-resident witnesses and `.wtns` blobs give the same bytes; the others are unchanged by the flagged one
    from zkwg import wtns
    assert wp.prove_bytes(d_w, bl) == (st_b, raw_proofs)
    assert wp.prove_bytes([wtns.write_wtns(zkeytest.wit_bytes(x)) for x in ws], bl) == (st_b, raw_proofs)
    keep = [0, 1, 2, 3, 5, 6]
    st2, raw2 = wp.prove_bytes(b"".join(zkeytest.wit_bytes(ws[e]) for e in keep), [bl[e] for e in keep])
    assert st2 == [0] * 6 and raw2 == b"".join(raw_proofs[256 * e:256 * e + 256] for e in keep)
    # misuse: the email entry points on this prover, a .wtns of another size, a short stride
    assert wp.lib.zkwg_prover_prove_batch(wp._h, b"x", 1, bytes(64), (C.c_int32 * 1)(), (C.c_uint8 * 256)()) == -2
    with pytest.raises(ValueError):
        wp.prove([wtns.write_wtns(bytes(32 * (n_wires - 1)))], bl[:1])
    assert wp.lib.zkwg_prover_prove_witnesses(wp._h, raw, 32 * n_wires - 32, 1, bytes(64), (C.c_int32 * 1)(), (C.c_uint8 * 256)()) == -2


@pytest.fixture(scope="module")
def ev_576_192():
    """EmailVerifier(576,192): handle, constraints, ONE toy key (G.setup is the expensive part) and its .zkey"""
    import torch
    import zkwg
    from zkwg import r1cs as zr
    N, M, n_public = 576, 192, 20
    c = zkwg.Circuit(zkwg.MAIN_EMAIL_VERIFIER, max_header=N, max_body=M, device=0)
    cons = zr.email_verifier_constraints(c.symbols(), N, M)
    full = zr.append_public_rows(cons, n_public)
    key = G.setup(c.W, n_public, cons, seed=31)
    coeffs = [(m, j, w, v % R) for j, row in enumerate(full) for m in (0, 1) for w, v in row[m].items() if v % R]
    pk, z = _toy_zkey(c.W, n_public, cons, key, coeffs)
    del pk, coeffs
    torch.cuda.empty_cache()
    return c, key, len(full), z


@pytest.mark.gpu
def test_gpu_email_verifier_witnesses_prove_byte_identically_to_the_handle_path(ev_576_192):
    import torch
    import zkwg
    from zkwg import prover, synth
    c, key, n_rows, z = ev_576_192
    n, n_public = 3, 20
    recs, _ = synth.packed_batch(c, seed=8, n=n, body_len=100)
    rng = random.Random(4)
    bl = [(rng.randrange(R), rng.randrange(R)) for _ in range(n)]
    pz = prover.Prover.from_zkey(c, z, slots=4)
    st1, want = pz.prove_records(recs, bl, slots=4)
    wit, st0 = c.calculate_batch_host(recs)
    assert st0 == st1 == [0] * n
    wits = [wit[e * c.witness_bytes:e * c.witness_bytes + 32 * c.W] for e in range(n)]
    wp = prover.WitnessProver(z, device=0, slots=4)
    assert wp.n_rows == n_rows and wp.n_vars == c.W
    st2, got = wp.prove(wits, bl)
    assert st2 == [0] * n and got == want
    # the witness entry points on a handle prover are misuse
    assert wp.lib.zkwg_prover_prove_witnesses(pz._h, wits[0], 32 * c.W, 1, bytes(64), (C.c_int32 * 1)(), (C.c_uint8 * 256)()) == -2
    vk = G.vkey_json(key)
    assert P.groth16_verify(vk, wp.public_signals(wits[0]), prover.Prover.proof_json(got[0]))
    # zk_zkey_abc against zkwg_expand_abc_device(montgomery = 1) of the same emails + C.w = A.w o B.w (what zk_abc_c_from_ab forms)
    dev = torch.device("cuda", 0)
    d_in = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to(dev)
    d_status = torch.zeros(n, dtype=torch.int32, device=dev)
    d_scratch = torch.empty(c.scratch_bytes(n), dtype=torch.uint8, device=dev)
    c.prepare_device(d_in, n, d_status, d_scratch)
    torch.cuda.synchronize()
    assert c.abc_bytes == 96 * n_rows
    d_ref = torch.empty(n * c.abc_bytes, dtype=torch.uint8, device=dev)
    c.expand_abc_device(d_in, n, d_scratch, 0, n, d_ref, montgomery=True)
    d_w = torch.frombuffer(bytearray(b"".join(wits)), dtype=torch.uint8).to(dev)
    ours = bytes(wp.abc_device(d_w, n).cpu().numpy())
    torch.cuda.synchronize()
    ref = bytes(d_ref.cpu().numpy())
    rinv = pow(1 << 256, -1, R)
    for e in range(n):
        o, q = ours[96 * n_rows * e:96 * n_rows * (e + 1)], ref[96 * n_rows * e:96 * n_rows * (e + 1)]
        assert o[:64 * n_rows] == q[:64 * n_rows], e                 # A.w and B.w, every byte
        a, b, cc = (zkwg.witness_ints(o[32 * n_rows * k:32 * n_rows * (k + 1)]) for k in range(3))
        assert all(x * y * rinv % R == t for x, y, t in zip(a, b, cc)), e


@pytest.mark.gpu
def test_gpu_node_host_proves_a_wtns_file(ev_576_192, tmp_path):
    """js/prove.js --wtns witness.wtns circuit.zkey proof.json public.json (zkwg.js groth16.prove -> the addon -> zkwg_prover_create_wtns /
    zkwg_prover_prove_witnesses) on a .wtns written by zkwg_write_wtns: accepted by the pinned verifier"""
    import json
    import os
    import shutil
    import subprocess
    from conftest import ROOT
    from zkwg import synth
    js = os.path.join(ROOT, "zk-email-verify_amd", "js")
    if shutil.which("node") is None or not os.path.exists(os.path.join(js, "zkwg_addon.node")):
        pytest.skip("node or the built addon is missing")
    c, key, n_rows, z = ev_576_192
    recs, _ = synth.packed_batch(c, seed=9, n=1, body_len=100)
    wit, st = c.calculate_batch_host(recs)
    assert st == [0]
    (tmp_path / "c.zkey").write_bytes(z)
    (tmp_path / "w.wtns").write_bytes(c.wtns(wit))
    r = subprocess.run(["node", os.path.join(js, "prove.js"), "--wtns", str(tmp_path / "w.wtns"), str(tmp_path / "c.zkey"), str(tmp_path / "proof.json"),
                        str(tmp_path / "public.json")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    proof, public = json.load(open(tmp_path / "proof.json")), json.load(open(tmp_path / "public.json"))
    w = [int.from_bytes(wit[32 * i:32 * i + 32], "little") for i in range(21)]
    assert public == [str(x) for x in w[1:21]]
    assert P.groth16_verify(G.vkey_json(key), public, proof)
