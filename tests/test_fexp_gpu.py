"""Per-proof groth16 verification on the device (zkwg.verify.verify_each -> zkwg_groth16_verify_each -> zk_g16_vkx / zk_pair_miller /
zk_fexp_fold / zk_fexp_step / zk_fexp_ninv / zk_fexp_pow_u, csrc/zkwg_kernels_fexp.hip): the final exponentiation of
zkwg_final_exp_device against the host's 2,790-bit square-and-multiply (csrc/zkwg_pairing.h, through tests/native/pairtest.cpp) BYTE FOR
BYTE, and the verdicts against the host path (device = -1), planted truth and verify_batch, on sets in which MOST proofs are bad.  32
values per workgroup, so n = 1, 33 and 131: a single value, one past a workgroup, five workgroups with a ragged last one.  All comparisons
are exact.  Reference call: packages/helpers/src/chunked-zkey.ts:93-101."""
import json
import os
import random
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

import pairtest
import verifytest
from conftest import ROOT
from oracle.pyref import bn254_g2 as G2

pytestmark = pytest.mark.gpu
R, Q = pairtest.R, pairtest.Q
N = 131
GOLDEN = os.path.join(ROOT, "tests", "golden", "proof_of_twitter")
PKG = os.path.join(ROOT, "zk-email-verify_amd", "py")
ZERO = bytes(384)


def _gpu_points(group, scalars):
    from zkwg import prover
    return bytes(prover.fixed_base(0, group, scalars).cpu().numpy())


def _many(fn, args):
    """fn over args on 16 threads (the host pairing's pieces are C calls that release the interpreter)"""
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda a: fn(*a), args))


@pytest.fixture(scope="module")
def values():
    """131 values: the device's Miller values of the fixture pairs of tests/test_pair_gpu.py (the same seeds: exact 1s from infinity at 0,
    70 and 130, the meaningless but non-zero values of G2 points outside the subgroup at 5, 64 and 129), with the seven members of the
    edge family at 10 .. 16 and an all-zero value at 20 -> ([384 bytes], the host's final exponentiation of each)"""
    import torch
    from zkwg import _call, _lib
    rng = random.Random(1320)
    l1, l2 = [rng.randrange(1, R) for _ in range(N)], [rng.randrange(1, R) for _ in range(N)]
    l1[0] = l2[70] = l1[130] = l2[130] = 0
    l1[1] = l2[1] = 1
    l1[2] = l2[2] = R - 1
    g1, g2 = _gpu_points(1, l1), bytearray(_gpu_points(2, l2))
    t = verifytest.twist_points(1, 1321)[0]
    small = verifytest.small_order_points(t)[0]
    for i, p in {5: t, 64: small, 129: G2.add(G2.mul(l2[129], G2.G2), small)}.items():
        g2[128 * i:128 * i + 128] = pairtest.mont2(p)
    d1, d2 = _call.upload(g1, 0), _call.upload(bytes(g2), 0)
    f = torch.zeros(384 * N, dtype=torch.uint8, device=d1.device)
    inside = torch.zeros(N, dtype=torch.uint8, device=d1.device)
    assert _lib.load().zkwg_miller_device(0, d1.data_ptr(), d2.data_ptr(), N, f.data_ptr(), inside.data_ptr(), None) == 0
    raw = _call.download(f)
    vals = [raw[384 * i:384 * i + 384] for i in range(N)]
    assert [int(v) for v in _call.download(inside)] == [0 if i in (5, 64, 129) else 1 for i in range(N)]
    assert all(vals[i] == pairtest.ONE for i in (0, 70, 130)) and all(vals[i] not in (ZERO, pairtest.ONE) for i in (5, 64, 129))
    for j, (_, v) in enumerate(pairtest.f12_edge_family(1420)):
        vals[10 + j] = v
    vals[20] = ZERO
    return vals, _many(pairtest.final_exp, [(v,) for v in vals])


@pytest.mark.parametrize("n", [1, 33, 131])
def test_the_final_exponentiation_equals_the_hosts_byte_for_byte(values, n):
    import torch
    from zkwg import _call, _lib
    vals, want = values
    d_f = _call.upload(b"".join(vals[:n]), 0)
    out = torch.full((384 * N,), 0xAB, dtype=torch.uint8, device=d_f.device)
    assert _lib.load().zkwg_final_exp_device(0, d_f.data_ptr(), n, out.data_ptr(), None) == 0
    raw = _call.download(out)
    got = [raw[384 * i:384 * i + 384] for i in range(n)]
    bad = [i for i in range(n) if got[i] != want[i]]
    assert not bad, bad
    assert raw[384 * n:] == bytes([0xAB]) * (384 * (N - n))       # nothing beyond n is written
    assert _call.download(d_f) == b"".join(vals[:n])              # the input is as it was
    if n == 33:
        assert want[20] == ZERO and want[0] == pairtest.ONE and want[14] == pairtest.ONE          # 0 -> 0, 1 -> 1, a value of Fq2 (c0 alone) -> 1
        assert _lib.load().zkwg_final_exp_device(0, d_f.data_ptr(), n, d_f.data_ptr(), None) == 0  # in place
        assert _call.download(d_f) == b"".join(want[:n])
        assert _lib.load().zkwg_final_exp_device(0, d_f.data_ptr(), 0, out.data_ptr(), None) == 0
        assert _lib.load().zkwg_final_exp_device(-1, d_f.data_ptr(), n, out.data_ptr(), None) != 0
        assert _lib.load().zkwg_final_exp_device(0, d_f.data_ptr() + 8, 1, out.data_ptr(), None) == -2      # alignment: ZKWG_RC_BAD_ARG


# ---- verdicts ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy():
    """131 fabricated proofs of a toy key with 3 public inputs, some of them 0: (vkey, publics, the points in the zkey's form)"""
    rng = random.Random(1421)
    key = pairtest.toy_key(3, 1421)
    publics = [[rng.randrange(R) for _ in range(3)] for _ in range(N)]
    publics[3], publics[4], publics[32] = [0, publics[3][1], 0], [0, 0, 0], [R - 1, 0, 1]
    logs = [pairtest.fabricate(key, x, rng.randrange(1, R), rng.randrange(1, R)) for x in publics]
    a, b, c = _gpu_points(1, [l[0] for l in logs]), _gpu_points(2, [l[1] for l in logs]), _gpu_points(1, [l[2] for l in logs])
    c_bad = _gpu_points(1, [(l[2] + 1) % R for l in logs])
    return pairtest.G.vkey_json(key), publics, (a, b, c, c_bad)


def _planted(toy, n):
    """n proofs of which MOST are bad: every odd index and every index from n - n // 8 on has a wrong pi_c, and the six rejection kinds sit at
    even indices 6 .. 16 -> (publics, proofs, the planted verdicts, how many reach the device)"""
    vkey, publics, (a, b, c, c_bad) = toy
    pt = lambda s, i, w: s[w * i:w * i + w]
    wrong_c = {i for i in range(n) if i % 2 == 1 or i >= n - n // 8}
    proofs = [pairtest.proof_bytes_from_mont(pt(a, i, 64), pt(b, i, 128), pt(c_bad if i in wrong_c else c, i, 64)) for i in range(n)]
    publics = [list(p) for p in publics[:n]]
    want = [i not in wrong_c for i in range(n)]
    excluded = 0
    if n > 16:
        small = verifytest.small_order_points(verifytest.twist_points(1, 1422)[0])[0]
        word = lambda v: int(v).to_bytes(32, "little")
        ax, ay = (int.from_bytes(proofs[8][o:o + 32], "little") for o in (0, 32))
        publics[6][1] += R                                                                                   # a public input >= r
        proofs[8] = word(ax + Q) + proofs[8][32:]                                                            # a coordinate >= q
        proofs[10] = proofs[10][:32] + word((int.from_bytes(proofs[10][32:64], "little") + 1) % Q) + proofs[10][64:]      # A off its curve
        b12 = verifytest.decode_g2(pt(b, 12, 128))
        proofs[12] = pairtest.proof_bytes_from_mont(pt(a, 12, 64), pairtest.mont2(G2.add(b12, small)), pt(c, 12, 64))     # B outside the subgroup, ON its curve
        proofs[14] = bytes(256)                                                                              # all zero
        proofs[16] = proofs[16][:192] + bytes(64)                                                            # C at infinity
        for i in (6, 8, 10, 12, 14, 16):
            want[i] = False
        excluded = 5                                                                                         # (12 reaches the device)
    assert sum(1 for w in want if not w) > n // 2 or n == 1
    return publics, proofs, want, n - excluded


@pytest.mark.parametrize("n", [1, 33, 131])
def test_verdicts_equal_the_host_path_and_the_planted_truth_with_most_proofs_bad(toy, n):
    from zkwg import verify
    vkey = toy[0]
    publics, proofs, want, reached = _planted(toy, n)
    got = verify.verify_each(vkey, publics, proofs, device=0)
    sec, cnt = verify.stats_each()
    print("seconds", sec, "counts", cnt)
    assert got == want
    # three pairs through the Miller kernel and one value through the final exponentiation per proof that reached the device (+ e(alpha,
    # beta)): the work does not depend on how many of them are bad
    assert cnt == [3 * reached, reached + 1, n - reached, sum(1 for w in want if not w) - (n - reached)]
    assert verify.verify_each(vkey, publics, proofs, device=-1) == want
    assert verify.stats_each()[1] == cnt
    if n <= 33:
        assert verify.verify_batch(vkey, publics, proofs, device=0) == want
    # every proof good: the same work
    good = [pairtest.proof_bytes_from_mont(toy[2][0][64 * i:64 * i + 64], toy[2][1][128 * i:128 * i + 128], toy[2][2][64 * i:64 * i + 64]) for i in range(n)]
    assert verify.verify_each(vkey, toy[1][:n], good, device=0) == [True] * n
    assert verify.stats_each()[1] == [3 * n, n + 1, 0, 0]


def test_the_golden_proof_alone_and_among_tampered_ones():
    from zkwg import verify
    vkey, public, proof = (json.load(open(os.path.join(GOLDEN, f))) for f in ("vkey.json", "public.json", "proof.json"))
    bad_public = [str((int(public[0]) + 1) % R)] + public[1:]
    assert verify.verify_each(vkey, [public], [proof], device=0) == [True]
    assert verify.verify_each(vkey, [bad_public, public, bad_public], [proof] * 3, device=0) == [False, True, False]
    assert verify.verify_each(vkey, [], [], device=0) == []


def test_a_proof_of_the_device_prover_verifies_and_fails_with_a_changed_public_input():
    import test_prove_wtns as tpw
    import zkeytest
    from zkwg import prover, verify
    n_public = 5
    n_wires, cons, w = zkeytest.random_system(seed=7, n_public=n_public)
    key = pairtest.G.setup(n_wires, n_public, cons, seed=41)
    _, z = tpw._toy_zkey(n_wires, n_public, cons, key, zkeytest.section4(cons, n_public))
    wp = prover.WitnessProver(z, device=0, slots=4)
    raw = zkeytest.wit_bytes(w)
    st, proofs = wp.prove_bytes(raw, [(12345, 67890)])
    assert st == [0]
    vkey, pub = pairtest.G.vkey_json(key), wp.public_signals(raw)
    flipped = [str((int(pub[0]) + 1) % R)] + pub[1:]
    assert verify.verify_each(vkey, [pub, flipped], [proofs[:256]] * 2, device=0) == [True, False]


def test_the_command_line_with_each_on_the_device(tmp_path):
    public = json.load(open(os.path.join(GOLDEN, "public.json")))
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = lambda pub: subprocess.run([sys.executable, "-m", "zkwg.verify", os.path.join(GOLDEN, "vkey.json"), pub, os.path.join(GOLDEN, "proof.json"), "--device", "0", "--each"],
                                     env=env, capture_output=True, text=True)
    r = run(os.path.join(GOLDEN, "public.json"))
    assert (r.returncode, r.stdout.split()) == (0, ["OK"]), r.stderr
    bad = tmp_path / "public.json"
    bad.write_text(json.dumps([str((int(public[0]) + 1) % R)] + public[1:]))
    r = run(str(bad))
    assert (r.returncode, r.stdout.split()) == (1, ["INVALID"]), r.stderr
