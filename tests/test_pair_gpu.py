"""Batched groth16 verification on the device (zkwg.verify -> zkwg_groth16_verify_batch -> zk_pair_miller / zk_pair_product,
csrc/zkwg_kernels_pair.hip): the Miller values and subgroup flags of zkwg_miller_device against the host pairing (csrc/zkwg_pairing.h,
through tests/native/pairtest.cpp), the product tree against the host product, and the verdicts against the host path (device = -1) and
planted truth.  32 pairs per workgroup, so n = 1, 33 and 131: a single pair, one past a workgroup, five workgroups with a ragged last one.
All comparisons are exact.  Reference call: packages/helpers/src/chunked-zkey.ts:93-101."""
import ctypes as C
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
from oracle.pyref import bn254_g1 as G1
from oracle.pyref import bn254_g2 as G2

pytestmark = pytest.mark.gpu
R, Q = pairtest.R, pairtest.Q
N = 131
GOLDEN = os.path.join(ROOT, "tests", "golden", "proof_of_twitter")
PKG = os.path.join(ROOT, "zk-email-verify_amd", "py")


def _gpu_points(group, scalars):
    from zkwg import prover
    return bytes(prover.fixed_base(0, group, scalars).cpu().numpy())


def _rand16(n, seed):
    rng = random.Random(seed)
    return b"".join(rng.randrange(1, 1 << 128).to_bytes(16, "little") for _ in range(n))


def _many(fn, args):
    """fn over args on 16 threads (the host pairing's pieces are C calls that release the interpreter)"""
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda a: fn(*a), args))


def _miller_device(g1, g2, n):
    """zkwg_miller_device over the first n pairs -> (rc, [384-byte values], [inside])"""
    import torch
    from zkwg import _call, _lib
    lib = _lib.load()
    d1, d2 = _call.upload(g1[:64 * n], 0), _call.upload(g2[:128 * n], 0)
    f = torch.zeros(384 * n, dtype=torch.uint8, device=d1.device)
    inside = torch.full((n,), 9, dtype=torch.uint8, device=d1.device)
    rc = lib.zkwg_miller_device(0, d1.data_ptr(), d2.data_ptr(), n, f.data_ptr(), inside.data_ptr(), None)
    raw = _call.download(f)
    return rc, [raw[384 * i:384 * i + 384] for i in range(n)], [int(v) for v in _call.download(inside)]


@pytest.fixture(scope="module")
def pairs():
    """131 pairs: infinity on the G1 side at 0, on the G2 side at 70, on both at 130; logarithms 1 and r - 1 at 1 and 2; G2 points outside
    the subgroup at 5 (a raw twist point), 64 (order 10069) and 129 (that point added to a subgroup point)"""
    rng = random.Random(1320)
    l1, l2 = [rng.randrange(1, R) for _ in range(N)], [rng.randrange(1, R) for _ in range(N)]
    l1[0] = l2[70] = l1[130] = l2[130] = 0
    l1[1] = l2[1] = 1
    l1[2] = l2[2] = R - 1
    g1, g2 = _gpu_points(1, l1), bytearray(_gpu_points(2, l2))
    t = verifytest.twist_points(1, 1321)[0]
    small = verifytest.small_order_points(t)[0]
    outside = {5: t, 64: small, 129: G2.add(G2.mul(l2[129], G2.G2), small)}
    for i, p in outside.items():
        g2[128 * i:128 * i + 128] = pairtest.mont2(p)
    return g1, bytes(g2), sorted(outside)


@pytest.fixture(scope="module")
def leaves(pairs):
    g1, g2, _ = pairs
    rc, f, inside = _miller_device(g1, g2, N)
    assert rc == 0
    return f, inside


def test_miller_values_and_subgroup_flags_equal_the_host(pairs, leaves):
    g1, g2, outside = pairs
    f, inside = leaves
    assert inside == [0 if i in outside else 1 for i in range(N)]
    assert inside == [int(v) for v in verifytest.g2_subgroup(g2)]
    for i in (0, 70, 130):
        assert f[i] == pairtest.ONE, i
    idx = [i for i in range(N) if i not in outside]               # (the value of a pair whose G2 point is outside the subgroup is ignored by every caller)
    host = _many(pairtest.host_miller, [(g1[64 * i:64 * i + 64], g2[128 * i:128 * i + 128]) for i in idx])
    want = _many(pairtest.final_exp, [(h,) for h in host])
    got = _many(pairtest.final_exp, [(f[i],) for i in idx])
    assert got == want
    for i in outside + [1, 2, 131 - 1]:                           # the device runs the host build's arithmetic: the same bytes, outsiders included
        assert pairtest.core_miller(g1[64 * i:64 * i + 64], g2[128 * i:128 * i + 128]) == (f[i], bool(inside[i])), i
    for n in (1, 33):
        rc, fn, inn = _miller_device(g1, g2, n)
        assert rc == 0 and fn == f[:n] and inn == inside[:n], n


def test_an_off_curve_point_refuses_the_call(pairs):
    from zkwg import _lib
    g1, g2, _ = pairs
    bad = bytearray(g1[:64 * 33])
    y = int.from_bytes(bad[64 * 16 + 32:64 * 17], "little")
    bad[64 * 16 + 32:64 * 17] = ((y + 1) % Q).to_bytes(32, "little")
    rc, _, _ = _miller_device(bytes(bad), g2, 33)
    assert rc == -1 and "curve" in _lib.load().zkwg_last_error().decode()


@pytest.mark.parametrize("n", [1, 33, 131])
def test_the_product_tree_equals_the_host_product(leaves, n):
    import torch
    from zkwg import _call, _lib
    lib = _lib.load()
    f, _ = leaves
    d_f = _call.upload(b"".join(f[:n]), 0)
    uses = [None, [1] * n] if n == 1 else [None, [0 if i in (0, n // 2, n - 1) else 1 for i in range(n)], [0] * n]
    for use in uses:
        d_use = None if use is None else _call.upload(bytes(use), 0)
        out = (C.c_uint8 * 384)()
        assert lib.zkwg_fq12_product_device(0, d_f.data_ptr(), None if use is None else d_use.data_ptr(), n, out, None) == 0
        want = pairtest.ONE
        for i in range(n):
            if use is None or use[i]:
                want = pairtest.f12_mul(want, f[i])
        assert bytes(out) == want, (n, use is None)
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [1, 4, 5, 17])
def test_the_product_tree_at_edge_words_equals_the_oracle(n):
    """zkwg_fq12_product_device on values the Miller loop never makes -- every stored word q - 1, every 29-bit limb all ones, every word 1,
    c5 alone, c0 alone, random elements -- for one value, exactly one lane pair's fold of 4, one past it, and two tree levels with a ragged
    end; with every value in use and with the first, a middle and the last one switched off.  Expected: the product on Python integers
    (oracle/pyref/bn254_pairing.f12_mul), not the host build of the kernel's header.  Exact."""
    import torch
    from oracle.pyref import bn254_pairing as P
    from zkwg import _call, _lib
    lib = _lib.load()
    fam = [v for _, v in pairtest.f12_edge_family(1341)]
    vals = [fam[i % len(fam)] for i in range(n)]
    d_f = _call.upload(b"".join(vals), 0)
    for use in (None, [0 if i in (0, n // 2, n - 1) else 1 for i in range(n)]):
        d_use = None if use is None else _call.upload(bytes(use), 0)
        out = (C.c_uint8 * 384)()
        assert lib.zkwg_fq12_product_device(0, d_f.data_ptr(), None if use is None else d_use.data_ptr(), n, out, None) == 0
        want = P.F12_ONE
        for i in range(n):
            if use is None or use[i]:
                want = P.f12_mul(want, pairtest.f12_to_oracle(vals[i]))
        assert bytes(out) == pairtest.f12_from_oracle(want), (n, use is None)
    torch.cuda.synchronize()


# ---- verdicts ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy():
    """131 fabricated proofs of a toy key with 3 public inputs: (vkey, publics, the points in the zkey's form, the logarithms)"""
    rng = random.Random(1322)
    key = pairtest.toy_key(3, 1322)
    publics = [[rng.randrange(R) for _ in range(3)] for _ in range(N)]
    logs = [pairtest.fabricate(key, x, rng.randrange(1, R), rng.randrange(1, R)) for x in publics]
    a, b, c = _gpu_points(1, [l[0] for l in logs]), _gpu_points(2, [l[1] for l in logs]), _gpu_points(1, [l[2] for l in logs])
    c_bad = _gpu_points(1, [(l[2] + 1) % R for l in logs])
    return pairtest.G.vkey_json(key), publics, (a, b, c, c_bad)


def _proofs(toy, n, bad=()):
    a, b, c, c_bad = toy[2]
    return [pairtest.proof_bytes_from_mont(a[64 * i:64 * i + 64], b[128 * i:128 * i + 128], (c_bad if i in bad else c)[64 * i:64 * i + 64]) for i in range(n)]


@pytest.mark.parametrize("n,bad", [(1, ()), (1, (0,)), (33, (32,)), (33, tuple(range(33)))], ids=["1-good", "1-bad", "33-last", "33-all"])
def test_verdicts_equal_the_host_path_and_the_planted_truth(toy, n, bad):
    from zkwg import verify
    vkey, publics, _ = toy
    proofs, rand = _proofs(toy, n, bad), _rand16(n, 1323)
    got = verify.verify_batch(vkey, publics[:n], proofs, device=0, rand=rand)
    sec, cnt = verify.stats()
    print("seconds", sec, "counts", cnt)
    assert got == [i not in bad for i in range(n)]
    assert got == verify.verify_batch(vkey, publics[:n], proofs, device=-1, rand=rand)
    assert verify.stats()[1] == cnt                               # the same checks on both paths
    if n == 1:
        assert got == verify.verify_batch(vkey, publics[:n], proofs, device=0)  # rand16 from the operating system


def test_verdicts_of_five_workgroups_with_bad_proofs_an_outsider_and_a_large_public_input(toy):
    from zkwg import verify
    vkey, publics, (a, b, c, _) = toy
    bad = (0, 64, 65, 130)
    proofs, rand = _proofs(toy, N, bad), _rand16(N, 1324)
    small = verifytest.small_order_points(verifytest.twist_points(1, 1325)[0])[0]
    b100 = verifytest.decode_g2(b[128 * 100:128 * 101])
    proofs[100] = pairtest.proof_bytes_from_mont(a[64 * 100:64 * 101], pairtest.mont2(G2.add(b100, small)), c[64 * 100:64 * 101])
    publics = [list(p) for p in publics]
    publics[7][1] += R
    want = [i not in bad + (100, 7) for i in range(N)]
    got = verify.verify_batch(vkey, publics, proofs, device=0, rand=rand)
    sec, cnt = verify.stats()
    print("seconds", sec, "counts", cnt)
    assert got == want and cnt[0] == N - 1 and cnt[2] == 1 and cnt[3] == 5 and cnt[1] <= 1 + 2 * 4 * 8
    assert verify.verify_batch(vkey, publics, proofs, device=-1, rand=rand) == want


def test_the_golden_proof_as_a_batch_of_one_and_of_three():
    from zkwg import verify
    vkey, public, proof = (json.load(open(os.path.join(GOLDEN, f))) for f in ("vkey.json", "public.json", "proof.json"))
    bad_public = [str((int(public[0]) + 1) % R)] + public[1:]
    assert verify.verify_batch(vkey, [public], [proof], device=0) == [True]
    assert verify.verify_batch(vkey, [public, bad_public, public], [proof] * 3, device=0) == [True, False, True]


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
    assert verify.verify_batch(vkey, [pub], [proofs[:256]], device=0) == [True]
    assert verify.verify_batch(vkey, [[str((int(pub[0]) + 1) % R)] + pub[1:]], [proofs[:256]], device=0) == [False]


def test_the_command_line_on_the_device(tmp_path):
    public = json.load(open(os.path.join(GOLDEN, "public.json")))
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = lambda pub: subprocess.run([sys.executable, "-m", "zkwg.verify", os.path.join(GOLDEN, "vkey.json"), pub, os.path.join(GOLDEN, "proof.json"), "--device", "0"],
                                     env=env, capture_output=True, text=True)
    r = run(os.path.join(GOLDEN, "public.json"))
    assert (r.returncode, r.stdout.split()) == (0, ["OK"]), r.stderr
    bad = tmp_path / "public.json"
    bad.write_text(json.dumps([str((int(public[0]) + 1) % R)] + public[1:]))
    r = run(str(bad))
    assert (r.returncode, r.stdout.split()) == (1, ["INVALID"]), r.stderr
