"""Batched groth16 verification on the CPU: the Miller loop of csrc/zkwg_pair_core.h -- the body a lane pair of zk_pair_miller runs --
against the host pairing (csrc/zkwg_pairing.h) and the oracle (oracle/pyref/bn254_pairing.py), its subgroup flag against the host build of
the subgroup test, and the verdicts, refusals and bisection accounting of zkwg_groth16_verify_batch's host path (device = -1) against planted
truth and the oracle's verifier.  All comparisons are exact, and no limb-form bound is violated.  Reference call:
packages/helpers/src/chunked-zkey.ts:93-101."""
import copy
import json
import math
import os
import random
import subprocess
import sys

import pytest

import pairtest
import verifytest
from conftest import ROOT
from oracle.pyref import bn254_g1 as G1
from oracle.pyref import bn254_g2 as G2
from oracle.pyref import bn254_pairing as P

R, Q = pairtest.R, pairtest.Q
mont1, mont2 = pairtest.mont1, pairtest.mont2
GOLDEN = os.path.join(ROOT, "tests", "golden", "proof_of_twitter")
PKG = os.path.join(ROOT, "zk-email-verify_amd", "py")


def _rand16(n, seed):
    rng = random.Random(seed)
    return b"".join(rng.randrange(1, 1 << 128).to_bytes(16, "little") for _ in range(n))


@pytest.fixture(scope="module")
def pairs():
    """6 random pairs of known logarithms, then the logarithms 1 and r - 1"""
    rng = random.Random(1301)
    logs = [(rng.randrange(1, R), rng.randrange(1, R)) for _ in range(6)] + [(1, R - 1), (R - 1, 1)]
    return logs, [(G1.mul(a, G1.G), G2.mul(b, G2.G2)) for a, b in logs]


@pytest.fixture(scope="module")
def golden():
    return tuple(json.load(open(os.path.join(GOLDEN, f))) for f in ("vkey.json", "public.json", "proof.json"))


def test_the_core_miller_loop_equals_the_host_pairing_and_the_oracle(pairs):
    _, pts = pairs
    for k, (p, q) in enumerate(pts):
        f, inside = pairtest.core_miller(mont1(p), mont2(q))
        want = pairtest.final_exp(pairtest.host_miller(mont1(p), mont2(q)))
        assert inside and pairtest.final_exp(f) == want, k
        if k < 2:
            assert want == pairtest.f12_from_oracle(P.pairing(p, q)), k


def test_bilinearity_of_the_core_miller_values(pairs):
    rng = random.Random(1302)
    a, b = rng.randrange(1, R), rng.randrange(1, R)
    f1, _ = pairtest.core_miller(mont1(G1.mul(a, G1.G)), mont2(G2.mul(b, G2.G2)))
    for extra, want in ((0, True), (1, False)):
        f2, _ = pairtest.core_miller(mont1(G1.mul(-(a * b + extra) % R, G1.G)), mont2(G2.G2))
        for core in (False, True):                               # the host's product and the core's (what zk_pair_product runs)
            assert (pairtest.final_exp(pairtest.f12_mul(f1, f2, core)) == pairtest.ONE) == want, (extra, core)
    assert pairtest.f12_mul(f1, f2, True) == pairtest.f12_mul(f1, f2, False)
    assert pairtest.f12_mul(f1, pairtest.ONE, True) == f1 == pairtest.f12_mul(pairtest.ONE, f1, True)


def test_the_core_product_at_edge_words_equals_the_oracle_and_the_host():
    """every stored word q - 1, every limb all ones, every word 1, c5 alone (the hi / xi path alone), c0 alone, each against itself, against
    each other and against random elements: the expected product is oracle/pyref/bn254_pairing.f12_mul on Python integers"""
    fam = pairtest.f12_edge_family(1340)
    for na, a in fam:
        for nb, b in fam:
            want = pairtest.f12_from_oracle(P.f12_mul(pairtest.f12_to_oracle(a), pairtest.f12_to_oracle(b)))
            assert pairtest.f12_mul(a, b, True) == want, (na, nb)
            assert pairtest.f12_mul(a, b, False) == want, (na, nb)
    assert pairtest.f12_to_oracle(pairtest.f12_from_oracle(P.F12_ONE)) == P.F12_ONE and pairtest.f12_from_oracle(P.F12_ONE) == pairtest.ONE
    assert pairtest.violations() == 0


def test_one_level_of_the_product_tree_as_the_kernel_folds_it_equals_the_oracle():
    """the loop of zk_pair_product (csrc/zkwg_kernels_pair.hip) in the host build, its carried accumulator claimed after every product"""
    fam = [v for _, v in pairtest.f12_edge_family(1341)]
    vals = [fam[i % len(fam)] for i in range(17)]
    for n in (1, 4, 5, 17):
        for use in (None, [0 if i in (0, n // 2, n - 1) else 1 for i in range(n)]):
            want = []
            for j in range(0, n, 4):
                acc = P.F12_ONE
                for i in range(j, min(j + 4, n)):
                    if use is None or use[i]:
                        acc = P.f12_mul(acc, pairtest.f12_to_oracle(vals[i]))
                want.append(pairtest.f12_from_oracle(acc))
            assert pairtest.pair_product(vals[:n], use) == want, (n, use is None)
    assert pairtest.violations() == 0


def test_infinity_on_either_side_gives_exactly_one(pairs):
    _, pts = pairs
    p, q = pts[0]
    for g1, g2 in ((bytes(64), mont2(q)), (mont1(p), bytes(128)), (bytes(64), bytes(128))):
        assert pairtest.core_miller(g1, g2) == (pairtest.ONE, True)
    assert pairtest.core_miller(mont1((p[0], (p[1] + 1) % Q)), mont2(q)) is None         # off the curve: the caller's curve check


def test_the_subgroup_flag_equals_the_subgroup_test(pairs):
    _, pts = pairs
    p, q = pts[1]
    t = verifytest.twist_points(1, 1303)[0]
    small = verifytest.small_order_points(t)[0]                   # order 10069
    outsiders = [t, small, G2.add(q, small)]
    assert verifytest.g2_subgroup(b"".join(mont2(x) for x in outsiders + [q])) == [False, False, False, True]
    for x in outsiders:                                           # the loop runs to its end on them; only the flag means anything
        f, inside = pairtest.core_miller(mont1(p), mont2(x))
        assert inside is False and len(f) == 384
    assert pairtest.core_miller(mont1(p), mont2(q))[1] is True


# ---- verdicts of the host path --------------------------------------------------------------------------------------------------------------
class _Batch:
    """fabricated proofs of a toy key: JSON for the oracle and zkwg.verify, bytes for the host build"""

    def __init__(self, n_public, seed, n):
        rng = random.Random(seed)
        self.key = pairtest.toy_key(n_public, seed)
        self.vkey = pairtest.G.vkey_json(self.key)
        self.publics = [[rng.randrange(R) for _ in range(n_public)] for _ in range(n)]
        self.logs = [pairtest.fabricate(self.key, x, rng.randrange(1, R), rng.randrange(1, R)) for x in self.publics]
        self.points = [(G1.mul(a, G1.G), G2.mul(b, G2.G2), G1.mul(c, G1.G)) for a, b, c in self.logs]

    def raw(self, bad=()):
        """the 256-byte proofs; proof i in `bad` gets pi_c + G"""
        return [pairtest.proof_bytes_from_points(a, b, G1.add(c, G1.G) if i in bad else c) for i, (a, b, c) in enumerate(self.points)]

    def json(self, i):
        return pairtest.proof_json_from_logs(self.logs[i])


@pytest.fixture(scope="module")
def batch3():
    return _Batch(3, 1310, 5)


@pytest.fixture(scope="module")
def batch16():
    return _Batch(1, 1311, 16)


def test_the_golden_proof_and_its_tampered_forms(golden):
    from zkwg import verify
    vkey, public, proof = golden
    rand = _rand16(3, 1304)
    assert verify.verify_batch(vkey, [public], [proof], device=-1, rand=rand[:16]) == [True]
    bad_public = [str((int(public[0]) + 1) % R)] + public[1:]
    two_c = copy.deepcopy(proof)
    c2 = G1.add(P.g1_from_json(proof["pi_c"]), P.g1_from_json(proof["pi_c"]))
    two_c["pi_c"] = [str(c2[0]), str(c2[1]), "1"]
    assert verify.verify(vkey, bad_public, proof) is False and verify.verify(vkey, public, two_c) is False
    assert P.groth16_verify(vkey, public, proof) is True and P.groth16_verify(vkey, public, two_c) is False          # oracle calls 1, 2
    assert verify.verify_batch(vkey, [public, bad_public, public], [proof] * 3, device=-1, rand=rand) == [True, False, True]
    # the host build of the same header, range checks counting
    raw = verify.proof_bytes(proof)
    rc, msg, got, _, cnt = pairtest.verify_batch_host(vkey, [public, bad_public, public], [raw] * 3, rand)
    assert (rc, got) == (0, [True, False, True]) and cnt[3] == 1, msg
    # malformed shapes raise
    short = dict(vkey, IC=vkey["IC"][:-1])
    z2 = dict(proof, pi_a=proof["pi_a"][:2] + ["2"])
    for args in ((short, [public], [proof]), (vkey, [public[:-1]], [proof]), (vkey, [public], [z2]), (vkey, [public, public], [proof])):
        with pytest.raises(verify.VerifyError):
            verify.verify_batch(*args, device=-1)


def test_toy_key_verdicts_agree_with_the_oracle_and_rejections_leave_the_neighbours_alone(batch3):
    from zkwg import verify
    b = batch3
    rand = _rand16(5, 1305)
    assert verify.verify_batch(b.vkey, b.publics, b.raw(), device=-1, rand=rand) == [True] * 5
    assert verify.verify_batch(b.vkey, b.publics, [b.json(i) for i in range(5)], device=-1, rand=_rand16(5, 1306)) == [True] * 5
    assert verify.verify_batch(b.vkey, b.publics, b.raw(bad={1, 4}), device=-1, rand=rand) == [True, False, True, True, False]
    assert verify.verify_batch(b.vkey, b.publics, b.raw(bad={1, 4}), device=-1, rand=_rand16(5, 1307)) == [True, False, True, True, False]
    assert verify.verify_batch(b.vkey, b.publics, b.raw(bad={1, 4}), device=-1) == [True, False, True, True, False]      # rand16 from the operating system
    assert P.groth16_verify(b.vkey, [str(x) for x in b.publics[0]], b.json(0)) is True                                   # oracle call 3
    wrong = pairtest.proof_json_from_logs(pairtest.fabricate(b.key, b.publics[1], b.logs[1][0], b.logs[1][1], bad=True))
    assert P.groth16_verify(b.vkey, [str(x) for x in b.publics[1]], wrong) is False                                      # oracle call 4
    assert verify.verify(b.vkey, b.publics[1], wrong) is False
    # a key with one public input
    b1 = _Batch(1, 1308, 2)
    assert verify.verify_batch(b1.vkey, b1.publics, b1.raw(bad={0}), device=-1, rand=rand[:32]) == [False, True]
    assert P.groth16_verify(b1.vkey, [str(x) for x in b1.publics[1]], b1.json(1)) is True                                # oracle call 5
    # the per-proof rejections: verdict False, the call goes on
    raw = b.raw()
    a, bb, c = b.points[2]
    small = verifytest.small_order_points(verifytest.twist_points(1, 1309)[0])[0]
    cases = {
        "public >= r": (raw[2], [b.publics[2][0] + R] + b.publics[2][1:]),
        "coordinate >= q": (pairtest.proof_bytes_from_points((a[0] + Q, a[1]), bb, c), b.publics[2]),
        "A off its curve": (pairtest.proof_bytes_from_points((a[0], (a[1] + 1) % Q), bb, c), b.publics[2]),
        "B outside the subgroup": (pairtest.proof_bytes_from_points(a, G2.add(bb, small), c), b.publics[2]),
        "all zero": (bytes(256), b.publics[2]),
        "C at infinity": (raw[2][:192] + bytes(64), b.publics[2]),
    }
    assert b.publics[2][0] + R < 1 << 256
    for name, (proof, pub) in cases.items():
        got = verify.verify_batch(b.vkey, [b.publics[1], pub, b.publics[3]], [raw[1], proof, raw[3]], device=-1, rand=rand[:48])
        assert got == [True, False, True], name
        sec, cnt = verify.stats()
        assert cnt[2] + cnt[3] == 1 and (cnt[2] == 0) == (name == "B outside the subgroup"), (name, cnt)
    # the key is refused, never turned into verdicts
    off = copy.deepcopy(b.vkey)
    off["IC"][1][1] = str((int(off["IC"][1][1]) + 1) % Q)
    with pytest.raises(verify.VerifyError, match="curve"):
        verify.verify_batch(off, b.publics, raw, device=-1, rand=rand)
    outside = dict(b.vkey, vk_gamma_2=pairtest.G.g2_json(G2.add(P.g2_from_json(b.vkey["vk_gamma_2"]), small)))
    with pytest.raises(verify.VerifyError, match="subgroup"):
        verify.verify_batch(outside, b.publics, raw, device=-1, rand=rand)
    with pytest.raises(verify.VerifyError):                       # a zero entry of rand16: ZKWG_RC_BAD_ARG
        verify.verify_batch(b.vkey, b.publics, raw, device=-1, rand=rand[:16] + bytes(16) + rand[32:])
    assert verify.verify_batch(b.vkey, [], [], device=-1) == []


@pytest.mark.parametrize("bad", [(), (0,), (15,), (7, 8), tuple(range(16))], ids=["none", "0", "15", "7,8", "all"])
def test_bisection_finds_the_bad_proofs_within_the_stated_number_of_checks(batch16, bad):
    b, n = batch16, 16
    rc, msg, got, sec, cnt = pairtest.verify_batch_host(b.vkey, b.publics, b.raw(bad=set(bad)), _rand16(n, 1312))
    assert rc == 0 and got == [i not in bad for i in range(n)], msg
    bound = min(2 * n - 1, 1 + 2 * len(bad) * math.ceil(math.log2(n)))
    print("final exponentiations", cnt[1], "bound", bound)
    assert cnt[0] == n and cnt[2] == 0 and cnt[3] == len(bad)
    assert cnt[1] <= bound and (cnt[1] == 1) == (not bad)


def test_no_limb_form_bound_was_violated():
    assert pairtest.violations() == 0


def test_the_command_line_exits_0_on_the_golden_proof_and_1_on_a_tampered_one(golden, tmp_path):
    vkey, public, proof = golden
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = lambda *files: subprocess.run([sys.executable, "-m", "zkwg.verify", *files, "--device", "-1"], env=env, capture_output=True, text=True)
    g = [os.path.join(GOLDEN, f) for f in ("vkey.json", "public.json", "proof.json")]
    r = run(*g)
    assert (r.returncode, r.stdout.split()) == (0, ["OK"]), r.stderr
    bad = tmp_path / "public.json"
    bad.write_text(json.dumps([str((int(public[0]) + 1) % R)] + public[1:]))
    r = run(g[0], str(bad), g[2])
    assert (r.returncode, r.stdout.split()) == (1, ["INVALID"]), r.stderr
    pubs, proofs = tmp_path / "publics.json", tmp_path / "proofs.json"
    pubs.write_text(json.dumps([public, json.loads(bad.read_text())]))
    proofs.write_text(json.dumps([proof, proof]))
    r = run(g[0], str(pubs), str(proofs))
    assert (r.returncode, r.stdout.split()) == (1, ["OK", "INVALID"]), r.stderr
