"""Per-proof groth16 verification on the CPU: the final exponentiation of csrc/zkwg_fexp_core.h -- the steps a lane pair of the zk_fexp_*
kernels runs -- against the host's 2,790-bit square-and-multiply (csrc/zkwg_pairing.h zk_pair_final_exp, through tests/native/pairtest.cpp)
BYTE FOR BYTE, its pieces against the oracle's field arithmetic (oracle/pyref) on Python integers, the sum of a proof's public-input points
against the oracle's group law, and the verdicts, rejections, refusals and counts of zkwg_groth16_verify_each's host path (device = -1)
against planted truth, the oracle's verifier and verify_batch.  All comparisons are exact, and no limb-form bound is violated: every new
function claims its contract on entry, so each call below is that function from the top of its contract.
Reference call: packages/helpers/src/chunked-zkey.ts:93-101."""
import copy
import json
import os
import random
import subprocess
import sys

import pytest

import fexptest
import pairtest
import verifytest
from conftest import ROOT
from oracle.pyref import bn254_g1 as G1
from oracle.pyref import bn254_g2 as G2
from oracle.pyref import bn254_pairing as P

R, Q, U = pairtest.R, pairtest.Q, P.U
mont1 = pairtest.mont1
GOLDEN = os.path.join(ROOT, "tests", "golden", "proof_of_twitter")
PKG = os.path.join(ROOT, "zk-email-verify_amd", "py")
ZERO = bytes(384)
to_o, from_o = pairtest.f12_to_oracle, pairtest.f12_from_oracle


def _frob_constants(k):
    return [P.f2_pow(P.XI, j * (Q ** k - 1) // 6) for j in range(6)]


def _frob(f, k):
    """f^(q^k) on the oracle's 6-tuple: every coefficient conjugated (k odd) and multiplied by its constant"""
    return tuple(G2.f2_mul(P.f2_conj(c) if k % 2 else c, g) for c, g in zip(f, _frob_constants(k)))


def _conj(f):
    return tuple(c if j % 2 == 0 else G2.f2_neg(c) for j, c in enumerate(f))


@pytest.fixture(scope="module")
def family():
    """the edge family and what is non-zero of it, as (name, 384 bytes)"""
    return pairtest.f12_edge_family(1401)


@pytest.fixture(scope="module")
def cyclotomic(family):
    """g = easy(f) for the members of the family: values of the cyclotomic subgroup"""
    return [(name, fexptest.easy(v)) for name, v in family]


def test_the_exponent_splits_as_the_header_states():
    h = (Q ** 4 - Q ** 2 + 1) // R
    assert (Q ** 4 - Q ** 2 + 1) % R == 0 and (Q ** 12 - 1) // R == (Q ** 6 - 1) * (Q ** 2 + 1) * h == P.FINAL_EXP
    l2, l1, l0 = 6 * U * U + 1, -(36 * U ** 3 + 18 * U * U + 12 * U - 1), -(36 * U ** 3 + 30 * U * U + 18 * U + 2)
    assert h == Q ** 3 + l2 * Q ** 2 + l1 * Q + l0
    # the chain of the hard part: y0 y1^2 y2^6 y3^12 y4^18 y5^30 y6^36 with the y's exponents in q and u
    y = [Q + Q ** 2 + Q ** 3, -1, U * U * Q * Q, -U * Q, -(U + U * U * Q), -U * U, -(U ** 3 + U ** 3 * Q)]
    assert sum(w * e for w, e in zip((1, 2, 6, 12, 18, 30, 36), y)) == h
    # the digits of u that zk_fexp_power_u walks (ZK_FEXP_U_POS, ZK_FEXP_U_NEG): non-adjacent, 24 non-zero, the top one at bit 62
    pos, neg = 0x450a14044a890a01, 0x0020815000200010
    assert pos - neg == U and pos & neg == 0 and (pos | neg) & ((pos | neg) << 1) == 0 and bin(pos | neg).count("1") == 24 and (pos >> 62) == 1


def test_the_frobenius_table_and_map_equal_the_oracle_and_the_hosts_power(family):
    for k in (1, 2, 3):
        want = _frob_constants(k)
        assert [fexptest.frob_const(k, j) for j in range(6)] == want, k
        assert want[0] == (1, 0) and (k != 2 or all(c[1] == 0 for c in want))
    for name, v in family:
        for k in (1, 2, 3):
            got = fexptest.f12_op(fexptest.FROB1 + k - 1, v)
            assert got == from_o(_frob(to_o(v), k)), (name, k)
            if name.startswith("random"):                         # the two random values: the host's square-and-multiply f^(q^k)
                assert got == fexptest.host_pow(v, Q ** k), (name, k)
        assert fexptest.f12_op(fexptest.CONJ, v) == from_o(_conj(to_o(v))) == fexptest.host_pow(v, Q ** 6), name


def test_the_inverse(family):
    rng = random.Random(1402)
    word = lambda: rng.randrange(Q).to_bytes(32, "little")
    values = list(family) + [("random%d" % i, b"".join(word() for _ in range(12))) for i in range(3, 6)]
    for name, v in values:
        inv = fexptest.f12_inv(v)
        assert pairtest.f12_mul(inv, v) == pairtest.ONE and pairtest.f12_mul(v, inv, True) == pairtest.ONE, name
    assert fexptest.f12_inv(ZERO) == ZERO
    assert fexptest.f12_inv(pairtest.ONE) == pairtest.ONE


def test_the_pieces_of_the_inverse_and_of_the_squaring_equal_the_oracles_arithmetic():
    rng = random.Random(1403)
    m, a, s = G2.f2_mul, G2.f2_add, G2.f2_sub
    r2 = lambda: (rng.randrange(Q), rng.randrange(Q))
    flat = lambda *f2: [c for x in f2 for c in x]
    pairs = lambda v: [tuple(v[i:i + 2]) for i in range(0, len(v), 2)]
    x, y, k = r2(), r2(), r2()
    assert pairs(fexptest.piece(0, flat(x), 2)) == [G2.f2_inv(x)]
    assert fexptest.piece(0, [0, 0], 2) == [0, 0]
    for op in (1, 2):
        assert pairs(fexptest.piece(op, flat(x, y), 4)) == [a(m(x, x), m(m(y, y), P.XI)), m(x, y)]
    assert pairs(fexptest.piece(3, flat(x, y), 2)) == [s(a(a(x, x), x), a(y, y))]
    six = a(a(a(x, x), a(x, x)), a(x, x))
    assert pairs(fexptest.piece(4, flat(x, y), 2)) == [a(six, a(y, y))]
    f = tuple(r2() for _ in range(6))
    assert tuple(pairs(fexptest.piece(5, flat(*f) + flat(k), 12))) == tuple(m(c, k) for c in f)
    # the step that leaves the tower: n in Fq6, N = n^(q^2) n^(q^4) -> 1 / n
    n = (r2(), (0, 0), r2(), (0, 0), r2(), (0, 0))
    n2 = _frob(n, 2)
    big = P.f12_mul(n2, _frob(n2, 2))
    ninv = to_o(fexptest.f12_op(fexptest.NINV, from_o(n) + from_o(big)))
    assert P.f12_mul(ninv, n) == P.F12_ONE
    # an operand of a step as the step wants it
    v = from_o(f)
    want = {1: _conj(f), 2: _frob(f, 1), 3: _frob(f, 2), 4: _frob(f, 3), 5: _frob(_frob(f, 2), 2)}
    for pre, w in want.items():
        assert fexptest.f12_op(fexptest.PRE + pre, v) == from_o(w), pre


def test_the_cyclotomic_squaring_and_the_power_by_u(cyclotomic):
    for name, g in cyclotomic:
        sq = fexptest.f12_op(fexptest.CYC_SQR, g)
        assert sq == pairtest.f12_mul(g, g, True) == pairtest.f12_mul(g, g), name
        assert sq == fexptest.f12_op(fexptest.PRE + 6, g), name
        assert pairtest.f12_mul(fexptest.f12_op(fexptest.CONJ, g), g) == pairtest.ONE, name
        assert fexptest.f12_op(fexptest.POW_U, g) == fexptest.host_pow(g, U), name
    assert fexptest.f12_op(fexptest.CYC_SQR, ZERO) == ZERO and fexptest.f12_op(fexptest.POW_U, ZERO) == ZERO


@pytest.fixture(scope="module")
def miller_values():
    """the core's Miller values of 8 pairs: 6 random ones of known logarithms, then the logarithms 1 and r - 1"""
    rng = random.Random(1404)
    logs = [(rng.randrange(1, R), rng.randrange(1, R)) for _ in range(6)] + [(1, R - 1), (R - 1, 1)]
    out = []
    for a, b in logs:
        f, inside = pairtest.core_miller(mont1(G1.mul(a, G1.G)), pairtest.mont2(G2.mul(b, G2.G2)))
        assert inside
        out.append(f)
    return out


def test_the_final_exponentiation_equals_the_hosts_byte_for_byte(miller_values, family):
    for k, f in enumerate(miller_values):
        assert fexptest.final_exp(f) == pairtest.final_exp(f), k
    for name, v in family:                                        # any non-zero f must agree, not only Miller values
        want = pairtest.final_exp(v)
        assert fexptest.final_exp(v) == want, name
        if name == "c0":
            assert want == pairtest.ONE                           # a value of Fq2 dies in the easy part
    assert fexptest.final_exp(pairtest.ONE) == pairtest.ONE == pairtest.final_exp(pairtest.ONE)
    assert fexptest.final_exp(ZERO) == ZERO == pairtest.final_exp(ZERO)
    # three values folded first, as a proof's three Miller values are
    a, b, c = miller_values[:3]
    assert fexptest.final_exp(a, b, c) == pairtest.final_exp(pairtest.f12_mul(pairtest.f12_mul(a, b), c))
    assert fexptest.final_exp(a, ZERO, c) == ZERO and fexptest.final_exp(pairtest.ONE, pairtest.ONE, pairtest.ONE) == pairtest.ONE


def test_the_sum_of_the_public_input_points_takes_every_branch_of_the_point_formulas():
    """-(IC_0 + the terms) against the oracle's group law: generic summands, a term at infinity (a public input 0), equal summands (the
    doubling inside the mixed addition), opposite summands (infinity on the way), a sum at infinity, and no term at all"""
    rng = random.Random(1405)
    p = [G1.mul(rng.randrange(1, R), G1.G) for _ in range(4)]
    cases = [(p[0], p[1:]), (p[0], [None, p[1], None]), (p[0], [p[0], p[2]]), (p[0], [G1.neg(p[0]), p[3]]), (p[0], [p[1], G1.neg(G1.add(p[0], p[1]))]),
             (p[0], [G1.neg(p[0])]), (p[0], [])]
    for k, (ic0, terms) in enumerate(cases):
        want = ic0
        for t in terms:
            want = G1.add(want, t)
        assert fexptest.vkx(mont1(ic0), [mont1(t) for t in terms]) == mont1(G1.neg(want) if want is not None else None), k


# ---- verdicts of the host path ----------------------------------------------------------------------------------------------------------------
class _Batch:
    """fabricated proofs of a toy key (tests/test_pair_cpu.py's, with public inputs of the caller's choice)"""

    def __init__(self, n_public, seed, n, publics=None):
        rng = random.Random(seed)
        self.key = pairtest.toy_key(n_public, seed)
        self.vkey = pairtest.G.vkey_json(self.key)
        self.publics = publics or [[rng.randrange(R) for _ in range(n_public)] for _ in range(n)]
        self.logs = [pairtest.fabricate(self.key, x, rng.randrange(1, R), rng.randrange(1, R)) for x in self.publics]
        self.points = [(G1.mul(a, G1.G), G2.mul(b, G2.G2), G1.mul(c, G1.G)) for a, b, c in self.logs]

    def raw(self, bad=()):
        """the 256-byte proofs; proof i in `bad` gets pi_c + G"""
        return [pairtest.proof_bytes_from_points(a, b, G1.add(c, G1.G) if i in bad else c) for i, (a, b, c) in enumerate(self.points)]

    def json(self, i):
        return pairtest.proof_json_from_logs(self.logs[i])


def _each(vkey, publics, proofs, reached=None):
    """verify_each on the host path, with the counts every call must show: 3 pairs per proof that reached the stage, those proofs + 1
    for e(alpha, beta) through the new body -- whatever share of them is bad"""
    from zkwg import verify
    got = verify.verify_each(vkey, publics, proofs, device=-1)
    _, cnt = verify.stats_each()
    reached = len(proofs) - cnt[2] if reached is None else reached
    assert cnt[0] == 3 * reached and cnt[1] == (reached + 1 if reached else 0) and cnt[2] == len(proofs) - reached, cnt
    assert cnt[3] == sum(1 for g in got if not g) - cnt[2], cnt
    return got


@pytest.fixture(scope="module")
def golden():
    return tuple(json.load(open(os.path.join(GOLDEN, f))) for f in ("vkey.json", "public.json", "proof.json"))


def test_the_golden_proof_and_its_tampered_forms(golden):
    from zkwg import verify
    vkey, public, proof = golden
    bad_public = [str((int(public[0]) + 1) % R)] + public[1:]
    two_c = copy.deepcopy(proof)
    c2 = G1.add(P.g1_from_json(proof["pi_c"]), P.g1_from_json(proof["pi_c"]))
    two_c["pi_c"] = [str(c2[0]), str(c2[1]), "1"]
    assert _each(vkey, [public], [proof]) == [True]
    assert _each(vkey, [public, bad_public, public, public], [proof, proof, two_c, proof], reached=4) == [True, False, False, True]
    # the host build of the same header, range checks counting
    raw = verify.proof_bytes(proof)
    rc, msg, got, _, cnt = fexptest.verify_each_host(vkey, [public, bad_public, public], [raw] * 3)
    assert (rc, got, cnt) == (0, [True, False, True], [9, 4, 0, 1]), msg
    for args in ((dict(vkey, IC=vkey["IC"][:-1]), [public], [proof]), (vkey, [public[:-1]], [proof]), (vkey, [public, public], [proof])):
        with pytest.raises(verify.VerifyError):
            verify.verify_each(*args, device=-1)
    assert verify.verify_each(vkey, [], [], device=-1) == []


def test_toy_keys_with_0_1_and_3_public_inputs_agree_with_the_oracles_verifier():
    b0 = _Batch(0, 1410, 3)
    assert _each(b0.vkey, b0.publics, b0.raw(bad={1})) == [True, False, True]
    assert P.groth16_verify(b0.vkey, [], b0.json(0)) is True                                                              # oracle call 1
    wrong = pairtest.proof_json_from_logs(pairtest.fabricate(b0.key, [], b0.logs[1][0], b0.logs[1][1], bad=True))
    assert P.groth16_verify(b0.vkey, [], wrong) is False and _each(b0.vkey, [[]], [wrong]) == [False]                     # oracle call 2
    b1 = _Batch(1, 1411, 2)
    assert _each(b1.vkey, b1.publics, b1.raw(bad={0})) == [False, True]
    assert P.groth16_verify(b1.vkey, [str(x) for x in b1.publics[1]], b1.json(1)) is True                                 # oracle call 3
    # three public inputs, among them 0 (its term is the point at infinity), r - 1 and 1
    rng = random.Random(1412)
    publics = [[rng.randrange(R) for _ in range(3)], [0, rng.randrange(R), 0], [0, 0, 0], [R - 1, 1, rng.randrange(R)]]
    b3 = _Batch(3, 1412, 4, publics)
    assert _each(b3.vkey, b3.publics, b3.raw()) == [True] * 4
    assert _each(b3.vkey, b3.publics, [b3.json(i) for i in range(4)]) == [True] * 4
    assert _each(b3.vkey, b3.publics, b3.raw(bad={1, 2})) == [True, False, False, True]
    assert P.groth16_verify(b3.vkey, [str(x) for x in publics[1]], b3.json(1)) is True                                    # oracle call 4
    assert _each(b3.vkey, [publics[0], [1, publics[1][1], 0]] + publics[2:], b3.raw()) == [True, False, True, True]       # a public input changed
    rc, msg, got, _, cnt = fexptest.verify_each_host(b3.vkey, b3.publics, b3.raw(bad={2}))                                # range checks counting
    assert (rc, got, cnt) == (0, [True, True, False, True], [12, 5, 0, 1]), msg
    rc, msg, got, _, cnt = fexptest.verify_each_host(b0.vkey, b0.publics, b0.raw())
    assert (rc, got, cnt) == (0, [True] * 3, [9, 4, 0, 0]), msg


def test_every_rejection_leaves_the_neighbours_alone_and_bad_keys_are_refused():
    from zkwg import verify
    b = _Batch(3, 1413, 5)
    raw = b.raw()
    a, bb, c = b.points[2]
    small = verifytest.small_order_points(verifytest.twist_points(1, 1414)[0])[0]
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
        args = (b.vkey, [b.publics[1], pub, b.publics[3]], [raw[1], proof, raw[3]])
        outside = name == "B outside the subgroup"                # on its curve, so it reaches the stage, and its flag rejects it
        assert _each(*args, reached=3 if outside else 2) == [True, False, True], name
        assert verify.verify_batch(*args, device=-1) == [True, False, True], name
    off = copy.deepcopy(b.vkey)
    off["IC"][1][1] = str((int(off["IC"][1][1]) + 1) % Q)
    with pytest.raises(verify.VerifyError, match="curve"):
        verify.verify_each(off, b.publics, raw, device=-1)
    outside = dict(b.vkey, vk_gamma_2=pairtest.G.g2_json(G2.add(P.g2_from_json(b.vkey["vk_gamma_2"]), small)))
    with pytest.raises(verify.VerifyError, match="subgroup"):
        verify.verify_each(outside, b.publics, raw, device=-1)
    rc, msg, _, _, _ = fexptest.verify_each_host(outside, b.publics, raw)          # the host build of the same header refuses it too
    assert rc == -1 and "subgroup" in msg


@pytest.fixture(scope="module")
def batch16():
    return _Batch(1, 1415, 16)


@pytest.mark.parametrize("bad", [(0,), (15,), (7, 8), tuple(range(16))], ids=["0", "15", "7,8", "all"])
def test_the_verdicts_equal_verify_batch_whatever_share_is_bad(batch16, bad):
    from zkwg import verify
    b, n = batch16, 16
    proofs = b.raw(bad=set(bad))
    got = _each(b.vkey, b.publics, proofs, reached=n)             # (the counts: 48 pairs, 17 values, with 1 bad proof or with 16)
    assert got == [i not in bad for i in range(n)]
    assert got == verify.verify_batch(b.vkey, b.publics, proofs, device=-1)


def test_the_command_line_with_each(golden, tmp_path):
    vkey, public, proof = golden
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = lambda *files: subprocess.run([sys.executable, "-m", "zkwg.verify", *files, "--device", "-1", "--each"], env=env, capture_output=True, text=True)
    g = [os.path.join(GOLDEN, f) for f in ("vkey.json", "public.json", "proof.json")]
    r = run(*g)
    assert (r.returncode, r.stdout.split()) == (0, ["OK"]), r.stderr
    pubs, proofs = tmp_path / "publics.json", tmp_path / "proofs.json"
    pubs.write_text(json.dumps([public, [str((int(public[0]) + 1) % R)] + public[1:]]))
    proofs.write_text(json.dumps([proof, proof]))
    r = run(g[0], str(pubs), str(proofs))
    assert (r.returncode, r.stdout.split()) == (1, ["OK", "INVALID"]), r.stderr


def test_no_limb_form_bound_was_violated():
    assert fexptest.counters() == (0, 0, 0) and pairtest.counters() == (0, 0, 0)
