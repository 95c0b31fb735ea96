"""`powersoftau verify` on the CPU: the host pairing of csrc/zkwg_pairing.h against the oracle pairing (oracle/pyref/bn254_pairing.py) and
the golden snarkjs proof, and the G2 subgroup criterion of csrc/zkwg_verify_core.h -- the body a lane pair of zk_verify_g2_subgroup runs --
against the DEFINITION [r] Q = infinity by plain double-and-add.  All comparisons are exact, and no limb-form bound is violated."""
import json
import os
import random

import pytest

import setuptest
import verifytest
from conftest import ROOT
from oracle.pyref import bn254_g1 as G1
from oracle.pyref import bn254_g2 as G2
from oracle.pyref import bn254_pairing as P

R, Q = verifytest.R, verifytest.Q
mont1, mont2 = setuptest.mont1, setuptest.mont2


@pytest.fixture(scope="module")
def six_pairs():
    """6 random pairs with their oracle pairings (computed once)"""
    rng = random.Random(1101)
    pairs = [(G1.mul(rng.randrange(1, R), G1.G), G2.mul(rng.randrange(1, R), G2.G2)) for _ in range(6)]
    return pairs, [P.pairing(p, q) for p, q in pairs]


def test_pairing_equals_the_oracle_on_random_pairs_and_their_products(six_pairs):
    pairs, want = six_pairs
    for (p, q), w in zip(pairs, want):
        rc, msg, got = verifytest.pairing([(mont1(p), mont2(q))])
        assert rc == 0 and got == w, msg
    for idx in ((0, 1), (2, 3, 4), (0, 1, 2, 3, 4, 5)):
        prod = P.F12_ONE
        for i in idx:
            prod = P.f12_mul(prod, want[i])
        rc, msg, got = verifytest.pairing([(mont1(pairs[i][0]), mont2(pairs[i][1])) for i in idx])
        assert rc == 0 and got == prod, (idx, msg)
    # bilinearity through the check itself: e(a P, Q) e(-P, a Q) = 1, and not with another scalar
    a = 0x1234567890abcdef1234567890abcdef
    p, q = pairs[0]
    assert verifytest.pairing_check([(mont1(G1.mul(a, p)), mont2(q)), (mont1(G1.neg(p)), mont2(G2.mul(a, q)))]) == (0, "", True)
    assert verifytest.pairing_check([(mont1(G1.mul(a, p)), mont2(q)), (mont1(G1.neg(p)), mont2(G2.mul(a + 1, q)))]) == (0, "", False)


def test_the_golden_proof_verifies_as_one_four_pair_product_and_no_changed_point_does():
    d = os.path.join(ROOT, "tests", "golden", "proof_of_twitter")
    vkey, public, proof = (json.load(open(os.path.join(d, f))) for f in ("vkey.json", "public.json", "proof.json"))
    ic = [P.g1_from_json(v) for v in vkey["IC"]]
    vk_x = ic[0]
    for x, base in zip((int(v) for v in public), ic[1:]):
        vk_x = G1.add(vk_x, G1.mul(x, base))
    a, b, c = P.g1_from_json(proof["pi_a"]), P.g2_from_json(proof["pi_b"]), P.g1_from_json(proof["pi_c"])
    alpha, beta = P.g1_from_json(vkey["vk_alpha_1"]), P.g2_from_json(vkey["vk_beta_2"])
    gamma, delta = P.g2_from_json(vkey["vk_gamma_2"]), P.g2_from_json(vkey["vk_delta_2"])
    pairs = [(G1.neg(a), b), (alpha, beta), (vk_x, gamma), (c, delta)]
    enc = lambda ps: [(mont1(p), mont2(q)) for p, q in ps]
    assert verifytest.pairing_check(enc(pairs)) == (0, "", True)
    for k in range(4):                                            # any one point changed (to another point of its group)
        for side in (0, 1):
            ch = [list(pq) for pq in pairs]
            ch[k][side] = G1.add(ch[k][0], G1.G) if side == 0 else G2.add(ch[k][1], G2.G2)
            assert verifytest.pairing_check(enc(ch)) == (0, "", False), (k, side)
    # e(alpha, beta) in snarkjs' convention is the stored vk_alphabeta_12
    rc, _, got = verifytest.pairing([(mont1(alpha), mont2(beta))])
    assert rc == 0 and P.to_snarkjs_f12(P.f12_pow(got, P.FC_EXPONENT % R)) == vkey["vk_alphabeta_12"]


def test_pairing_edge_cases(six_pairs):
    pairs, want = six_pairs
    (p, q), w = pairs[0], want[0]
    one = tuple(P.F12_ONE)
    assert verifytest.pairing([])[2] == one
    assert verifytest.pairing([(bytes(64), mont2(q))])[2] == one and verifytest.pairing([(mont1(p), bytes(128))])[2] == one
    assert verifytest.pairing([(bytes(64), bytes(128)), (mont1(p), mont2(q)), (mont1(p), bytes(128))])[2] == w
    assert verifytest.pairing_check([(bytes(64), mont2(q))]) == (0, "", True)
    # refusals: not reduced, off the curve, outside the subgroup
    big = bytearray(mont1(p))
    big[0:32] = (int.from_bytes(big[0:32], "little") + Q).to_bytes(32, "little")
    for g1, g2 in ((bytes(big), mont2(q)), (mont1((p[0], (p[1] + 1) % Q)), mont2(q)), (mont1(p), mont2((q[0], G2.f2_add(q[1], (0, 1)))))):
        rc, msg, val = verifytest.pairing_check([(mont1(p), mont2(q)), (g1, g2)])
        assert rc == -1 and "curve" in msg and "pair 1" in msg and val is None
    t = verifytest.twist_points(1, 1102)[0]
    for outside in (t, verifytest.small_order_points(t)[0], G2.add(q, verifytest.small_order_points(t)[0])):
        assert G2.on_curve(outside)
        rc, msg, val = verifytest.pairing_check([(mont1(p), mont2(outside))])
        assert rc == -1 and "subgroup" in msg and val is None


def test_the_subgroup_criterion_equals_the_definition():
    rng = random.Random(1103)
    inside = [G2.mul(rng.randrange(1, R), G2.G2) for _ in range(30)] + [G2.G2, G2.neg(G2.G2)]
    raw = verifytest.twist_points(8, 1104)
    small = [s for t in raw[:3] for s in verifytest.small_order_points(t)]
    assert all(s is not None for s in small)
    for t in raw[:3]:                                             # the orders are what the names say
        s = verifytest.small_order_points(t)
        assert [verifytest.plain_mul(m, x) for m, x in zip(verifytest.SMALL, s)] == [None] * 3
        assert verifytest.plain_mul(10069, s[2]) is not None and verifytest.plain_mul(5864401, s[2]) is not None
    mixed = [G2.add(inside[i], s) for i, s in enumerate(small)]
    points = inside + [None] + raw + small + mixed
    assert all(G2.on_curve(p) for p in points)
    want = [verifytest.plain_mul(R, p) is None for p in points]   # the definition
    assert want == [True] * 33 + [False] * (8 + 9 + 9)
    before = verifytest.violations()
    got = verifytest.g2_subgroup(b"".join(mont2(p) for p in points))
    assert got == want
    assert verifytest.violations() == before == 0
    # the walk every lane shares: the non-adjacent form of u
    length, nz = verifytest.u_digits()
    assert (length, nz) == (63, 24), (length, nz)
    # off the curve: refused
    bad = bytearray(mont2(inside[0]))
    bad[70] ^= 1
    assert verifytest.g2_subgroup(mont2(inside[1]) + bytes(bad)) is None


# ---- zkwg.ptau.verify over host mirrors ------------------------------------------------------------------------------------------------------
POWER = 3


def _host_backend(mp):
    """zkwg.ptau with every device call replaced by its host mirror (as tests/test_ptau_key_cpu.py does for a contribution)"""
    import torch
    import phase2test
    import ptaukeytest
    from zkwg import phase2, prover, ptau
    mp.setattr(phase2, "scale_points", lambda group, pts, s, device=0: phase2test.scale(group, pts, s))
    mp.setattr(prover, "fixed_base", lambda device, group, scalars: torch.frombuffer(bytearray(setuptest.host_points(group, scalars)), dtype=torch.uint8))

    def apply_key(data, tau, alpha, beta, s7, device=0):
        rc, msg, out = ptaukeytest.apply_key(data, tau, alpha, beta, s7, piece=16)
        if rc != 0:
            raise ptau.PtauError(msg)
        return out
    mp.setattr(ptau, "apply_key", apply_key)
    mp.setattr(ptau, "_backend", lambda device: verifytest.HostBackend())


@pytest.fixture(scope="module")
def files():
    """new -> contribute -> beacon at POWER, its prepared form and the prepared form of POWER - 1, on the host mirrors (which stay in
    place for the module's verifications)"""
    import ptautest
    from zkwg import ptau
    mp = pytest.MonkeyPatch()
    _host_backend(mp)
    seed = bytes(range(64))
    p0 = ptau.new(POWER)
    p1 = ptau.contribute(p0, "alice", "entropy", urandom=lambda n: seed[:n])
    p2 = ptau.beacon(p1, "the beacon", "0102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f20", 10)
    rc, msg, prepared = ptautest.prepare(p2)
    assert rc == 0, msg
    rc, msg, cut = ptautest.prepare(p2, POWER - 1)
    assert rc == 0, msg
    yield {"new": p0, "one": p1, "two": p2, "prepared": prepared, "cut": cut}
    mp.undo()


def _verify(data, seed=1105):
    from zkwg import ptau
    rng = random.Random(seed)
    res = ptau.verify(data, urandom=lambda n: rng.randbytes(n))
    assert res["ok"] == all(ok is not False for _, ok, _ in res["checks"])
    return res, {name: ok for name, ok, _ in res["checks"]}


def _failed(checks):
    return {name for name, ok in checks.items() if ok is False}


_reseal, _with_records, _swap, _map_g2 = verifytest.reseal, verifytest.with_records, verifytest.swap_points, verifytest.map_g2


def test_good_files_pass_every_check_in_every_state(files):
    names = ["structure", "points", "subgroup", "anchors", "powers_2", "powers_3", "powers_4", "powers_5", "beta"]
    lagrange = ["lagrange_12", "lagrange_13", "lagrange_14", "lagrange_15"]
    tail = ["last_record", "last_challenge"]
    before = verifytest.violations()
    res, checks = _verify(files["new"])
    assert res["ok"] and list(checks) == names and all(checks.values()) and "no contributions" in res["checks"][0][2]
    res, checks = _verify(files["one"])
    assert res["ok"] and list(checks) == names + ["record_1"] + tail and all(checks.values())
    res, checks = _verify(files["two"])
    assert res["ok"] and list(checks) == names + ["record_1", "record_2"] + tail and all(checks.values())
    assert "beacon" in dict((n, d) for n, _, d in res["checks"])["record_2"]
    res, checks = _verify(files["prepared"])
    assert res["ok"] and list(checks) == names + ["record_1", "record_2"] + tail + lagrange and all(checks.values())
    assert dict((n, d) for n, _, d in res["checks"])["lagrange_12"] == f"{POWER + 2} levels"
    # a file cut to a smaller power: the hash of the last link covers sections that are gone
    res, checks = _verify(files["cut"])
    assert res["ok"] and checks["last_challenge"] is None and dict((n, d) for n, _, d in res["checks"])["last_challenge"] == "skipped (truncated)"
    assert all(ok for name, ok in checks.items() if name != "last_challenge") and "lagrange_15" in checks
    assert verifytest.violations() == before == 0


@pytest.mark.parametrize("sid", [2, 3, 4, 5])
def test_two_swapped_points_of_a_section_fail_its_powers_check_alone(files, sid):
    res, checks = _verify(_reseal(_swap(files["two"], sid, 4, 5)))
    assert not res["ok"] and _failed(checks) == {f"powers_{sid}"}, res
    # without the helper's new hash the chain's last link breaks as well
    assert _failed(_verify(_swap(files["two"], sid, 4, 5))[1]) == {f"powers_{sid}", "last_challenge"}


def test_a_point_outside_the_subgroup_fails_the_subgroup_check_alone(files):
    small = verifytest.small_order_points(verifytest.twist_points(1, 1106)[0])[0]
    assert small is not None and verifytest.plain_mul(10069, small) is None
    res, checks = _verify(_reseal(_map_g2(files["two"], 3, 5, lambda p: G2.add(p, small))))
    assert not res["ok"] and _failed(checks) == {"subgroup"}, res
    assert checks["powers_3"] is None                             # no pairing is defined on such a sum: skipped, and `subgroup` says why
    assert "section 3: 1 point outside the subgroup, the first at 5" in dict((n, d) for n, _, d in res["checks"])["subgroup"]


def test_section_6_doubled_fails_beta(files):
    """(the record holds beta_g2 too, so `last_record` sees the same change: no single check can fail alone here)"""
    res, checks = _verify(_reseal(_map_g2(files["two"], 6, 0, lambda p: G2.add(p, p))))
    assert not res["ok"] and checks["beta"] is False and _failed(checks) == {"beta", "last_record"}, res


def test_a_changed_proof_of_knowledge_fails_its_record_alone(files):
    from zkwg import ptau
    recs = ptau.read_contributions(files["two"])
    first = dict(recs[0])
    first["tau_g2_spx"] = mont2(G2.mul(5, G2.G2))
    res, checks = _verify(_with_records(files["two"], [ptau.pack_record(first), recs[1]["raw"]]))
    assert not res["ok"] and _failed(checks) == {"record_1"}, res
    assert "tau: proof of knowledge" in dict((n, d) for n, _, d in res["checks"])["record_1"]


def test_a_changed_byte_of_the_last_challenge_fails_the_last_link_alone(files):
    from zkwg import ptau
    recs = ptau.read_contributions(files["two"])
    last = dict(recs[1])
    last["next_challenge"] = bytes([last["next_challenge"][0] ^ 1]) + last["next_challenge"][1:]
    res, checks = _verify(_with_records(files["two"], [recs[0]["raw"], ptau.pack_record(last)]))
    assert not res["ok"] and _failed(checks) == {"last_challenge"}, res


@pytest.mark.parametrize("sid", [12, 13, 14, 15])
def test_two_swapped_points_of_a_lagrange_level_fail_its_check_alone(files, sid):
    res, checks = _verify(_swap(files["prepared"], sid, 1, 2, first=(1 << 2) - 1))      # level 2
    assert not res["ok"] and _failed(checks) == {f"lagrange_{sid}"}, res
    assert "level 2 " in dict((n, d) for n, _, d in res["checks"])[f"lagrange_{sid}"]


def test_a_section_of_infinity_and_a_point_off_its_curve_fail_the_points_check(files):
    from zkwg import ptau
    o, size = ptau.read_any(files["two"])[0]["sections"][4]
    res, checks = _verify(_reseal(files["two"][:o] + bytes(size) + files["two"][o + size:]))
    assert not res["ok"] and _failed(checks) == {"points"} and list(checks)[-1] == "points", res
    for sid, state in ((2, "two"), (3, "two"), (6, "two"), (13, "prepared"), (15, "prepared")):
        o, size = ptau.read_any(files[state])[0]["sections"][sid]
        b = bytearray(files[state])
        b[o + size - 40] ^= 4
        res, checks = _verify(bytes(b))
        assert not res["ok"] and checks["points"] is False and list(checks)[-1] == "points" and f"section {sid}" in res["checks"][-1][2], (sid, res)


def test_a_broken_container_fails_the_structure_check(files):
    for bad in (files["two"][:-30], b"ptbu" + files["two"][4:], files["two"][:-1]):
        res, checks = _verify(bad)
        assert not res["ok"] and list(checks) == ["structure"] and checks["structure"] is False
