"""`powersoftau new / contribute / beacon` on the device (zkwg.ptau -> zkwg_point_mul_device / zkwg_point_powers_device /
zkwg_ptau_apply_key -> csrc/zkwg_kernels_ptau_key.hip): each point times its own scalar against known logarithms and the host mirror, a
power-9 file against the host mirror in every byte, contributions against the toy ceremony of the product keys, and the whole workflow
from nothing but generators:  new -> contribute -> beacon -> prepare -> setup.new_zkey -> phase 2 -> prove, accepted by the PINNED
verifier (oracle/pyref/bn254_pairing.py).  All comparisons are exact (the points are canonical affine: no tolerance anywhere)."""
import json
import random

import pytest

import ptaukeytest
import ptautest
import setuptest
import zkeytest
from oracle.pyref import bn254_pairing as P

R = ptaukeytest.R
EDGES = ptaukeytest.EDGES


def _gpu_points(group, scalars):
    from zkwg import prover
    return bytes(prover.fixed_base(0, group, scalars).cpu().numpy())


def _sections(data):
    from zkwg import ptau
    sec = ptau.read_ptau(data, prepared=False)["sections"]
    return {sid: bytes(data[o:o + size]) for sid, (o, size) in sec.items()}


@pytest.fixture(scope="module")
def points():
    """4,099 G1 and 2,051 G2 points of known logarithms (not a multiple of 64 / 32, several workgroups), infinity among them, and their scalars"""
    rng = random.Random(61)
    out = {}
    for group, n in ((1, 4099), (2, 2051)):
        logs = [rng.randrange(1, R) for _ in range(n)]
        logs[0] = logs[70] = logs[n - 1] = 0                      # infinity, the first and the last point included
        logs[1], logs[2] = 1, R - 1
        scalars = EDGES + [rng.randrange(R) for _ in range(n - 2 * len(EDGES))] + EDGES       # the edges in the first and in the last wavefront
        scalars[70] = R - 1
        out[group] = (logs, scalars, _gpu_points(group, logs))
    return out


@pytest.mark.gpu
def test_gpu_point_mul_device_equals_the_known_logarithms_and_the_host_mirror(points):
    from zkwg import ptau
    for group, pt, head in ((1, 64, 256), (2, 128, 128)):
        logs, scalars, pts = points[group]
        got = ptau.point_mul(group, pts, scalars)
        assert got == _gpu_points(group, [a * s % R for a, s in zip(logs, scalars)]), group          # every byte
        assert got[:pt] == bytes(pt) and got[-pt:] == bytes(pt)
        assert got[:pt * head] == ptaukeytest.mul(group, pts[:pt * head], scalars[:head]), group
        assert ptau.point_mul(group, pts[:pt * 3], [s + R for s in scalars[:3]]) == got[:pt * 3]     # reduced modulo r
        assert ptau.point_mul(group, b"", []) == b""
    assert ptaukeytest.violations() == 0


@pytest.mark.gpu
def test_gpu_point_powers_device_equals_its_halves_and_point_mul(points):
    from zkwg import ptau
    rng = random.Random(62)
    for group, pt, n in ((1, 64, 2050), (2, 128, 1026)):
        pts = points[group][2][:pt * n]
        c, t = rng.randrange(1, R), rng.randrange(1, R)
        whole = ptau.point_powers(group, pts, c, t)
        assert whole == ptau.point_powers(group, pts[:pt * (n // 2)], c, t, 0) + ptau.point_powers(group, pts[pt * (n // 2):], c, t, n // 2), group
        assert whole == ptau.point_mul(group, pts, [c * pow(t, k, R) % R for k in range(n)]), group
        first = (1 << 33) + 5                                     # an index above 2^32, and the keys reduced modulo r
        assert ptau.point_powers(group, pts[:pt * 130], c + R, t + R, first) == ptau.point_mul(group, pts[:pt * 130], [c * pow(t, first + k, R) % R for k in range(130)]), group
        for bad in ((0, t), (c, 0), (R, t)):
            with pytest.raises(ptau.PtauError):
                ptau.point_powers(group, pts[:pt], *bad)


@pytest.mark.gpu
def test_gpu_in_place_and_a_bad_point_leaves_the_buffer_as_it_was(points):
    import torch
    from zkwg import _lib, ptau
    lib = _lib.load()
    for group, pt in ((1, 64), (2, 128)):
        logs, scalars, pts = points[group]
        n = len(logs)
        d = torch.frombuffer(bytearray(pts), dtype=torch.uint8).cuda()
        k = torch.frombuffer(bytearray(b"".join(int(s).to_bytes(32, "little") for s in scalars)), dtype=torch.uint8).cuda()
        assert lib.zkwg_point_mul_device(0, group, d.data_ptr(), n, k.data_ptr(), d.data_ptr(), 0) == 0            # d_out == d_points
        assert bytes(d.cpu().numpy()) == ptau.point_mul(group, pts, scalars), group
        bad = bytearray(pts)
        bad[pt * (n // 2) + 5] ^= 1                               # a point in the middle
        d = torch.frombuffer(bytearray(bad), dtype=torch.uint8).cuda()
        assert lib.zkwg_point_mul_device(0, group, d.data_ptr(), n, k.data_ptr(), d.data_ptr(), 0) == -1
        assert b"curve" in lib.zkwg_last_error() and bytes(d.cpu().numpy()) == bytes(bad), group
        one = (1).to_bytes(32, "little")
        assert lib.zkwg_point_powers_device(0, group, d.data_ptr(), n, one, one, 0, d.data_ptr(), 0) == -1
        assert b"curve" in lib.zkwg_last_error() and bytes(d.cpu().numpy()) == bytes(bad), group
        assert lib.zkwg_point_mul_device(0, group, d.data_ptr() + 8, 1, k.data_ptr(), d.data_ptr(), 0) == -2      # alignment: BAD_ARG
        with pytest.raises(ptau.PtauError, match="curve"):
            ptau.point_mul(group, bytes(bad), scalars)


PIECES = {1: 1 << 20, 2: 1 << 19}                 # ZK_KEY_PIECE_G1 / ZK_KEY_PIECE_G2 (csrc/zkwg_ptau_key_core.h): the points of one piece


@pytest.mark.gpu
def test_gpu_point_powers_device_over_two_pieces_equals_its_single_piece_halves():
    """piece + 1 points: the smallest call that checks every piece first and then brings each to the tables' form again"""
    import torch
    from zkwg import _lib, ptau
    lib = _lib.load()
    rng = random.Random(64)
    le = lambda v: int(v).to_bytes(32, "little")
    for group, pt in ((1, 64), (2, 128)):
        piece = PIECES[group]
        n = piece + 1
        g, t0 = ptau.generators()[group - 1], rng.randrange(2, R)
        pts = ptau.point_powers(group, g * piece, 1, t0) + ptau.point_powers(group, g, 1, t0, piece)      # t0^i G, from single-piece calls
        c, t = rng.randrange(1, R), rng.randrange(2, R)
        whole = ptau.point_powers(group, pts, c, t)
        assert whole == ptau.point_powers(group, pts[:pt * piece], c, t, 0) + ptau.point_powers(group, pts[pt * piece:], c, t, piece), group
        at = (0, piece - 1, piece)
        pick = lambda b: b"".join(b[pt * i:pt * i + pt] for i in at)
        assert pick(whole) == ptaukeytest.mul(group, pick(pts), [c * pow(t, i, R) % R for i in at]), group
        d = torch.frombuffer(bytearray(pts), dtype=torch.uint8).cuda()
        assert lib.zkwg_point_powers_device(0, group, d.data_ptr(), n, le(c), le(t), 0, d.data_ptr(), 0) == 0      # d_out == d_points
        assert bytes(d.cpu().numpy()) == whole, group
        del pts, whole, d
    assert ptaukeytest.violations() == 0


@pytest.mark.gpu
def test_gpu_apply_key_on_a_power_9_file_equals_the_host_mirror():
    from zkwg import ptau
    rng = random.Random(63)
    tau, alpha, beta = (rng.randrange(1, R) for _ in range(3))
    pot = ptautest.toy_ceremony(9, rng.randrange(1, R), rng.randrange(1, R), rng.randrange(1, R), _gpu_points, ceremony_power=11, contributions=b"before")
    got = ptau.apply_key(pot, tau, alpha, beta, b"the record")
    rc, msg, want = ptaukeytest.apply_key(pot, tau, alpha, beta, b"the record", piece=300)
    assert rc == 0, msg
    assert got == want                                            # every byte of the file
    info = ptau.read_ptau(got, prepared=False)
    assert (info["power"], info["ceremony_power"]) == (9, 11) and list(info["sections"]) == [1, 2, 3, 4, 5, 6, 7]
    assert _sections(got)[7] == b"the record" and _sections(got)[1] == _sections(pot)[1]
    st = ptau.apply_key_stats()
    assert all(st[sid]["walk"] > 0 and st[sid]["dbl"] > st[sid]["add"] > 0 for sid in (2, 3, 4, 5))
    for bad in ((0, alpha, beta), (tau, R, beta), (tau, alpha, 0)):
        with pytest.raises(ptau.PtauError, match="0 modulo"):
            ptau.apply_key(pot, *bad, b"")
    with pytest.raises(ptau.PtauError, match="already prepared"):
        ptau.apply_key(ptau.prepare(ptau.truncate(pot, 3)), tau, alpha, beta, b"")
    with pytest.raises(ptau.PtauError, match="past the end"):
        ptau.apply_key(pot[:-30], tau, alpha, beta, b"")
    for sid in (3, 5, 6):
        b = bytearray(pot)
        b[info["sections"][sid][0] + 70] ^= 2                     # (the output's sections sit where the input's did: "before" -> "the record" moves section 7 only)
        with pytest.raises(ptau.PtauError, match="curve"):
            ptau.apply_key(bytes(b), tau, alpha, beta, b"")
    assert ptaukeytest.violations() == 0


@pytest.fixture(scope="module")
def ceremony():
    """new(9) -> contribute (seeded urandom) -> beacon, and the keys of both"""
    from zkwg import phase2, ptau
    seed = bytes(range(100, 164))
    p0 = ptau.new(9)
    p1 = ptau.contribute(p0, "first", b"text", urandom=lambda n: seed[:n])
    p2 = ptau.beacon(p1, "beacon", bytes(range(32)), 10)
    k1 = ptau.key_scalars(seed + b"text")[0]
    k2 = ptau.key_scalars(phase2.beacon_seed(bytes(range(32)), 10))[0]
    return p0, p1, p2, k1, k2


@pytest.mark.gpu
def test_gpu_contribute_then_beacon_equal_the_toy_ceremony_of_the_product_keys(ceremony):
    from zkwg import ptau
    p0, p1, p2, k1, k2 = ceremony
    assert _sections(p0)[2][:64] == _gpu_points(1, [1]) and _sections(p0)[6] == _gpu_points(2, [1])         # the generators of zkwg_fixed_base_device
    want1 = _sections(ptautest.toy_ceremony(9, *k1, _gpu_points))
    want2 = _sections(ptautest.toy_ceremony(9, *(a * b % R for a, b in zip(k1, k2)), _gpu_points))
    for sid in (1, 2, 3, 4, 5, 6):
        assert _sections(p1)[sid] == want1[sid], sid
        assert _sections(p2)[sid] == want2[sid], sid
    recs = ptau.read_contributions(p2)
    assert [(r["name"], r["type"]) for r in recs] == [("first", None), ("beacon", 1)] and ptau.read_contributions(p1) == recs[:1]
    assert recs[1]["tau_g1"] == want2[2][64:128] and recs[1]["beta_g2"] == want2[6]
    assert recs[0]["next_challenge"] == ptau.current_challenge(p1) != ptau.current_challenge(p0)
    assert ptau.beacon(p1, "beacon", bytes(range(32)).hex(), 10) == p2                                    # a beacon is reproducible


@pytest.fixture(scope="module")
def world():
    from zkwg import r1cs as zr
    n_public = 4
    n_wires, cons, w = setuptest.system(seed=33, n_in=24, n_public=n_public, n_cons=220, degrees=[(20, 70)])
    assert setuptest.satisfied(cons, w)
    return {"n_public": n_public, "w": w, "r1cs": zr.write_r1cs(n_wires, cons, n_pub_out=2, n_pub_in=2, n_prv_in=20)}


@pytest.mark.gpu
def test_gpu_from_generators_to_an_accepted_proof(world):
    from zkwg import phase2, prover, ptau, setup, zkey
    pot = ptau.beacon(ptau.contribute(ptau.new(8), "one"), "two", "00ff" * 16, 10)
    z = phase2.contribute(setup.new_zkey(world["r1cs"], ptau.prepare(pot)), "three")
    w, n_public = world["w"], world["n_public"]
    wp = prover.WitnessProver(z, device=0, slots=2)
    st, proofs = wp.prove(zkeytest.wit_bytes(w), [(12345, 67890)])
    assert st == [0]
    pub = wp.public_signals(zkeytest.wit_bytes(w))
    assert pub == [str(w[i]) for i in range(1, n_public + 1)]
    pj = prover.Prover.proof_json(proofs[0])
    vk = zkey.verification_key(z)
    assert P.groth16_verify(vk, pub, pj)
    bad = list(pub)
    bad[1] = str((int(bad[1]) + 1) % R)
    assert not P.groth16_verify(vk, bad, pj)
    del wp


@pytest.mark.gpu
def test_gpu_the_command_lines_in_a_row(tmp_path, capsys):
    from zkwg import ptau
    f = lambda name: str(tmp_path / name)
    assert ptau.main(["new", "5", f("pot_0000.ptau")]) == 0
    assert ptau.main(["new", "0", f("x.ptau")]) == 1
    assert ptau.main(["contribute", f("pot_0000.ptau"), f("pot_0001.ptau"), "--name", "cli", "--entropy", "some text"]) == 0
    assert ptau.main(["beacon", f("pot_0001.ptau"), f("pot_beacon.ptau"), "0102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f", "10", "--name", "final"]) == 0
    assert ptau.main(["beacon", f("pot_0001.ptau"), f("x.ptau"), "01", "9", "--name", "final"]) == 1
    capsys.readouterr()
    assert ptau.main(["info", f("pot_beacon.ptau")]) == 0
    out = capsys.readouterr().out
    assert "power 5, ceremony power 5, not prepared" in out and "contribution 1: contribution, name 'cli'" in out and "contribution 2: beacon 0102" in out
    assert ptau.main(["prepare", f("pot_beacon.ptau"), f("pot_final.ptau")]) == 0
    assert ptau.main(["contribute", f("pot_final.ptau"), f("x.ptau"), "--name", "late"]) == 1
    assert "already prepared" in capsys.readouterr().err
    final = open(f("pot_final.ptau"), "rb").read()
    assert sorted(ptau.read_ptau(final)["sections"]) == [1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15]
    assert len(ptau.read_contributions(final)) == 2
    json.dumps(ptau.apply_key_stats())
