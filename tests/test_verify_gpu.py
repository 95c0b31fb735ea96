"""`powersoftau verify` on the device (zkwg.ptau.verify -> zkwg_g2_subgroup_device / zkwg_point_rlc_device -> csrc/zkwg_kernels_verify.hip
and the multi-exponentiation plans; the pairings on the host, csrc/zkwg_pairing.h): the subgroup test against the host build and against
the DEFINITION [r] Q = infinity on the device, the sums against known logarithms, and power-9 files -- good ones pass in both states, each
single tamper fails its named check, the command line exits 0 / 1.  All comparisons are exact."""
import random

import pytest

import setuptest
import verifytest
from oracle.pyref import bn254_g2 as G2
from oracle.pyref import ntt as NTT

R = verifytest.R
mont2 = setuptest.mont2
N1, N2 = 4099, 2051                                               # not multiples of 64 / 32: several workgroups, a ragged last one


def _gpu_points(group, scalars):
    from zkwg import prover
    return bytes(prover.fixed_base(0, group, scalars).cpu().numpy())


@pytest.fixture(scope="module")
def points():
    """4,099 G1 and 2,051 G2 points of known logarithms, infinity at 0, 70 and the end"""
    rng = random.Random(1111)
    out = {}
    for group, n in ((1, N1), (2, N2)):
        logs = [rng.randrange(1, R) for _ in range(n)]
        logs[0] = logs[70] = logs[n - 1] = 0
        logs[1], logs[2] = 1, R - 1
        out[group] = (logs, _gpu_points(group, logs))
    return out


@pytest.fixture(scope="module")
def outside():
    """a raw twist point, its multiple of order 10069, and that added to a subgroup point"""
    raw = verifytest.twist_points(1, 1112)[0]
    small = verifytest.small_order_points(raw)[0]
    assert small is not None and verifytest.plain_mul(10069, small) is None
    return [mont2(raw), mont2(small), mont2(G2.add(G2.mul(12345, G2.G2), small))]


@pytest.mark.gpu
def test_gpu_subgroup_test_equals_the_host_build_and_the_definition(points, outside):
    from zkwg import phase2, ptau
    pts = points[2][1]
    assert pts[:128] == bytes(128) and pts[128 * 70:128 * 71] == bytes(128) and pts[-128:] == bytes(128)
    assert ptau.g2_subgroup(pts) == (0, None)
    planted = bytearray(pts)
    for at, p in zip((1, 70, N2 - 1), outside):
        planted[128 * at:128 * at + 128] = p
    planted = bytes(planted)
    assert ptau.g2_subgroup(planted) == (3, 1)
    assert ptau.g2_subgroup(planted[128 * 2:]) == (2, 68) and ptau.g2_subgroup(planted[128 * 71:]) == (1, N2 - 72)
    # the verdict of every one of the first 128 points is the host build's (the same per-point body)
    host = verifytest.g2_subgroup(planted[:128 * 128])
    assert host == [i not in (1, 70) for i in range(128)]
    assert [ptau.g2_subgroup(planted[128 * i:128 * i + 128])[0] == 0 for i in range(128)] == host
    # the definition on the device: [r] Q is infinity exactly for the points called inside
    by_r = phase2.scale_points(2, planted, R)
    zero = [by_r[128 * i:128 * i + 128] == bytes(128) for i in range(N2)]
    assert zero == [i not in (1, 70, N2 - 1) for i in range(N2)]
    # a point off the curve in the middle: the call is refused
    bad = bytearray(pts)
    bad[128 * 1000 + 70] ^= 1
    with pytest.raises(ptau.PtauError, match="curve"):
        ptau.g2_subgroup(bytes(bad))
    assert verifytest.violations() == 0


PIECE = 1 << 20                                   # ZK_VERIFY_PIECE (csrc/zkwg_verify_core.h): the points of one launch of the subgroup test


@pytest.mark.gpu
def test_gpu_subgroup_test_over_two_pieces_counts_and_places_across_them(outside):
    """piece + 1 points: the smallest call with a second piece, whose flags start afresh and whose index is offset by the piece"""
    from zkwg import ptau
    pts = bytearray(ptau.point_powers(2, ptau.generators()[1] * (PIECE + 1), 1, 1114))      # 1114^i G2: distinct points of the subgroup
    pts[128 * PIECE:] = outside[2]
    assert ptau.g2_subgroup(bytes(pts)) == (1, PIECE)
    pts[128 * 5:128 * 6] = outside[2]
    assert ptau.g2_subgroup(bytes(pts)) == (2, 5)


def _scalars(rng, n, bits=128):
    top = (1 << bits) - 1 if bits == 128 else R - 1
    s = [rng.randrange(top + 1) for _ in range(n)]
    s[0], s[1], s[2] = 0, 1, top
    s[n - 3], s[n - 2], s[n - 1] = top, 1, 0
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("group", [1, 2])
def test_gpu_ratio_sums_equal_the_known_logarithms(points, group):
    from zkwg import ptau
    rng = random.Random(1113 + group)
    pt = 64 if group == 1 else 128
    logs, pts = points[group]
    n = len(logs) - 1
    s = _scalars(rng, n)
    sb = b"".join(v.to_bytes(16, "little") for v in s)
    want_a = _gpu_points(group, [sum(v * a for v, a in zip(s, logs[:-1])) % R])
    want_b = _gpu_points(group, [sum(v * a for v, a in zip(s, logs[1:])) % R])
    assert any(want_a) and any(want_b) and want_a != want_b
    # the shifted form: both sums from one array, d_b = d_a + one point
    assert ptau.rlc(group, pts, sb, shifted=True) == (want_a, want_b)
    assert ptau.rlc(group, pts, sb, shifted=True, piece=1000) == (want_a, want_b)      # five / three pieces, the last one short
    # one sum (d_b = NULL), and full-width scalars through the same plans
    assert ptau.rlc(group, pts[:-pt], sb) == want_a == ptau.rlc(group, pts[:-pt], sb, piece=1000)
    w = _scalars(rng, n, bits=254)
    want_w = _gpu_points(group, [sum(v * a for v, a in zip(w, logs[:-1])) % R])
    assert ptau.rlc(group, pts[:-pt], b"".join(v.to_bytes(32, "little") for v in w), wide=True, piece=1500) == want_w
    assert ptau.rlc(group, pts[:pt], (5).to_bytes(16, "little")) == bytes(pt)                     # infinity only
    assert ptau.rlc(group, pts[pt:2 * pt], (0).to_bytes(16, "little")) == bytes(pt)               # a zero scalar only
    assert ptau.rlc(group, pts[:5 * pt], sb[:16 * 5]) == verifytest.rlc(group, pts[:5 * pt], sb[:16 * 5])
    # a bad point is refused, also when only the second array reaches it
    bad = bytearray(pts)
    bad[-pt + 3] ^= 1
    with pytest.raises(ptau.PtauError, match="curve"):
        ptau.rlc(group, bytes(bad), sb, shifted=True)
    assert ptau.rlc(group, bytes(bad)[:-pt], sb) == want_a
    bad = bytearray(pts)
    bad[pt * 1000 + 3] ^= 1
    with pytest.raises(ptau.PtauError, match="curve"):
        ptau.rlc(group, bytes(bad)[:-pt], sb, piece=300)


@pytest.mark.gpu
def test_gpu_inverse_transform_of_standard_form_scalars_is_the_oracles():
    from zkwg import ptau
    rng = random.Random(1116)
    B = ptau._backend(0)
    for q in (2, 5, 10):
        s = rng.randbytes(16 << q)
        got = bytes(B.ifft(s, q).cpu().numpy())
        want = NTT.ifft_fast([int.from_bytes(s[16 * j:16 * j + 16], "little") for j in range(1 << q)])
        assert got == b"".join(v.to_bytes(32, "little") for v in want), q
    for q in (0, 1, 2, 3):
        vals = [rng.randrange(1 << 128) for _ in range(1 << q)]
        assert ptau.ifft_host(vals, q) == NTT.ifft_fast(vals), q


# ---- files at power 9 ------------------------------------------------------------------------------------------------------------------------
POWER = 9


@pytest.fixture(scope="module")
def files():
    from zkwg import ptau
    seed = bytes(range(64))
    p0 = ptau.new(POWER)
    p1 = ptau.contribute(p0, "alice", "entropy", urandom=lambda n: seed[:n])
    p2 = ptau.beacon(p1, "the beacon", "0102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f20", 10)
    return {"new": p0, "two": p2, "prepared": ptau.prepare(p2), "cut": ptau.prepare(p2, POWER - 1)}


def _verify(data, seed=1117):
    from zkwg import ptau
    rng = random.Random(seed)
    res = ptau.verify(data, urandom=lambda n: rng.randbytes(n))
    return res, {name: ok for name, ok, _ in res["checks"]}


def _failed(checks):
    return {name for name, ok in checks.items() if ok is False}


@pytest.mark.gpu
@pytest.mark.parametrize("state", ["new", "two", "prepared", "cut"])
def test_gpu_good_files_pass(files, state):
    res, checks = _verify(files[state])
    assert res["ok"], res
    names = ["structure", "points", "subgroup", "anchors", "powers_2", "powers_3", "powers_4", "powers_5", "beta"]
    records = [] if state == "new" else ["record_1", "record_2", "last_record", "last_challenge"]
    lagrange = ["lagrange_12", "lagrange_13", "lagrange_14", "lagrange_15"] if state in ("prepared", "cut") else []
    assert list(checks) == names + records + lagrange
    assert all(ok for name, ok in checks.items() if name != "last_challenge")
    if state != "new":
        assert checks["last_challenge"] is (None if state == "cut" else True)


def _tampers():
    small = lambda: verifytest.small_order_points(verifytest.twist_points(1, 1112)[0])[0]

    def record(data):
        from zkwg import ptau
        recs = ptau.read_contributions(data)
        first = dict(recs[0])
        first["tau_g2_spx"] = mont2(G2.mul(5, G2.G2))
        return verifytest.with_records(data, [ptau.pack_record(first), recs[1]["raw"]])

    def challenge(data):
        from zkwg import ptau
        recs = ptau.read_contributions(data)
        last = dict(recs[1])
        last["next_challenge"] = bytes([last["next_challenge"][0] ^ 1]) + last["next_challenge"][1:]
        return verifytest.with_records(data, [recs[0]["raw"], ptau.pack_record(last)])

    def infinity(data):
        from zkwg import ptau
        o, size = ptau.read_any(data)[0]["sections"][4]
        return verifytest.reseal(data[:o] + bytes(size) + data[o + size:])
    swap = lambda sid: (lambda data: verifytest.reseal(verifytest.swap_points(data, sid, 200, 201)))
    # name -> (the file it starts from, the tamper, the checks that fail)
    return {
        "swap_2": ("two", swap(2), {"powers_2"}), "swap_3": ("two", swap(3), {"powers_3"}),
        "swap_4": ("two", swap(4), {"powers_4"}), "swap_5": ("two", swap(5), {"powers_5"}),
        "order_10069": ("two", lambda d: verifytest.reseal(verifytest.map_g2(d, 3, 300, lambda p: G2.add(p, small()))), {"subgroup"}),
        # (the record holds beta_g2 too, so `last_record` sees the same change: no single check can fail alone here)
        "beta_doubled": ("two", lambda d: verifytest.reseal(verifytest.map_g2(d, 6, 0, lambda p: G2.add(p, p))), {"beta", "last_record"}),
        "record": ("two", record, {"record_1"}), "challenge": ("two", challenge, {"last_challenge"}),
        "lagrange_12": ("prepared", lambda d: verifytest.swap_points(d, 12, 3, 4, first=(1 << 10) - 1), {"lagrange_12"}),      # the extra level
        "lagrange_13": ("prepared", lambda d: verifytest.swap_points(d, 13, 3, 4, first=(1 << 5) - 1), {"lagrange_13"}),
        "lagrange_15": ("prepared", lambda d: verifytest.swap_points(d, 15, 0, 1, first=1), {"lagrange_15"}),                  # level 1: host integers
        "infinity": ("two", infinity, {"points"}),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("tamper", list(_tampers()))
def test_gpu_each_tamper_fails_its_named_check(files, tamper):
    state, change, want = _tampers()[tamper]
    res, checks = _verify(change(files[state]))
    assert not res["ok"] and _failed(checks) == want, res
    if tamper == "order_10069":
        assert checks["powers_3"] is None and "the first at 300" in dict((n, d) for n, _, d in res["checks"])["subgroup"]
    if tamper == "infinity":
        assert list(checks)[-1] == "points"


@pytest.mark.gpu
def test_gpu_command_line_exits_0_on_a_good_file_and_1_on_a_tampered_one(files, tmp_path, capsys):
    from zkwg import ptau
    good, bad = tmp_path / "good.ptau", tmp_path / "bad.ptau"
    good.write_bytes(files["prepared"])
    bad.write_bytes(verifytest.swap_points(files["prepared"], 14, 3, 4, first=(1 << 6) - 1))
    assert ptau.main(["verify", str(good)]) == 0
    out = capsys.readouterr().out
    assert "lagrange_15: ok" in out and "record_2: ok" in out and "FAILED" not in out and "the file verifies" in out
    assert ptau.main(["verify", str(bad), "--device", "0"]) == 1
    out = capsys.readouterr().out
    assert "lagrange_14: FAILED" in out and out.count("FAILED") == 1 and "the file does NOT verify" in out
