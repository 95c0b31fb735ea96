"""The powers-of-tau preparation on the CPU: the host build of csrc/zkwg_ptau_core.h (tests/native/ptautest.cpp) runs the launch series
of zkwg_group_ntt_device / zkwg_ptau_prepare over the per-point functions the kernels compile, with every limb-form bound counted.
Inputs have known logarithms, so every expected point is the fixed-base multiple (tests/setuptest.host_points: canonical-word arithmetic,
none of the code under test) of a scalar transform computed in Python integers (oracle/pyref/ntt).  All comparisons are exact."""
import random
import struct

import pytest

import ptautest
import setuptest
from oracle.pyref import groth16 as G
from oracle.pyref import ntt

R = ptautest.R
PT = {1: 64, 2: 128}
TAU, ALPHA, BETA = (random.Random(77).randrange(2, R) for _ in range(3))


@pytest.fixture(scope="module")
def toy():
    """an unprepared power-5 file from the seeded trapdoor, its logarithms, and its preparation by the host mirror"""
    from zkwg import ptau
    pot = ptautest.toy_ceremony(5, TAU, ALPHA, BETA, setuptest.host_points, ceremony_power=7, contributions=b"the contributions")
    rc, msg, out = ptautest.prepare(pot)
    assert rc == 0, msg
    return {"pot": pot, "out": out, "scalars": ptautest.ceremony_scalars(5, TAU, ALPHA, BETA), "info": ptau.read_ptau(out)}


def _cases(L, rng):
    n = 1 << L
    w = ntt.root(L)
    some = [rng.randrange(R) for _ in range(n)]
    for k in rng.sample(range(n), min(n, 3)):
        some[k] = 0
    tau = rng.randrange(2, R)
    return {"random tau": [pow(tau, k, R) for k in range(n)], "tau = 1": [1] * n, "tau a root of unity": [pow(w, k, R) for k in range(n)],
            "infinity among the inputs": some, "all at infinity": [0] * n}


@pytest.mark.parametrize("group,top", [(1, 7), (2, 5)])
def test_host_transform_equals_the_scalar_transform_of_the_logarithms(group, top):
    rng = random.Random(100 + group)
    for L in range(top + 1):
        for name, logs in _cases(L, rng).items():
            pts = setuptest.host_points(group, logs)
            inv = ptautest.ntt(group, pts, True)
            assert inv == setuptest.host_points(group, ntt.ifft_fast(logs)), (L, name)
            fwd = ptautest.ntt(group, pts, False)
            assert fwd == setuptest.host_points(group, ntt.fft_fast(logs)), (L, name)
            assert ptautest.ntt(group, inv, False) == pts and ptautest.ntt(group, fwd, True) == pts, (L, name)       # forward o inverse = identity
        n = 1 << L
        ones = setuptest.host_points(group, [1] * n)
        assert ptautest.ntt(group, ones, True) == ones[:PT[group]] + bytes(PT[group] * (n - 1))                 # tau = 1: the rest is infinity
    assert ptautest.violations() == 0


def test_inverse_transform_of_the_powers_is_the_lagrange_basis_at_tau():
    """level q <= power of a prepared file is what groth16.lagrange_at gives; the padded level is NOT"""
    for q in range(6):
        assert ntt.ifft_fast([pow(TAU, k, R) for k in range(1 << q)]) == G.lagrange_at(TAU, q)
    n2 = 64
    padded = ntt.ifft_fast([pow(TAU, k, R) for k in range(n2 - 1)] + [0])
    full = G.lagrange_at(TAU, 6)
    w, top = ntt.root(6), pow(TAU, n2 - 1, R) * pow(n2, -1, R) % R
    assert padded != full and padded == [(full[j] - top * pow(w, j, R)) % R for j in range(n2)]


def test_host_prepare_of_a_power_5_file_equals_the_scalar_transforms_in_every_byte(toy):
    from zkwg import ptau
    out, info = toy["out"], toy["info"]
    assert (info["power"], info["ceremony_power"]) == (5, 7) and sorted(info["sections"]) == [1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15]
    assert struct.unpack_from("<II", out, 4) == (1, 11)
    want = ptautest.lagrange_scalars(5, toy["scalars"])
    for sid, group in ((12, 1), (13, 2), (14, 1), (15, 1)):
        o, size = info["sections"][sid]
        assert len(want[sid]) * PT[group] == size
        assert out[o:o + size] == setuptest.host_points(group, want[sid]), sid
    assert want[12][63:] != G.lagrange_at(TAU, 6) and want[12][31:63] == G.lagrange_at(TAU, 5)
    src = ptau.read_ptau(toy["pot"], prepared=False)
    for sid in range(1, 8):                                                     # sections 1 - 7 are unchanged
        (o, n), (o2, n2) = info["sections"][sid], src["sections"][sid]
        assert out[o:o + n] == toy["pot"][o2:o2 + n2], sid
    o7 = info["sections"][7]
    assert out[o7[0]:o7[0] + o7[1]] == b"the contributions"
    assert ptautest.violations() == 0
    # what the set-up reads from it: the walker accepts the file
    rc, msg, offs, pts = setuptest.host_ptau_parse(out, 5)
    assert rc == 0, msg
    assert offs[0] == info["sections"][12][0] + 31 * 64 and offs[4] == info["sections"][12][0] + 63 * 64


def test_prepare_at_a_smaller_power_equals_prepare_of_the_truncated_file(toy):
    from zkwg import ptau
    cut = ptau.truncate(toy["pot"], 3)
    ci = ptau.read_ptau(cut, prepared=False)
    assert (ci["power"], ci["ceremony_power"]) == (3, 7)
    assert [ci["sections"][s][1] for s in (2, 3, 4, 5, 6)] == [15 * 64, 8 * 128, 8 * 64, 8 * 64, 128]
    rc, msg, a = ptautest.prepare(toy["pot"], 3)
    assert rc == 0, msg
    rc, msg, b = ptautest.prepare(cut)
    assert rc == 0, msg
    assert a == b                                                               # byte for byte
    # its levels <= 3 are the corresponding levels of the full preparation; its padded level 4 is not level 4 of the full one
    ia = ptau.read_ptau(a)
    for sid in (12, 13, 14, 15):
        for q in range(4):
            assert bytes(ptau.level(a, ia, sid, q)) == bytes(ptau.level(toy["out"], toy["info"], sid, q)), (sid, q)
    assert bytes(ptau.level(a, ia, 12, 4)) != bytes(ptau.level(toy["out"], toy["info"], 12, 4))
    s = toy["scalars"][2]
    assert bytes(ptau.level(a, ia, 12, 4)) == setuptest.host_points(1, ntt.ifft_fast(s[:15] + [0]))
    rc, msg, same = ptautest.prepare(toy["pot"], 5)
    assert rc == 0 and same == toy["out"]


def test_refusals(toy):
    from zkwg import ptau
    pot, out = toy["pot"], toy["out"]
    src = ptau.read_ptau(pot, prepared=False)
    rc, msg, _ = ptautest.prepare(out)
    assert rc == -1 and "already prepared" in msg
    # one Lagrange section is enough
    o12 = toy["info"]["sections"][12]
    half = bytearray(out[:o12[0] + o12[1]])
    struct.pack_into("<I", half, 8, 8)
    rc, msg, _ = ptautest.prepare(bytes(half))
    assert rc == -1 and "already prepared" in msg
    rc, msg, _ = ptautest.prepare(pot, 6)
    assert rc == -1 and "above the file's" in msg
    rc, msg, _ = ptautest.prepare(pot[:-40])
    assert rc == -1 and "runs past the end" in msg
    short = bytearray(pot)                                                      # section 3 one point short
    o3 = src["sections"][3][0]
    struct.pack_into("<Q", short, o3 - 8, 31 * 128)
    del short[o3 + 31 * 128:o3 + 32 * 128]
    rc, msg, _ = ptautest.prepare(bytes(short))
    assert rc == -1 and "missing or of the wrong size" in msg
    for sid, at in ((2, 62 * 64 + 40), (2, 3), (3, 31 * 128 + 100), (4, 5), (5, 31 * 64 + 33)):          # a point off the curve: first, last, every section
        bad = bytearray(pot)
        bad[src["sections"][sid][0] + at] ^= 1
        rc, msg, _ = ptautest.prepare(bytes(bad))
        assert rc == -1 and "curve" in msg, (sid, at)
    for sid, at in ((2, 7 * 64), (3, 128 + 96)):                               # a word >= q: x + q (still below 2^256), on the curve modulo q
        bad = bytearray(pot)
        o = src["sections"][sid][0] + at
        v = int.from_bytes(bad[o:o + 32], "little") + setuptest.Q
        assert v < 1 << 256
        bad[o:o + 32] = v.to_bytes(32, "little")
        rc, msg, _ = ptautest.prepare(bytes(bad))
        assert rc == -1 and "curve" in msg and "not reduced" in msg, sid
    # a bad point beyond the prefix a smaller power reads is not looked at
    bad = bytearray(pot)
    bad[src["sections"][2][0] + 62 * 64 + 40] ^= 1
    rc, msg, cut = ptautest.prepare(bytes(bad), 3)
    assert rc == 0 and cut == ptautest.prepare(pot, 3)[2]
    # the transform alone
    pts = bytearray(setuptest.host_points(1, [3, 4, 5, 6]))
    pts[64 * 3 + 2] ^= 1
    assert ptautest.ntt(1, bytes(pts), True) is None


def test_the_walkers_refusals_keep_their_messages(toy):
    from zkwg import ptau
    pot, out = toy["pot"], toy["out"]
    rc, msg, _, _ = setuptest.host_ptau_parse(pot, 5)
    assert rc == -1 and msg == "Powers of tau is not prepared"
    with pytest.raises(ValueError, match="Powers of tau is not prepared"):
        ptau.read_ptau(pot)
    with pytest.raises(ValueError, match="already prepared"):
        ptau.read_ptau(out, prepared=False)
    rc, msg, _, _ = setuptest.host_ptau_parse(out, 6)
    assert rc == -1 and msg == ".ptau: the power of the file is too small for the circuit"
    rc, msg, _, _ = setuptest.host_ptau_parse(b"ptaX" + out[4:], 5)
    assert rc == -1 and msg == "not a .ptau file (magic)"
    rc, msg, _ = ptautest.prepare(b"ptaX" + pot[4:])
    assert rc == -1 and msg == "not a .ptau file (magic)"
    o15 = toy["info"]["sections"][15]
    short = bytearray(out[:-64])
    struct.pack_into("<Q", short, o15[0] - 8, o15[1] - 64)
    rc, msg, _, _ = setuptest.host_ptau_parse(bytes(short), 5)
    assert rc == -1 and msg == ".ptau: a Lagrange section (12 - 15) is of the wrong size"
    with pytest.raises(ValueError, match="section 15 holds"):
        ptau.read_ptau(bytes(short))
    with pytest.raises(ptau.PtauError, match="cannot cut"):
        ptau.truncate(pot, 6)


def test_recoding_of_every_twiddle_of_2_to_the_10():
    for inverse in (False, True):
        w = ntt.root(10)
        w = pow(w, R - 2, R) if inverse else w
        digits = ptautest.twiddle_digits(10, inverse)
        assert len(digits) == 512
        acc = 1
        for e, d in enumerate(digits):
            assert sum(x << i for i, x in enumerate(d)) == acc, e                # the sum reproduces w^e
            assert all(not (d[i] and d[i + 1]) for i in range(254)), e           # no two neighbours non-zero
            acc = acc * w % R
    assert ptautest.twiddle_digits(0, False) == [[1] + [0] * 254]
