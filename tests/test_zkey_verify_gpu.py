"""`zkey verify` on the device (zkwg.phase2.verify / verify_from_init -> zkwg_zkey_new, zkwg_point_rlc_device with TWO arrays,
zkwg_point_scale_device; the pairings on the host, csrc/zkwg_pairing.h): (a) the two-array form of the sums against known logarithms
(all 4,099 / 2,051 points: the independent reference) and against the host mirror (a 300-point prefix in pieces of 128, which holds
infinity in either array: the mirror's double-and-add is too slow for the whole arrays), (b) the seeded 5,200-constraint system of tests/test_phase2_gpu.py with one more wire that occurs in no constraint, on a
power-13 ceremony file made and prepared on the device, through  setup.new_zkey -> contribute -> beacon -> verify,  folded in pieces of
1,000 points, and (c) the tampers of tests/zkeyverifytest.py -- each fails its named check(s) and only those -- and the command line in a
process of its own.  All comparisons are exact."""
import os
import random
import subprocess
import sys

import pytest

import setuptest
import verifytest
import zkeyverifytest as zv
from conftest import ROOT

R = verifytest.R
N1, N2 = 4099, 2051                                               # not multiples of 64 / 32, nor of the piece: pieces end short
CHECKS = ["structure", "header", "section_3", "section_4", "section_5", "section_6", "section_7", "delta"]
TAIL = ["last_record", "section_8", "section_9"]
BEACON_HASH = "0102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f20"
UNUSED = 35


def _gpu_points(group, scalars):
    from zkwg import prover
    return bytes(prover.fixed_base(0, group, scalars).cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("group", [1, 2])
def test_gpu_two_array_sums_equal_the_known_logarithms_and_the_host_mirror(group):
    from zkwg import ptau
    rng = random.Random(1211 + group)
    n, pt = (N1, 64) if group == 1 else (N2, 128)
    logs_a, logs_b = ([rng.randrange(1, R) for _ in range(n)] for _ in range(2))
    for i in (0, 999, 1000, n - 1):
        logs_a[i] = logs_b[i] = 0                                 # infinity at the same index: the first point, both sides of a piece's end, the last
    logs_a[70] = logs_b[71] = logs_a[2000] = logs_b[1999] = 0     # and at different ones
    a, b = _gpu_points(group, logs_a), _gpu_points(group, logs_b)
    assert a[:pt] == b[:pt] == bytes(pt) and a != b
    s = [rng.randrange(1 << 128) for _ in range(n)]
    s[1], s[2], s[3], s[n - 2] = 0, 1, (1 << 128) - 1, (1 << 128) - 1
    sb = b"".join(v.to_bytes(16, "little") for v in s)
    want = tuple(_gpu_points(group, [sum(v * x for v, x in zip(s, logs)) % R]) for logs in (logs_a, logs_b))
    assert any(want[0]) and any(want[1]) and want[0] != want[1]
    assert ptau.rlc(group, a, sb, piece=1000, other=b) == want    # five / three pieces, the last one short
    assert ptau.rlc(group, a, sb, other=b) == want                # one piece
    assert ptau.rlc(group, b, sb, piece=1000, other=a) == want[::-1]
    assert ptau.rlc(group, a, sb, piece=1000, other=a) == (want[0], want[0])
    m = 300                                                       # the host mirror, on a prefix that holds infinity in either array
    assert ptau.rlc(group, a[:m * pt], sb[:16 * m], piece=128, other=b[:m * pt]) == zv.rlc2(group, a[:m * pt], b[:m * pt], sb[:16 * m])
    # the one-array forms are what they were
    assert ptau.rlc(group, a, sb, piece=1000) == want[0]
    # full-width scalars through the same call
    w = [rng.randrange(R) for _ in range(n)]
    want_w = tuple(_gpu_points(group, [sum(v * x for v, x in zip(w, logs)) % R]) for logs in (logs_a, logs_b))
    assert ptau.rlc(group, a, b"".join(v.to_bytes(32, "little") for v in w), wide=True, piece=1500, other=b) == want_w
    # a point off its curve in the SECOND array only is refused, in a later piece too
    for at in (5, n - 2):
        bad = bytearray(b)
        bad[pt * at + 3] ^= 1
        with pytest.raises(ptau.PtauError, match="curve"):
            ptau.rlc(group, a, sb, piece=1000, other=bytes(bad))
    for other in (b[:-pt], b + b[:pt]):
        with pytest.raises(ptau.PtauError, match="as many points"):
            ptau.rlc(group, a, sb, other=other)
    with pytest.raises(ptau.PtauError):
        ptau.rlc(group, a, sb[:-16], shifted=True, other=b)


@pytest.fixture(scope="module")
def chain():
    """the circuit, a power-13 ceremony file (new -> contribute -> prepare, on the device), the keys z0 -> contribute -> z1 -> beacon -> z2
    and the initial key of the system with one coefficient changed; the folds of every verification here go in pieces of 1,000 points"""
    from zkwg import phase2, ptau, r1cs as zr, setup
    n_public = 4
    heavy = {0: (4500, (0, 1, 2)), 3: (4300, (0,)), 4: (4200, (1,)), 5: (4100, (2,))}
    degrees = [(30, 1), (31, 2), (32, 63), (33, 64), (34, 65), (UNUSED, 0)]
    n_wires, cons, _ = setuptest.system(seed=21, n_in=40, n_public=n_public, n_cons=5200, heavy=heavy, degrees=degrees)
    assert setuptest.wire_degree(cons, UNUSED) == 0
    write = lambda c: zr.write_r1cs(n_wires, c, n_pub_out=2, n_pub_in=2, n_prv_in=35)
    r1cs = write(cons)
    assert setup.key_shape(r1cs)[0] == 13
    seed = bytes(range(64))
    pot = ptau.prepare(ptau.contribute(ptau.new(13), "alice", "entropy", urandom=lambda n: seed[:n]))
    z0 = setup.new_zkey(r1cs, pot)
    z1 = phase2.contribute(z0, "first", entropy="fixed entropy", urandom=lambda n: bytes(range(n)))
    z2 = phase2.beacon(z1, "the beacon", BEACON_HASH, 10)
    changed = list(cons)
    row = tuple(dict(m) for m in cons[3000])
    wire = min(row[1])
    row[1][wire] = (row[1][wire] + 1) % R or 2
    changed[3000] = row
    mp = pytest.MonkeyPatch()
    mp.setattr(phase2, "FOLD_PIECE", 1000)
    yield {"r1cs": r1cs, "pot": pot, "z": (z0, z1, z2), "changed": setup.new_zkey(write(changed), pot), "n_wires": n_wires, "n_public": n_public}
    mp.undo()


def _verify(chain, key, seed=1215, init=None):
    from zkwg import phase2
    rng = random.Random(seed)
    return phase2.verify_from_init(chain["z"][0] if init is None else init, key, urandom=lambda n: rng.randbytes(n))


@pytest.mark.gpu
def test_gpu_the_keys_of_the_chain_pass_every_check_by_rebuild_and_from_the_initial_key(chain):
    from zkwg import phase2
    z0, z1, z2 = chain["z"]
    assert phase2.FOLD_PIECE == 1000 and zv.count(z2, 8) == chain["n_wires"] - chain["n_public"] - 1 > 5000 and zv.count(z2, 9) == 8192
    assert zv.infinity_at(z2, 8) == zv.infinity_at(z0, 8) == [UNUSED - chain["n_public"] - 1]
    for k, z in enumerate((z0, z1, z2)):
        rng = random.Random(1216 + k)
        res = phase2.verify(chain["r1cs"], chain["pot"], z, urandom=lambda n: rng.randbytes(n))
        assert res["ok"] and all(ok is True for _, ok, _ in res["checks"]), res
        assert [name for name, _, _ in res["checks"]] == CHECKS + [f"record_{i + 1}" for i in range(k)] + TAIL
        assert _verify(chain, z, seed=1216 + k) == res             # verify_from_init: the same verdict, check by check
    detail = dict((n, d) for n, _, d in res["checks"])
    assert "beacon 'the beacon'" in detail["record_2"] and detail["section_9"] == "8192 points"
    assert _verify(chain, z2, init=z1)["ok"]                      # one contribution at a time


@pytest.mark.gpu
@pytest.mark.parametrize("tamper", list(zv.tampers()))
def test_gpu_each_tamper_fails_its_named_checks_and_only_those(chain, tamper):
    change, want = zv.tampers()[tamper]
    res = _verify(chain, change(chain["z"][2]))
    assert not res["ok"] and zv.failed(res) == want, res
    assert [name for name, _, _ in res["checks"]] == CHECKS + ["record_1", "record_2"] + TAIL


@pytest.mark.gpu
def test_gpu_a_changed_system_an_off_curve_point_and_broken_containers(chain):
    from zkwg import phase2
    z2 = chain["z"][2]
    res = phase2.verify(chain["r1cs"], chain["pot"], chain["changed"])
    got = zv.failed(res)
    assert not res["ok"] and "section_4" in got and got & {"section_5", "section_6", "section_7"} and "structure" not in got, res
    for sid, i in ((8, 4321), (9, 8191)):                          # in a later piece, and the last point
        p = bytearray(zv.point(z2, sid, i))
        p[40] ^= 2
        res = _verify(chain, zv.set_point(z2, sid, i, bytes(p)))
        assert zv.failed(res) == {f"section_{sid}"} and "curve" in dict((n, d) for n, _, d in res["checks"])[f"section_{sid}"]
    for bad in zv.broken_containers(z2):
        res = _verify(chain, bad)
        assert not res["ok"] and [c[:2] for c in res["checks"]] == [("structure", False)]


@pytest.mark.gpu
def test_gpu_command_line_in_a_process_of_its_own(chain, tmp_path):
    z0, _, z2 = chain["z"]
    f = lambda name: str(tmp_path / name)
    for name, data in (("c.r1cs", chain["r1cs"]), ("pot.ptau", chain["pot"]), ("c_0000.zkey", z0), ("c_final.zkey", z2),
                       ("bad.zkey", zv.tampers()["swap_8"][0](z2))):
        open(f(name), "wb").write(data)
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "zk-email-verify_amd", "py"))
    run = lambda *argv: subprocess.run([sys.executable, "-m", "zkwg.phase2", "verify"] + list(argv), env=env, capture_output=True, text=True, timeout=300)
    r = run(f("c.r1cs"), f("pot.ptau"), f("c_final.zkey"))
    assert r.returncode == 0 and "section_8: ok" in r.stdout and "record_2: ok" in r.stdout and "FAILED" not in r.stdout and "the key verifies" in r.stdout, r.stdout + r.stderr
    r = run(f("bad.zkey"), "--init", f("c_0000.zkey"), "--device", "0")
    assert r.returncode == 1 and "section_8: FAILED" in r.stdout and r.stdout.count("FAILED") == 1 and "the key does NOT verify" in r.stdout, r.stdout + r.stderr
