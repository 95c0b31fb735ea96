"""`zkey verify` on the CPU: zkwg.phase2.verify / verify_from_init with every device call replaced by the host mirror that exists
(tests/zkeyverifytest.py: the set-up, the scalings, the file operation and the sums; the pairing is the product's host code).  A toy
system of 12 constraints -- power 4 holds 16 rows, three of them the public ones -- with one private wire that occurs in no constraint, so
that section 8 holds a point at infinity; a toy ceremony of a known trapdoor, prepared on the host.  The initial key, the key after a
contribution and the key after contribution + beacon pass every check; each single tamper fails its named check(s) and only those."""
import random

import pytest

import ptautest
import setuptest
import zkeyverifytest as zv

R = setuptest.R
N_PUBLIC, N_IN, N_CONS, UNUSED = 2, 8, 12, 7
CHECKS = ["structure", "header", "section_3", "section_4", "section_5", "section_6", "section_7", "delta"]
TAIL = ["last_record", "section_8", "section_9"]
BEACON_HASH = "0102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f20"


def _r1cs(cons, n_wires, n_in=N_IN):
    from zkwg import r1cs as zr
    return zr.write_r1cs(n_wires, cons, n_pub_out=1, n_pub_in=1, n_prv_in=n_in - 1 - N_PUBLIC)


@pytest.fixture(scope="module")
def files():
    """the circuit, the prepared ceremony file, the keys z0 -> contribute -> z1 -> beacon -> z2, and the initial key of the system with one
    coefficient changed -- all on the host mirrors, which stay in place for the module's verifications"""
    from zkwg import phase2, setup
    mp = pytest.MonkeyPatch()
    zv.host_mirrors(mp)
    n_wires, cons, _ = setuptest.system(seed=1201, n_in=N_IN, n_public=N_PUBLIC, n_cons=N_CONS, degrees=[(UNUSED, 0)])
    assert setuptest.wire_degree(cons, UNUSED) == 0 and all(setuptest.wire_degree(cons, w) for w in range(1, n_wires) if w != UNUSED)
    rc, msg, pot = ptautest.prepare(ptautest.toy_ceremony(4, 0x1234567, 0x89abcde, 0xf012345, setuptest.host_points))
    assert rc == 0, msg
    r1cs = _r1cs(cons, n_wires)
    assert setup.key_shape(r1cs)[0] == 4
    z0 = setup.new_zkey(r1cs, pot)
    z1 = phase2.contribute(z0, "first", entropy="e", urandom=lambda n: bytes(range(n)))
    z2 = phase2.beacon(z1, "the beacon", BEACON_HASH, 10)
    changed = [tuple(dict(m) for m in row) for row in cons]
    wire = min(changed[3][0])
    changed[3][0][wire] = (changed[3][0][wire] + 1) % R or 2
    yield {"r1cs": r1cs, "pot": pot, "z": (z0, z1, z2), "changed": setup.new_zkey(_r1cs(changed, n_wires), pot), "n_wires": n_wires}
    mp.undo()


def _from_init(files, key, seed=1202, init=None):
    from zkwg import phase2
    rng = random.Random(seed)
    res = phase2.verify_from_init(files["z"][0] if init is None else init, key, urandom=lambda n: rng.randbytes(n))
    assert res["ok"] == all(ok is not False for _, ok, _ in res["checks"])
    return res


def test_the_two_array_mirror_is_two_sums_under_the_same_scalars():
    rng = random.Random(1203)
    logs_a, logs_b = ([rng.randrange(R) for _ in range(9)] for _ in range(2))
    logs_a[2] = logs_b[2] = logs_a[5] = logs_b[7] = 0                       # infinity at the same index and at different ones
    s = [rng.randrange(1 << 128) for _ in range(9)]
    sb = b"".join(v.to_bytes(16, "little") for v in s)
    for group in (1, 2):
        a, b = setuptest.host_points(group, logs_a), setuptest.host_points(group, logs_b)
        want = tuple(setuptest.host_points(group, [sum(x * y for x, y in zip(s, logs)) % R]) for logs in (logs_a, logs_b))
        assert zv.rlc2(group, a, b, sb) == want
        assert zv.HostBackend().rlc(group, a, 1, 8, sb[16:], other=b) == \
            tuple(setuptest.host_points(group, [sum(x * y for x, y in zip(s[1:], logs[1:])) % R]) for logs in (logs_a, logs_b))
        bad = bytearray(b)
        bad[len(b) - 9] ^= 1
        assert zv.rlc2(group, a, bytes(bad), sb) is None


def test_the_rebuilt_initial_key_is_the_set_up_and_holds_the_unused_wire_as_infinity(files):
    z0 = files["z"][0]
    assert zv.infinity_at(z0, 8) == [UNUSED - N_PUBLIC - 1]
    assert zv.count(z0, 8) == files["n_wires"] - N_PUBLIC - 1 and zv.count(z0, 9) == 16


def test_good_keys_pass_every_check(files):
    from zkwg import phase2
    z0, z1, z2 = files["z"]
    before = (zv.verifytest.violations(), zv.phase2test.violations())
    for k, z in enumerate((z0, z1, z2)):
        rng = random.Random(1204 + k)
        res = phase2.verify(files["r1cs"], files["pot"], z, urandom=lambda n: rng.randbytes(n))
        names = [name for name, _, _ in res["checks"]]
        assert res["ok"] and names == CHECKS + [f"record_{i + 1}" for i in range(k)] + TAIL and all(ok is True for _, ok, _ in res["checks"]), res
        assert res == {"ok": True, "checks": _from_init(files, z, seed=1204 + k)["checks"]}
    detail = dict((n, d) for n, _, d in _from_init(files, z2)["checks"])
    assert "contribution 'first'" in detail["record_1"] and "beacon 'the beacon'" in detail["record_2"] and "2 contributions" in detail["structure"]
    assert "no contribution" in dict((n, d) for n, _, d in _from_init(files, z0)["checks"])["last_record"]
    assert (zv.verifytest.violations(), zv.phase2test.violations()) == before == (0, 0)
    # one contribution at a time: the key before it as the initial key, whose records the key must repeat
    res = _from_init(files, z2, init=z1)
    assert res["ok"] and "as in the initial key" in res["checks"][8][2] and "beacon" in res["checks"][9][2]
    assert zv.failed(_from_init(files, z1, init=z2)) >= {"last_record"}


@pytest.mark.parametrize("tamper", list(zv.tampers()))
def test_each_tamper_fails_its_named_checks_and_only_those(files, tamper):
    change, want = zv.tampers()[tamper]
    res = _from_init(files, change(files["z"][2]))
    assert not res["ok"] and zv.failed(res) == want, res
    assert [name for name, _, _ in res["checks"]] == CHECKS + ["record_1", "record_2"] + TAIL
    detail = dict((n, d) for n, _, d in res["checks"])
    if tamper == "swap_5":
        i = zv.two_distinct(files["z"][2], 5)[0]
        assert detail["section_5"] == f"point {i} differs"
    if tamper == "coefficient_byte_4":
        assert detail["section_4"].startswith("coefficient 5 differs")
    if tamper == "last_g1_sx":
        assert "transcript" in detail["record_2"] and "proof of knowledge" in detail["record_2"] and "link" not in detail["record_2"]
    if tamper == "beacon_exponent":
        assert detail["record_2"].endswith("delta_after is not the beacon's scalar times the delta1 before")


def test_a_changed_record_in_the_middle_also_breaks_the_transcripts_after_it(files):
    from zkwg import phase2
    z2 = files["z"][2]
    recs = [dict(r) for r in phase2.read_contributions(z2)[1]]
    recs[0]["g1_sx"] = phase2.scale_points(1, recs[0]["g1_sx"], 2)
    res = _from_init(files, zv.with_records(z2, recs))
    assert zv.failed(res) == {"record_1", "record_2"}
    assert dict((n, d) for n, _, d in res["checks"])["record_2"].endswith(": transcript")


def test_the_key_of_a_changed_system_fails_against_the_original_circuit(files):
    from zkwg import phase2
    rng = random.Random(1205)
    res = phase2.verify(files["r1cs"], files["pot"], files["changed"], urandom=lambda n: rng.randbytes(n))
    got = zv.failed(res)
    assert not res["ok"] and "section_4" in got and got & {"section_5", "section_6", "section_7"} and "structure" not in got, res
    # and against its own circuit it is a good initial key
    assert _from_init(files, files["changed"], init=files["changed"])["ok"]


def test_a_delta2_the_pairing_refuses_fails_delta_and_does_not_raise(files):
    z2 = files["z"][2]
    d2 = bytearray(zv.header_point(z2, "delta2"))
    d2[5] ^= 1                                                             # off the curve
    small = zv.verifytest.small_order_points(zv.verifytest.twist_points(1, 1206)[0])[0]
    for p, word in ((bytes(d2), "curve"), (setuptest.mont2(small), "subgroup")):
        res = _from_init(files, zv.set_header_point(z2, "delta2", p))
        assert zv.failed(res) == {"delta", "section_8", "section_9"}, res
        assert word in dict((n, d) for n, _, d in res["checks"])["delta"]
    res = _from_init(files, zv.set_header_point(z2, "delta1", bytes(64)))
    assert zv.failed(res) == {"delta", "last_record"} and "infinity" in dict((n, d) for n, _, d in res["checks"])["delta"]


def test_a_changed_header_point_or_circuit_hash_fails_the_header_check_alone(files):
    from zkwg import phase2
    z2 = files["z"][2]
    res = _from_init(files, zv.set_header_point(z2, "gamma2", zv.header_point(z2, "beta2")))
    assert zv.failed(res) == {"header"} and "gamma2 differs" in dict((n, d) for n, _, d in res["checks"])["header"]
    # another circuit hash: the records were made over the old one, so their transcripts no longer hold either
    o = zv._sec(z2)[10][0]
    res = _from_init(files, z2[:o] + b"\x01" + z2[o + 1:])
    assert zv.failed(res) == {"header", "record_1", "record_2"}


def test_an_off_curve_point_of_section_8_or_9_is_the_mirrors_refusal_and_fails_that_section(files):
    z2 = files["z"][2]
    for sid in (8, 9):
        p = bytearray(zv.point(z2, sid, 3))
        p[40] ^= 2
        res = _from_init(files, zv.set_point(z2, sid, 3, bytes(p)))
        assert zv.failed(res) == {f"section_{sid}"} and "curve" in dict((n, d) for n, _, d in res["checks"])[f"section_{sid}"]


def test_a_broken_container_fails_the_structure_check_which_ends_the_run(files):
    z0, _, z2 = files["z"]
    for bad in zv.broken_containers(z2) + [b"zkez" + z2[4:], z2[:200]]:
        res = _from_init(files, bad)
        assert not res["ok"] and [name for name, _, _ in res["checks"]] == ["structure"] and res["checks"][0][1] is False
    res = _from_init(files, z2, init=z0[:-5])
    assert [c[:2] for c in res["checks"]] == [("structure", False)] and "the initial key" in res["checks"][0][2]
    # a key of another shape: the contributed key of a larger system against this circuit
    from zkwg import phase2, setup
    n_wires, cons, _ = setuptest.system(seed=1207, n_in=N_IN + 1, n_public=N_PUBLIC, n_cons=N_CONS)
    other = setup.new_zkey(_r1cs(cons, n_wires, N_IN + 1), files["pot"])
    res = _from_init(files, other)
    assert [c[:2] for c in res["checks"]] == [("structure", False)] and "nVars" in res["checks"][0][2]


def test_the_command_line_prints_a_line_per_check_and_exits_0_or_1(files, tmp_path, capsys):
    from zkwg import phase2
    z0, _, z2 = files["z"]
    f = lambda name: str(tmp_path / name)
    for name, data in (("c.r1cs", files["r1cs"]), ("pot.ptau", files["pot"]), ("c_0000.zkey", z0), ("c_final.zkey", z2),
                       ("bad.zkey", zv.tampers()["swap_9"][0](z2)), ("cut.zkey", z2[:-9])):
        open(f(name), "wb").write(data)
    assert phase2.main(["verify", f("c.r1cs"), f("pot.ptau"), f("c_final.zkey")]) == 0
    out = capsys.readouterr().out
    assert "record_2: ok" in out and "section_9: ok" in out and "FAILED" not in out and "the key verifies" in out
    assert len(out.splitlines()) == len(CHECKS) + 2 + len(TAIL) + 1
    assert phase2.main(["verify", f("c_final.zkey"), "--init", f("c_0000.zkey"), "--device", "0"]) == 0
    assert capsys.readouterr().out == out
    assert phase2.main(["verify", f("c.r1cs"), f("pot.ptau"), f("bad.zkey")]) == 1
    out = capsys.readouterr().out
    assert "section_9: FAILED" in out and out.count("FAILED") == 1 and "the key does NOT verify" in out
    assert phase2.main(["verify", f("bad.zkey"), "--init", f("c_0000.zkey")]) == 1
    assert phase2.main(["verify", f("cut.zkey"), "--init", f("c_0000.zkey")]) == 1
    assert capsys.readouterr().out.splitlines()[-2].startswith("structure: FAILED")
    # unreadable arguments: what the set-up refuses is reported as the other subcommands report it, exit code 1
    assert phase2.main(["verify", f("pot.ptau"), f("pot.ptau"), f("c_final.zkey")]) == 1
    assert phase2.main(["verify", f("c.r1cs"), f("c_final.zkey"), f("c_final.zkey")]) == 1
    # a file that is missing, and one that is empty
    open(f("empty.zkey"), "wb").close()
    assert phase2.main(["verify", f("c.r1cs"), f("pot.ptau"), f("nowhere.zkey")]) == 1
    assert phase2.main(["verify", f("nowhere.r1cs"), f("pot.ptau"), f("c_final.zkey")]) == 1
    assert phase2.main(["verify", f("empty.zkey"), "--init", f("c_0000.zkey")]) == 1
    assert phase2.main(["verify", f("c_final.zkey"), "--init", f("empty.zkey")]) == 1
    captured = capsys.readouterr()
    assert captured.err.count("no verdict: ") == 6 and captured.out == ""
    for argv in (["verify", f("c.r1cs"), f("pot.ptau")], ["verify", f("c.r1cs"), f("pot.ptau"), f("c_final.zkey"), "--init", f("c_0000.zkey")]):
        with pytest.raises(SystemExit) as e:
            phase2.main(argv)
        assert e.value.code == 2
