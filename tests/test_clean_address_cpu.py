"""The CleanEmailAddress main without a GPU (utils/email.circom:16-140; ZKWG_MAIN_CLEAN_EMAIL_ADDRESS).

The fixtures (tests/golden/clean_address, written by tests/golden/make_clean_address_fixtures.py) hold what the circom interpreter
computes from the reference's own template: the seven answers of clean-email-address.test.ts at 32 and 72, the project's edge cases at
every shape, a seeded batch of 130 at 24.  Checked here: the C++ walker's names and order, the prepare core on the host
(zkwg_cea_core.h) with the host expansion (zkwg_expand_host: the decoders zk_expand3_cea runs), the emitted constraint system, the
configuration bounds, the input helpers, and the core under the address / undefined-behaviour sanitizers as a stand-alone program."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import ceatest as ct
import r1cs_util
import zkwg
from conftest import ROOT
from zkwg import inputs as zi
from zkwg import r1cs as zr

P = ct.P
# clean-email-address.test.ts: encoded, decoded, isValid
REFERENCE = (("shreyas.londhe+alias@gmail.com", "shreyaslondhe@gmail.com", 1), ("shreyas.londhe+alias@gmail.com", "shreyaslondhe@yahoo.com", 0),
             ("shreyas.londhe@gmail.com", "shreyaslondhe@gmail.com", 1), ("shreyaslondhe+test@gmail.com", "shreyaslondhe@gmail.com", 1),
             ("shreyas.londhe.test@gmail.com", "shreyaslondhetest@gmail.com", 1), ("shs.loe+test.alias+123@gmail.com", "shsloe@gmail.com", 1),
             ("shreyaslondhe@gmail.com", "shreyaslondhe@gmail.com", 1))


def _circuit(L, device=-1):
    return zkwg.Circuit(device=device, **ct.circuit_kwargs(L))


_host = {}


def _host_witnesses(L):
    """(witness bytes of every case, statuses, bytes per witness, slot names) from the host core + zkwg_expand_host, once per shape"""
    if L not in _host:
        c = _circuit(L)
        wit, status = ct.host_witnesses(c, [inp for _, inp in ct.load_fixture(L)["cases"]])
        _host[L] = (wit, status, c.witness_bytes, [n for _, n in c.symbols()])
    return _host[L]


def _ints(w):
    return [int.from_bytes(w[i:i + 32], "little") for i in range(0, len(w), 32)]


@pytest.mark.parametrize("L", ct.SHAPES)
def test_walker_symbols_follow_the_interpreters_order(L):
    c = _circuit(L)
    fx = ct.load_fixture(L)
    sym = c.symbols()
    assert len(sym) == c.W == fx["W"] and [s for s, _ in sym] == list(range(c.W))
    assert ct.sym_hash(sym) == fx["sym_sha256"]
    assert [n for _, n in sym[:4]] == ["one", "main.isValid", "main.encoded[0]", "main.encoded[1]"] and sym[2 + L][1] == "main.decoded[0]"
    o0 = fx["o0_index"]
    assert len(o0) == c.W and o0[0] == 0 and bool(np.all(np.diff(o0.astype(np.int64)) > 0))
    nch = L // 8
    # one, isValid, the inputs; 4 arrays of L and 3 of L - 1 decoded from bytes; rDec, sumEnc, sumDec; rHasher; 3 L + 1 IsZero pairs; muxEnc
    assert c.W == 2 + 2 * L + (4 * L + 3 * (L - 1)) + (3 * L - 1) + (612 * nch + 243 * (nch - 1)) + 2 * (3 * L + 1) + (2 * L - 1)
    assert c.n_public == 1
    if L == 32:
        assert c.W == 3816      # the kept slot count of CleanEmailAddress(32)


def test_fixtures_are_what_the_interpreter_computes_today():
    from oracle.circom import ev
    if not ev.reference_available():
        pytest.skip("the reference tree is not present")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_clean_address_fixtures as mk
    assert mk.main(["--check"]) == 0


@pytest.mark.parametrize("L", ct.SHAPES)
def test_host_core_and_host_expansion_equal_every_fixture_slot(L):
    fx = ct.load_fixture(L)
    wit, status, wb, names = _host_witnesses(L)
    assert status == [0] * len(fx["cases"])          # the template asserts nothing
    for i in range(len(fx["cases"])):
        assert ct.mismatch(fx, i, wit[i * wb:(i + 1) * wb], names) is None
    # the comparison itself notices a changed slot of each coding: a small one, a field element stored in full, a hashed component
    slot_of = {n: s for s, n in enumerate(names)}
    for name in ("main.processed[1]", "main.sumDec[0]", "main.rHasher.anon_Poseidon_chunk[0].pEx.sigmaP[3].in2"):
        bad = bytearray(wit[:wb])
        bad[32 * slot_of[name]] ^= 1
        assert ct.mismatch(fx, 0, bytes(bad), names) is not None, name


def test_reference_known_answers_and_the_batchs_mix():
    for L in (32, 72):
        fx = ct.load_fixture(L)
        ref = [(n, inp) for n, inp in fx["cases"] if n.startswith("ref_")]
        assert len(ref) == 7
        for (name, inp), (enc, dec, valid), i in zip(ref, REFERENCE, range(7)):
            assert inp == {"encoded": ct.pad(enc, L), "decoded": ct.pad(dec, L)}
            assert int(fx["codes"][i][1]) == valid, name          # slot 1 = main.isValid
    fx = ct.load_fixture(ct.BATCH)
    batch = [i for i, (n, _) in enumerate(fx["cases"]) if n.startswith("batch_")]
    valid = sum(int(fx["codes"][i][1]) for i in batch)
    minus = sum(-1 in ct.should_remove(fx["cases"][i][1]["encoded"]) for i in batch)
    assert len(batch) == 130 and valid >= 40 and 130 - valid >= 40 and minus >= 10
    # equal and unequal sums: inv of the final IsZero is 0 exactly for the valid ones
    wit, _, wb, names = _host_witnesses(ct.BATCH)
    inv = names.index("main.anon_IsEqual_final.isz.inv")
    for i in batch:
        assert (wit[i * wb + 32 * inv:i * wb + 32 * inv + 32] == bytes(32)) == bool(fx["codes"][i][1])


def test_literal_semantics_of_an_at_before_the_first_plus():
    """"a@b+c.d": shouldRemove is -1 on the '@' and the 'b', processed is twice the byte there and rEnc takes the factor 2 r - 1"""
    L = 8
    fx = ct.load_fixture(L)
    i = next(k for k, (n, _) in enumerate(fx["cases"]) if n == "own_at_before_plus")
    enc = fx["cases"][i][1]["encoded"]
    assert ct.should_remove(enc) == [0, -1, -1, 0, 0, 0, 0, 0]
    wit, _, wb, names = _host_witnesses(L)
    w = _ints(wit[i * wb:(i + 1) * wb])
    v = lambda n: w[names.index(n)]
    assert [v(f"main.processed[{k}]") for k in range(4)] == [97, 128, 196, 43]
    assert [v(f"main.inAliasPart[{k}]") for k in range(4)] == [0, P - 1, P - 1, 0]
    r = v("main.muxEnc[0].mux.out[0]")                                       # rEnc[0] = r
    assert v("main.muxEnc[1].c[0]") == r * r % P                             # kept whatever shouldRemove is
    assert v("main.muxEnc[1].mux.out[0]") == r * (2 * r - 1) % P
    assert v("main.muxEnc[2].mux.out[0]") == r * (2 * r - 1) ** 2 % P


@pytest.mark.parametrize("L", ct.SHAPES)
def test_emitted_constraints_hold_for_every_fixture_witness_and_reject_tampering(L):
    c = _circuit(L)
    sym = c.symbols()
    cons = zr.clean_email_address_main_constraints(sym, L)
    assert len(cons) == zr.clean_email_address_constraint_count(L)
    used = set()                                      # every wire but the constant is constrained
    for a, b, cc in cons:
        used.update(a, b, cc)
    assert used | {0} == set(range(c.W))
    fx = ct.load_fixture(L)
    wit, _, wb, names = _host_witnesses(L)            # (equal to the fixtures in every slot: the test above)
    first = None
    for i, (name, _) in enumerate(fx["cases"]):
        if not (name.startswith("batch_") and int(name[6:]) % 13):
            w = _ints(wit[i * wb:(i + 1) * wb])
            assert r1cs_util.first_violation(cons, w) is None, name
            first = w if first is None and w[1] == 0 else first      # (IsZero leaves inv free where its input is 0: tamper with an invalid one)
    slot_of = {n: s for s, n in sym}
    # a flipped shouldRemove shows in processed and in muxEnc's output (shouldRemove itself is linear: not a wire)
    for t in ("main.processed[1]", "main.inAliasPart[2]", "main.muxEnc[3].mux.out[0]", "main.muxEnc[3].c[0]", f"main.sumDec[{L - 1}]",
              "main.sumEnc[0]", "main.anon_IsEqual_final.isz.inv", "main.anon_IsEqual_final.isz.out", "main.isValid", "main.rDec[1]"):
        w = list(first)
        w[slot_of[t]] = (w[slot_of[t]] + 1) % P
        assert r1cs_util.first_violation(cons, w) is not None, t


def test_constraint_count_formula():
    assert zr.clean_email_address_constraint_count(32) == 3751
    assert [zr.clean_email_address_constraint_count(L) for L in (8, 24)] == [
        3 * 204 * n + 3 * 81 * (n - 1) + 2 * (3 * L + 1) + 12 * L - 5 + 1 for L, n in ((8, 1), (24, 3))]


def test_r1cs_export_is_satisfied(tmp_path):
    """python -m zkwg.r1cs --main clean-email-address: the product's `.r1cs` reader and check core (zkwg_r1cs.h on the host) accept
    the witnesses of the reference's shape and reject a changed one"""
    import hosttest
    out = tmp_path / "cea.r1cs"
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "zk-email-verify_amd", "py"))
    subprocess.check_call([sys.executable, "-m", "zkwg.r1cs", "--main", "clean-email-address", "--max-length", "32", "-o", str(out),
                           "--sym", str(tmp_path / "cea.sym")], env=env)
    data = out.read_bytes()
    n_wires, n_out, n_pub, n_prv, _, n_cons = struct.unpack_from("<IIIIQI", data, 12 + 12 + 4 + 32)
    assert (n_wires, n_out, n_pub, n_prv, n_cons) == (3816, 1, 0, 64, 3751)
    assert (tmp_path / "cea.sym").read_text().splitlines()[0] == "1,1,0,main.isValid"
    lib = hosttest.load()
    wit, _, wb, _ = _host_witnesses(32)
    for i in range(len(wit) // wb):
        assert lib.ht_r1cs_first_bad(data, len(data), wit[i * wb:(i + 1) * wb]) == -1, i
    bad = bytearray(wit[:wb])
    bad[32 * 200] ^= 1
    assert lib.ht_r1cs_first_bad(data, len(data), bytes(bad)) >= 0


def test_configuration_bounds():
    M = zkwg.MAIN_CLEAN_EMAIL_ADDRESS
    assert M == ct.MAIN == 7

    def refused(what, **kw):
        kw = dict(dict(main_kind=M, n=0, k=0), **kw)
        with pytest.raises(zkwg.ZkwgError, match=what):
            zkwg.Circuit(device=-1, **kw)
    for L in (8, 1024):
        zkwg.Circuit(device=-1, **ct.circuit_kwargs(L)).close()
    for L in (12, 0, 1032, 4, 20):
        refused("multiple of 8", max_header=L, max_body=L)
    refused("max_body must equal max_header", max_header=32, max_body=24)
    refused("max_body must equal max_header", max_header=32, max_body=0)
    refused("n, k and every flag", max_header=32, max_body=32, n=1)
    refused("n, k and every flag", max_header=32, max_body=32, k=17)
    for flag in ("ignore_body_hash_check", "enable_header_masking", "enable_body_masking", "remove_soft_line_breaks"):
        refused(None, max_header=64, max_body=64, **{flag: 1})
    refused("no .sym", max_header=32, max_body=32, sym="1,1,0,main.isValid\n")            # no `.sym` layout for this main
    c = _circuit(32)
    with pytest.raises(zkwg.ZkwgError):                                                  # no attached constraint system
        c.attach_r1cs(zr.write_r1cs(c.W, zr.clean_email_address_main_constraints(c.symbols(), 32), 1, 0, 64))
    assert c.lib.zkwg_inverse_table_half(c.h) == 256                                     # K - byte lies in [-212, 64]
    assert c.in_stride % 16 == 0 and c.lib.zkwg_input_offset(c.h, 1) == 64               # the record pads both slots to 64 bytes


def test_inputs_that_are_not_bytes_are_refused_by_the_shim():
    c = _circuit(8)
    inp = {"encoded": ct.pad("a.b@c", 8), "decoded": ct.pad("ab@c", 8)}
    c.pack(inp)
    for key in ("encoded", "decoded"):
        with pytest.raises(zkwg.ZkwgError, match="not a byte"):
            c.pack(dict(inp, **{key: [256] + [0] * 7}))
        with pytest.raises(zkwg.ZkwgError, match="Not enough values"):
            c.pack(dict(inp, **{key: [1] * 7}))
    with pytest.raises(zkwg.ZkwgError, match="Signal not found"):
        c.pack(dict(inp, **{"in": [0] * 8}))


def test_clean_email_address_helper_on_the_reference_strings():
    for enc, dec, valid in REFERENCE:
        assert (zi.clean_email_address(enc) == dec) == bool(valid)
    assert zi.clean_email_address("a.b+c@d.e") == "ab@d.e" and zi.clean_email_address("+x@y") == "@y"
    for bad in ("no-at-sign", "a@b@c", "a@b+c.d"):
        with pytest.raises(ValueError):
            zi.clean_email_address(bad)
    inp = zi.generate_clean_email_address_inputs("shreyas.londhe+alias@gmail.com", 32)
    assert [int(x) for x in inp["encoded"]] == ct.pad(REFERENCE[0][0], 32) and [int(x) for x in inp["decoded"]] == ct.pad(REFERENCE[0][1], 32)
    with pytest.raises(ValueError):
        zi.generate_clean_email_address_inputs("a" * 30 + "@b.c", 32)
    # helper-made inputs are valid witnesses of the host core; one changed byte is not
    c = _circuit(32)
    addrs = ["first.last+tag@example.org", "plain@example.org", "a.b.c.d+e+f@x.y"]
    made = [zi.generate_clean_email_address_inputs(a, 32) for a in addrs]
    broken = [dict(m, decoded=[str(int(m["decoded"][0]) ^ 1)] + m["decoded"][1:]) for m in made]
    wit, status = ct.host_witnesses(c, made + broken)
    wb = c.witness_bytes
    assert status == [0] * 6
    assert [wit[i * wb + 32] for i in range(6)] == [1, 1, 1, 0, 0, 0]


def test_generate_witness_names_the_main_by_its_template_parameter():
    from zkwg import generate_witness as gw
    assert gw.circuit_kwargs("CleanEmailAddress(32)") == ct.circuit_kwargs(32)
    c = _circuit(32)
    wit, _, wb, _ = _host_witnesses(32)
    w = c.wtns(wit[:wb])                                                             # the `.wtns` writer
    assert w[:4] == b"wtns" and len(w) > 32 * c.W


def test_js_shim_packs_the_same_record():
    """js/zkwg.js: the new kind and its two input names -- the record of a fixture input is Python's; a non-byte is refused"""
    import json
    import shutil
    js = os.path.join(ROOT, "zk-email-verify_amd", "js")
    if shutil.which("node") is None or not os.path.exists(os.path.join(js, "zkwg_addon.node")):
        pytest.skip("node or the built addon is missing")
    c = _circuit(24)
    inp = ct.load_fixture(24)["cases"][0][1]
    script = ("const z = require(%r); const inp = JSON.parse(require('fs').readFileSync(0, 'utf8'));"
              "const c = new z.Circuit({mainKind: z.MAIN_CLEAN_EMAIL_ADDRESS, maxHeader: 24, maxBody: 24, n: 0, k: 0}, -1);"
              "let refused = 0; try { new z.Circuit({mainKind: z.MAIN_CLEAN_EMAIL_ADDRESS, maxHeader: 12, maxBody: 12, n: 0, k: 0}, -1); } catch (e) { refused = 1; }"
              "let nonbyte = 0; try { c.pack(Object.assign({}, inp, {decoded: [256].concat(inp.decoded.slice(1))})); } catch (e) { nonbyte = /not a byte/.test(e.message) ? 1 : 0; }"
              "console.log(JSON.stringify({W: c.witnessLen, pub: c.numPublic, refused, nonbyte, rec: c.pack(inp).toString('hex')}));") % os.path.join(js, "zkwg.js")
    out = subprocess.run(["node", "-e", script], input=json.dumps(inp), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout)
    assert (got["W"], got["pub"], got["refused"], got["nonbyte"]) == (c.W, c.n_public, 1, 1)
    assert bytes.fromhex(got["rec"]) == c.pack(inp)


def test_core_under_the_sanitizers_as_a_stand_alone_program(tmp_path):
    exe = tmp_path / "ceatest_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DCEATEST_MAIN",
                           "-I", os.path.join(ROOT, "zk-email-verify_amd", "csrc"), os.path.join(ROOT, "tests", "native", "ceatest.cpp"),
                           "-o", str(exe)])
    for L in ct.SHAPES:
        c = _circuit(L)
        fx = ct.load_fixture(L)
        cfg = c.cfg
        cases = [inp for n, inp in fx["cases"] if not (n.startswith("batch_") and int(n[6:]) % 10)]
        valid = [int(fx["codes"][i][1]) for i, (n, _) in enumerate(fx["cases"]) if not (n.startswith("batch_") and int(n[6:]) % 10)]
        path = tmp_path / "cases.bin"
        path.write_bytes(struct.pack("<10I", cfg.main_kind, cfg.max_header, cfg.max_body, cfg.n, cfg.k, 0, 0, 0, 0, 0) +
                         struct.pack("<II", len(cases), c.in_stride) + b"".join(c.pack(i) for i in cases))
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l.split() for l in r.stdout.splitlines()]
        assert [(int(l[0]), int(l[1])) for l in lines] == [(0, v) for v in valid], L
