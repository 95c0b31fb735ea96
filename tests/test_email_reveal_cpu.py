"""The application main EmailReveal without a GPU (zk-email-verify_amd/circuits/email-reveal.circom, ZKWG_MAIN_EMAIL_REVEAL):
EmailVerifier + RevealSubstring over the header or the body + the revealed bytes packed 31 per public signal + the email nullifier.

The fixtures (tests/golden/email_reveal, written by tests/golden/make_email_reveal_fixture.py) hold what the circom interpreter
computes from the project's circom file over the reference's templates.  Checked here: the C++ walker's names and order, what the
layout drops, the main's own prepare cores on the host (zkwg_substr_core.h + zkwg_app_core.h) with the host expansion, the exported
constraint system and its count, the configuration bounds and refusals, that the plain EmailVerifier layout did not move, and the
cores under the address / undefined-behaviour sanitizers as a stand-alone program.  EmailVerifier's own kernels have no host
build: its slots are compared on the device (tests/test_email_reveal_gpu.py)."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import emailreveal as er
import hosttest
import zkwg
from conftest import ROOT
from zkwg import r1cs as zr

P = er.P
NAMES = tuple(er.SHAPES)
_cache = {}


def _circuit(name):
    if ("c", name) not in _cache:
        c = zkwg.Circuit(device=-1, **er.circuit_kwargs(name))
        _cache["c", name] = (c, c.symbols())
    return _cache["c", name]


def _system(name):
    """(constraints, `.r1cs` bytes) of shape `name`, built once"""
    if ("r", name) not in _cache:
        c, sym = _circuit(name)
        cons = zr.email_reveal_constraints(sym, *er.SHAPES[name])
        _cache["r", name] = (cons, zr.email_reveal_r1cs(sym, *er.SHAPES[name]))
    return _cache["r", name]


def _host_witness(name):
    """the fixture's email through the host cores and zkwg_expand_host"""
    if ("h", name) not in _cache:
        c, _ = _circuit(name)
        rec = c.pack(er.load_fixture(name)["inputs"])
        scr, status = er.host_images(c, rec)
        _cache["h", name] = (c.expand_host(rec, 1, scr, 0, 1, threads=2), status, rec)
    return _cache["h", name]


@pytest.mark.parametrize("name", NAMES)
def test_walker_symbols_follow_the_interpreter(name):
    c, sym = _circuit(name)
    fx = er.load_fixture(name)
    N, M, ignore, body, S, uniq, nul = er.SHAPES[name]
    chunks = (S + 30) // 31
    assert len(sym) == c.W == fx["W"] and [s for s, _ in sym] == list(range(c.W))
    assert er.sym_hash(sym) == fx["sym_sha256"]
    assert len(set(fx["o0_index"].tolist())) == c.W and fx["o0_index"][0] == 0       # every slot is one signal of the interpreter's
    assert c.n_public == 1 + nul + chunks
    names = [n for _, n in sym]
    assert names[:2 + nul] == ["one", "main.pubkeyHash"] + ["main.emailNullifier"] * nul
    assert names[2 + nul:2 + nul + chunks] == [f"main.revealed[{i}]" for i in range(chunks)]
    inputs = ["emailHeader[0]", "emailHeaderLength", "pubkey[0]", "signature[0]"] + ([] if ignore else ["bodyHashIndex", "precomputedSHA[0]", "emailBody[0]", "emailBodyLength"]) + \
        ["substringStartIndex", "substringLength"]
    at = [names.index("main." + i) for i in inputs]
    assert at == sorted(at) and at[0] == 2 + nul + chunks                             # the inputs, in the template's order
    first = lambda p: next(i for i, n in enumerate(names) if n.startswith(p))
    order = [first("main.ev."), first("main.rs.")] + ([first("main.anon_EmailNullifier.")] if nul else [])
    assert order == sorted(order) and order[0] == at[-1] + 1
    # the match matrix and the +-65,025 inverse table only with the uniqueness check
    seg_types = {t[2] for t in c.segment_table()}
    assert (23 in seg_types) == bool(uniq)
    assert c.lib.zkwg_inverse_table_half(c.h) == (255 * 255 if uniq else 2100)
    if nul:      # 420 + 216 S-box signals
        assert sum(n.startswith("main.anon_EmailNullifier.anon_PoseidonLarge.") for n in names) == 420
        assert sum(n.startswith("main.anon_EmailNullifier.anon_Poseidon.") for n in names) == 216


def test_fixtures_are_what_the_interpreter_computes_today():
    from oracle.circom import ev
    if not ev.reference_available():
        pytest.skip("the reference tree is not present")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_email_reveal_fixture as mk
    assert mk.main(["--check"]) == 0


# what the kept-v1 rule drops outside `ev`: copies of inputs and outputs, and linear definitions (sums, aliases, constants)
LINEAR_LEAVES = {"in", "in[]", "out", "out[]", "inputs[]", "initialState", "poseidonInput[]", "signatureHash", "signature[]", "intSums[]",
                 "isSubstringLengthValid", "isSubstringStartIndexValid", "isSumValid", "sum", "sums[]", "nums[]", "count", "substring[]",
                 "substringLength", "substringStartIndex", "length", "startIndex", "shift", "firstElementNonZero", "isMatch",
                 "isZeroDifference[]", "matchAccumulator[]"}


@pytest.mark.parametrize("name", NAMES)
def test_dropped_signals_are_linear(name):
    c, sym = _circuit(name)
    fx = er.load_fixture(name)
    N, M, ignore, body, S, uniq, nul = er.SHAPES[name]
    dropped = {p: n for n, p in fx["dropped"]}
    assert sum(dropped.values()) == fx["n_o0"] - c.W
    ev = {p.replace("main.ev.", "main.", 1): n for p, n in dropped.items() if p.startswith("main.ev.")}
    own_io = {"main.emailHeader[]": N, "main.emailHeaderLength": 1, "main.pubkey[]": 17, "main.signature[]": 17, "main.pubkeyHash": 1,
              "main.shaHi": 1, "main.shaLo": 1}
    if not ignore:
        own_io.update({"main.bodyHashIndex": 1, "main.precomputedSHA[]": 32, "main.emailBody[]": M, "main.emailBodyLength": 1})
    for p, n in own_io.items():            # the component's copies of the inputs and its three outputs: aliases
        assert ev.pop(p) == n, p
    if not ignore:   # the rest of `ev` is exactly what the plain EmailVerifier(576, 192) fixture documents as dropped
        plain = np.load(os.path.join(ROOT, "tests", "golden", "circom_ev_576_192.npz"))
        assert ev == {l.split()[1]: int(l.split()[0]) for l in bytes(plain["dropped"]).decode().splitlines()}
    rest = {p: n for p, n in dropped.items() if not p.startswith("main.ev.")}
    assert rest and all(p.startswith(("main.rs.", "main.anon_PackBytes.", "main.anon_EmailNullifier.")) for p in rest)
    for p, n in rest.items():
        leaf = p.rsplit(".", 1)[1]
        assert leaf in LINEAR_LEAVES, p
        # `out` is quadratic in three places, `matchAccumulator` beyond its constant first element: those are kept
        assert not (leaf == "out[]" and p.endswith("selectSubArray.out[]")) and "n2b.out" not in p
        assert not (leaf == "out" and (".sigmaF" in p or ".sigmaP" in p or "anon_IsZero" in p))
        if leaf == "matchAccumulator[]":
            assert n == (M if body else N)
    L = M if body else N
    kept = {n for _, n in sym}
    assert f"main.rs.selectSubArray.out[{S - 1}]" in kept and "main.rs.selectSubArray.shifter.tmp[0]" in kept
    if uniq:
        assert f"main.rs.countSubstringOccurrences.matches[{L - 1}].matchAccumulator[{S}]" in kept
    assert rest["main.anon_PackBytes.intSums[]"] == 31 * ((S + 30) // 31)


@pytest.mark.parametrize("name", NAMES)
def test_host_cores_and_host_expansion_equal_the_interpreter(name):
    """every slot outside EmailVerifier's own values: the outputs, the inputs, RevealSubstring's signals, the nullifier's S-boxes"""
    c, sym = _circuit(name)
    fx = er.load_fixture(name)
    wit, status, _ = _host_witness(name)
    assert status == [0]
    ev_owned = {"main.pubkeyHash", "main.emailHeaderLength", "main.bodyHashIndex", "main.emailBodyLength"}
    mine = [s for s, n in sym if not n.startswith("main.ev.") and n not in ev_owned]
    assert len(mine) > c.W - sum(n.startswith("main.ev.") for _, n in sym) - 5
    exp = fx["witness"]
    for s in mine:
        assert wit[32 * s:32 * s + 32] == exp[32 * s:32 * s + 32], sym[s][1]


@pytest.mark.parametrize("name", NAMES)
def test_packed_bytes_and_nullifier_equal_an_independent_evaluation(name):
    from oracle.pyref import poseidon
    c, sym = _circuit(name)
    fx = er.load_fixture(name)
    N, M, ignore, body, S, uniq, nul = er.SHAPES[name]
    inp = fx["inputs"]
    w = er.ints(fx["witness"])
    slot = {n: s for s, n in sym}
    a, ln = int(inp["substringStartIndex"]), int(inp["substringLength"])
    src = bytes(int(x) for x in inp["emailBody" if body else "emailHeader"])
    sub = src[a:a + ln] + bytes(S - ln)
    packed = [int.from_bytes(sub[31 * i:31 * i + 31], "little") for i in range((S + 30) // 31)]
    assert [w[slot[f"main.revealed[{i}]"]] for i in range(len(packed))] == packed
    assert ln > 31 or name == "A"
    host = er.ints(_host_witness(name)[0])
    assert [host[slot[f"main.revealed[{i}]"]] for i in range(len(packed))] == packed
    if nul:
        sig = [int(x) for x in inp["signature"]]
        merged = [sig[2 * i] + (sig[2 * i + 1] << 121) for i in range(8)] + [sig[16]]
        want = poseidon.poseidon_hash([poseidon.poseidon_hash(merged)])
        assert w[slot["main.emailNullifier"]] == want == host[slot["main.emailNullifier"]]
    else:
        assert "main.emailNullifier" not in slot


@pytest.mark.parametrize("name", NAMES)
def test_exported_system_holds_and_rejects_tampering(name):
    c, sym = _circuit(name)
    fx = er.load_fixture(name)
    N, M, ignore, body, S, uniq, nul = er.SHAPES[name]
    cons, data = _system(name)
    lib = hosttest.load()
    hdr = struct.unpack_from("<IIIIQI", data, 12 + 12 + 4 + 32)
    assert hdr[0] == c.W and hdr[1] == c.n_public and hdr[2] == 0 and hdr[1] + hdr[3] == sym[[n for _, n in sym].index("main.substringLength")][0] and hdr[5] == len(cons)
    assert lib.ht_r1cs_first_bad(data, len(data), fx["witness"]) == -1
    # every wire but the constant and the 17 top carries the reference's CheckCarryToZero never reads is constrained
    used = set()
    for a, b, cc in cons:
        used.update(a, b, cc)
    free = [sym[k][1] for k in sorted(set(range(c.W)) - used - {0})]
    assert len(free) == 17 and all(n.startswith("main.ev.rsaVerifier.bigPow.") and n.endswith(".tCheck.carry[32]") for n in free)
    slot = {n: s for s, n in sym}
    L = M if body else N
    targets = ["main.revealed[0]", "main.ev.anon_Sha256Bytes.sha.sha256compression[1].t1[5].ch.out[3]", "main.rs.selectSubArray.out[1]"]
    if nul:
        targets += ["main.anon_EmailNullifier.anon_Poseidon.pEx.sigmaP[7].in2", "main.anon_EmailNullifier.anon_PoseidonLarge.anon_Poseidon.pEx.sigmaF[3][4].out", "main.emailNullifier"]
    if uniq:
        targets += [f"main.rs.countSubstringOccurrences.matches[{L // 2}].difference[0]"]
    for t in targets:
        bad = bytearray(fx["witness"])
        bad[32 * slot[t]] ^= 1
        assert lib.ht_r1cs_first_bad(data, len(data), bytes(bad)) >= 0, t


@pytest.mark.parametrize("name", ("A", "C"))
def test_constraint_count_is_the_formula(name):
    N, M, ignore, body, S, uniq, nul = er.SHAPES[name]
    c0 = zkwg.Circuit(zkwg.MAIN_EMAIL_VERIFIER, max_header=N, max_body=M, ignore_body_hash_check=ignore, device=-1)
    n_ev = len(zr.email_verifier_constraints(c0.symbols(), N, M, ignore_body_hash_check=ignore))
    cons, _ = _system(name)
    assert len(cons) == zr.email_reveal_constraint_count(N, M, ignore, body, S, uniq, nul, n_ev)
    if name == "A":      # B: the same EmailVerifier, the body's RevealSubstring without the match matrix, no nullifier
        nb = er.SHAPES["B"]
        assert len(_system("B")[0]) == zr.email_reveal_constraint_count(*nb, n_ev)


def test_plain_email_verifier_layout_did_not_move():
    """the walker was split into allocation, main I/O and sub-components: names, order and W of the plain main are what the stored
    interpreter fixture of EmailVerifier(576, 192) indexes"""
    c0 = zkwg.Circuit(zkwg.MAIN_EMAIL_VERIFIER, max_header=576, max_body=192, device=-1)
    fx = np.load(os.path.join(ROOT, "tests", "golden", "circom_ev_576_192.npz"))
    sym = c0.symbols()
    assert c0.W == len(fx["o0_index"]) == 735631 and c0.n_public == 20 and c0.in_stride == 1632
    assert er.sym_hash(sym).startswith("9b709ab7d5eca62e")
    names = [n for _, n in sym]
    assert names[1:4] == ["main.pubkeyHash", "main.shaHi", "main.shaLo"] and names[4] == "main.pubkey[0]"
    assert not any(n.startswith(("main.ev.", "main.rs.")) for n in names)
    # the two new record fields take no room in the records of the other mains
    assert c0.lib.zkwg_input_offset(c0.h, 13) == c0.lib.zkwg_input_offset(c0.h, 14) == c0.in_stride
    a, _ = _circuit("A")
    assert a.in_stride == c0.in_stride + 16 and [a.lib.zkwg_input_offset(a.h, f) for f in range(13)] == [c0.lib.zkwg_input_offset(c0.h, f) for f in range(13)]
    assert (a.lib.zkwg_input_offset(a.h, 13), a.lib.zkwg_input_offset(a.h, 14)) == (c0.in_stride, c0.in_stride + 4)


def test_configuration_bounds_and_refusals():
    E = zkwg.MAIN_EMAIL_REVEAL
    base = dict(main_kind=E, max_header=576, max_body=192, reveal_from_body=0, max_substring=12, check_uniqueness=1, with_nullifier=1)
    ok = lambda **kw: zkwg.Circuit(device=-1, **dict(base, **kw)).close()

    def refused(match=None, **kw):
        with pytest.raises(zkwg.ZkwgError, match=match):
            zkwg.Circuit(device=-1, **dict(base, **kw))
    ok()
    ok(max_substring=2)
    ok(max_substring=575)
    ok(reveal_from_body=1, max_substring=191)
    ok(ignore_body_hash_check=1, max_body=0)
    refused(max_substring=1)
    refused(max_substring=576)                               # assert(maxSubstringLength < maxLength)
    refused(reveal_from_body=1, max_substring=192)
    refused(reveal_from_body=1, ignore_body_hash_check=1)    # a body that no hash binds to the signature
    for flag in ("reveal_from_body", "check_uniqueness", "with_nullifier"):
        refused(**{flag: 2})
    refused(n=120)
    refused(k=16)
    refused(max_header=600)                                  # EmailVerifier's rules for the lengths
    refused(max_body=100)
    for flag in ("enable_header_masking", "enable_body_masking", "remove_soft_line_breaks"):
        refused(**{flag: 1})
    refused(match="EmailReveal", sym="1,1,0,main.pubkeyHash\n")
    refused(match="EmailReveal", regex=os.path.join(ROOT, "oracle", "circom", "lib", "@zk-email", "zk-regex-circom", "circuits", "common", "body_hash_regex.circom"))
    # the plain creation call refuses the kind and names the call that takes the parameters
    lib = zkwg._lib.load()
    h = C.c_void_p()
    cfg = zkwg.Config(E, 576, 192, 121, 17, 0, 0, 0, 0, 0)
    assert lib.zkwg_circuit_create(C.byref(cfg), -1, C.byref(h)) == -1 and b"zkwg_circuit_create_app" in lib.zkwg_last_error()
    app = zkwg._lib.AppConfig(0, 12, 1, 1)
    cfg0 = zkwg.Config(zkwg.MAIN_EMAIL_VERIFIER, 576, 192, 121, 17, 0, 0, 0, 0, 0)
    assert lib.zkwg_circuit_create_app(C.byref(cfg0), C.byref(app), -1, C.byref(h)) == -1
    assert lib.zkwg_abi_version() == 3
    # no attached constraint system (and with it no expand_abc)
    c, _ = _circuit("C")
    with pytest.raises(zkwg.ZkwgError):
        c.attach_r1cs(_system("C")[1])


def test_inputs_the_generic_path_and_the_needle():
    from zkwg import inputs, synth
    c, _ = _circuit("C")
    inp = dict(er.load_fixture("C")["inputs"])
    rec = c.pack(inp)
    off = lambda f: c.lib.zkwg_input_offset(c.h, f)
    assert struct.unpack_from("<II", rec, off(13)) == (int(inp["substringStartIndex"]), int(inp["substringLength"]))
    with pytest.raises(zkwg.ZkwgError, match="Not all inputs"):
        c.pack({k: v for k, v in inp.items() if k != "substringLength"})
    # a start or a length that does not fit its u32, a source element that is not a byte: range flag -> status 4
    flags = lambda r: struct.unpack_from("<I", r, off(12))[0]
    assert flags(rec) == 0
    assert flags(c.pack(dict(inp, substringStartIndex=str(1 << 32)))) == 1 << 13
    assert flags(c.pack(dict(inp, substringLength=str(P - 1)))) == 1 << 14
    hdr = list(inp["emailHeader"])
    hdr[5] = "256"
    assert flags(c.pack(dict(inp, emailHeader=hdr))) == 1 << 0
    recs = rec + c.pack(dict(inp, substringStartIndex=str(1 << 32))) + c.pack(dict(inp, emailHeader=hdr))
    assert er.host_images(c, recs)[1] == [0, 4, 4]
    # the needle is looked up in what the circuit sees
    d = synth.synthetic_dkim_result(7, 0, body_len=60)
    params = er.reveal_params(er.SHAPES["A"])
    got = inputs.generate_email_reveal_inputs_from_dkim_result(d, params, needle=b"message-id:<")
    assert int(got["substringStartIndex"]) == d["headers"].index(b"message-id:<") and got["substringLength"] == "12"
    assert {k: v for k, v in got.items() if not k.startswith("substring")} == inputs.generate_email_verifier_inputs_from_dkim_result(d, 576, 192)
    with pytest.raises(ValueError, match="does not occur"):
        inputs.generate_email_reveal_inputs_from_dkim_result(d, params, needle=b"no such text")
    with pytest.raises(ValueError, match="more than once"):
        inputs.generate_email_reveal_inputs_from_dkim_result(d, params, needle=b"example.com")
    inputs.generate_email_reveal_inputs_from_dkim_result(d, dict(params, shouldCheckUniqueness=0), needle=b"example.com")
    assert inputs.generate_email_reveal_inputs_from_dkim_result(d, params, start=3, length=4)["substringStartIndex"] == "3"
    with pytest.raises(ValueError):
        inputs.generate_email_reveal_inputs_from_dkim_result(d, dict(params, revealFromBody=1, ignoreBodyHashCheck=1), start=0, length=1)


def test_r1cs_command_line_writes_the_same_system(tmp_path):
    out = tmp_path / "reveal.r1cs"
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "zk-email-verify_amd", "py"))
    subprocess.check_call([sys.executable, "-m", "zkwg.r1cs", "--main", "email-reveal", "--max-header", "576", "--max-body", "0",
                           "--ignore-body-hash-check", "1", "--max-substring", "33", "--check-uniqueness", "1", "--with-nullifier", "1",
                           "-o", str(out), "--sym", str(tmp_path / "reveal.sym")], env=env)
    assert out.read_bytes() == _system("C")[1]
    assert (tmp_path / "reveal.sym").read_text().splitlines()[:2] == ["1,1,0,main.pubkeyHash", "2,2,0,main.emailNullifier"]
    c, _ = _circuit("C")
    w = c.wtns(er.load_fixture("C")["witness"])
    assert w[:4] == b"wtns" and len(w) > 32 * c.W


def test_cores_under_the_sanitizers_as_a_stand_alone_program(tmp_path):
    exe = tmp_path / "apptest_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DAPPTEST_MAIN",
                           "-I", os.path.join(ROOT, "zk-email-verify_amd", "csrc"), os.path.join(ROOT, "tests", "native", "apptest.cpp"),
                           "-o", str(exe)])
    for name in NAMES:
        c, _ = _circuit(name)
        cfg, app = c.cfg, c.app
        inp = er.load_fixture(name)["inputs"]
        L = cfg.max_body if app.reveal_from_body else cfg.max_header
        # the fixture's email, then the edges of the index range: the last byte, a start and a sum one past the end, a length past S
        cases = [(inp, 0), (dict(inp, substringStartIndex=L - 1, substringLength=1), None), (dict(inp, substringStartIndex=L, substringLength=1), 4),
                 (dict(inp, substringStartIndex=L - 1, substringLength=2), 4), (dict(inp, substringStartIndex=0, substringLength=app.max_substring + 1), 4),
                 (dict(inp, substringStartIndex=(1 << 32) - 1, substringLength=(1 << 32) - 1), 4)]
        path = tmp_path / "cases.bin"
        path.write_bytes(struct.pack("<10I", cfg.main_kind, cfg.max_header, cfg.max_body, cfg.n, cfg.k, cfg.ignore_body_hash_check, 0, 0, 0, 0) +
                         struct.pack("<4I", app.reveal_from_body, app.max_substring, app.check_uniqueness, app.with_nullifier) +
                         struct.pack("<II", len(cases), c.in_stride) + b"".join(c.pack(i) for i, _ in cases))
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        got = [int(l.split()[0]) for l in r.stdout.splitlines()]
        assert len(got) == len(cases) and all(g == e for g, (_, e) in zip(got, cases) if e is not None), (name, got)


def test_generate_witness_names_the_main_by_its_template_parameters():
    from zkwg import generate_witness as gw
    assert gw.circuit_kwargs("EmailReveal(576, 0, 121, 17, 1, 0, 33, 1, 1)") == dict(er.circuit_kwargs("C"), n=121, k=17)


def test_js_shim_packs_the_same_record():
    """js/zkwg.js: the new kind, the creation call and the two input names -- the record of the fixture's input is Python's"""
    import json
    import shutil
    js = os.path.join(ROOT, "zk-email-verify_amd", "js")
    if shutil.which("node") is None or not os.path.exists(os.path.join(js, "zkwg_addon.node")):
        pytest.skip("node or the built addon is missing")
    c, _ = _circuit("C")
    inp = er.load_fixture("C")["inputs"]
    script = ("const z = require(%r); const inp = JSON.parse(require('fs').readFileSync(0, 'utf8'));"
              "const c = new z.Circuit({mainKind: z.MAIN_EMAIL_REVEAL, maxHeader: 576, maxBody: 0, ignoreBodyHashCheck: 1, revealFromBody: 0,"
              " maxSubstring: 33, checkUniqueness: 1, withNullifier: 1}, -1);"
              "let refused = 0; try { new z.Circuit({mainKind: z.MAIN_EMAIL_REVEAL, maxHeader: 576, maxBody: 0, ignoreBodyHashCheck: 1, maxSubstring: 576}, -1); } catch (e) { refused = 1; }"
              "console.log(JSON.stringify({W: c.witnessLen, pub: c.numPublic, refused, rec: c.pack(inp).toString('hex')}));") % os.path.join(js, "zkwg.js")
    out = subprocess.run(["node", "-e", script], input=json.dumps(inp), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout)
    assert (got["W"], got["pub"], got["refused"]) == (c.W, c.n_public, 1)
    assert bytes.fromhex(got["rec"]) == c.pack(inp)
