"""The substring mains without a GPU: RevealSubstring(L, S, uniq) and CountSubstringOccurrences(L, S)
(helpers/reveal-substring.circom, utils/array.circom; ZKWG_MAIN_REVEAL_SUBSTRING / ZKWG_MAIN_COUNT_SUBSTRING).

The fixtures (tests/golden/substring, written by tests/golden/make_substring_fixtures.py) hold what the circom interpreter
computes from the reference's own templates.  Checked here: the C++ walker's names and order, the prepare core on the host
(zkwg_substr_core.h) with the host expansion (zkwg_expand_host: the decoders zk_expand3_subm runs), the emitted constraint
system, the configuration bounds, and the core under the address / undefined-behaviour sanitizers as a stand-alone program."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import r1cs_util
import substrtest as st
import zkwg
from conftest import ROOT
from zkwg import r1cs as zr

P = st.P


def _circuit(shape, device=-1):
    return zkwg.Circuit(device=device, **st.circuit_kwargs(*shape))


_host = {}


def _host_witnesses(shape):
    """(witness bytes of every case, statuses) from the host core + zkwg_expand_host, once per shape"""
    if shape not in _host:
        c = _circuit(shape)
        fx = st.load_fixture(*shape)
        recs = b"".join(c.pack(inp) for _, inp, _ in fx["cases"])
        scr, status = st.host_images(c, recs)
        n = len(fx["cases"])
        wit = c.expand_host(recs, n, scr, 0, n, threads=2)
        _host[shape] = (wit, status, c.witness_bytes)
    return _host[shape]


@pytest.mark.parametrize("shape", st.SHAPES)
def test_walker_symbols_follow_the_interpreters_order(shape):
    c = _circuit(shape)
    fx = st.load_fixture(*shape)
    sym = c.symbols()
    assert len(sym) == c.W == fx["W"] and [s for s, _ in sym] == list(range(c.W))
    assert st.sym_hash(sym) == fx["sym_sha256"]
    o0 = fx["o0_index"]
    assert len(o0) == c.W and o0[0] == 0 and bool(np.all(np.diff(o0.astype(np.int64)) > 0))
    kind, L, S, u = shape
    comp = L * (4 * S + 2)
    if kind == st.COUNT:
        assert c.W == 2 + L + S + comp and c.n_public == 1
    else:
        lc = zr.log2ceil
        assert c.W == 1 + S + L + 2 + (lc(L) + 1) + (lc(S + 1) + 1) + (lc(L + 1) + 1) + S + lc(L) * L + lc(L) + S * (lc(S) + 1) + u * comp
        assert c.n_public == S
    if shape == (st.COUNT, 1024, 128, 0):
        assert c.W == 527490


def test_fixtures_are_what_the_interpreter_computes_today():
    from oracle.circom import ev
    if not ev.reference_available():
        pytest.skip("the reference tree is not present")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_substring_fixtures as mk
    assert mk.main(["--check"]) == 0


@pytest.mark.parametrize("shape", st.SHAPES)
def test_host_core_and_host_expansion_equal_every_fixture_slot(shape):
    fx = st.load_fixture(*shape)
    wit, status, wb = _host_witnesses(shape)
    assert status == [s for _, _, s in fx["cases"]]
    assert 0 in status
    for i, (name, _, s) in enumerate(fx["cases"]):
        if s == 0:
            got, exp = wit[i * wb:(i + 1) * wb], fx["witness"][i]
            if got != exp:
                j = next(k for k in range(fx["W"]) if got[32 * k:32 * k + 32] != exp[32 * k:32 * k + 32])
                raise AssertionError(f"{name}: slot {j} ({_circuit(shape).symbols()[j][1]})")


def test_reference_known_answers():
    """reveal-substring.test.ts: witness[1..16]; count-substring-occurrences.test.ts: witness[1]"""
    shape = (st.REVEAL, 256, 16, 1)
    fx = st.load_fixture(*shape)
    by = {n: i for i, (n, _, _) in enumerate(fx["cases"])}
    val = lambda w, k: int.from_bytes(w[32 * k:32 * k + 32], "little")
    for name, exp in (("middle", [51, 52, 53, 54, 55]), ("start", [1, 2, 3, 4, 5]), ("end_of_nonzero", [96, 97, 98, 99, 100]),
                      ("length_1", [51]), ("maximum_length", list(range(1, 17))), ("zero_padded", [1, 2, 3])):
        w = fx["witness"][by["ref_" + name]]
        assert [val(w, k) for k in range(1, 17)] == exp + [0] * (16 - len(exp)), name
    assert sorted(n for n, _, s in fx["cases"] if n.startswith("ref_") and s == 4) == sorted(
        "ref_fail_" + n for n in ("start_eq_max", "start_gt_max", "length_eq_max", "length_gt_max", "sum_gt_max"))
    fx = st.load_fixture(st.COUNT, 1024, 128, 0)
    by = {n: i for i, (n, _, _) in enumerate(fx["cases"])}
    for name, exp in (("single_at_start", 1), ("multiple", 3), ("none", 0), ("overlap", 3), ("full_match", 256), ("single_char", 4),
                      ("at_end", 1)):
        assert val(fx["witness"][by["ref_" + name]], 1) == exp, name
    assert fx["cases"][by["ref_fail_empty_substring"]][2] == 4


def _ints(w):
    return [int.from_bytes(w[i:i + 32], "little") for i in range(0, len(w), 32)]


@pytest.mark.parametrize("shape", [s for s in st.SHAPES if s[1] <= 256])
def test_emitted_constraints_hold_for_every_fixture_witness_and_reject_tampering(shape):
    kind, L, S, u = shape
    c = _circuit(shape)
    sym = c.symbols()
    if kind == st.REVEAL:
        cons = zr.reveal_substring_main_constraints(sym, L, S, u)
        assert len(cons) == zr.reveal_substring_constraint_count(L, S, u)
    else:
        cons = zr.count_substring_main_constraints(sym, L, S)
        assert len(cons) == L * (4 * S + 3) + 1
    # every wire but the constant is constrained
    used = set()
    for a, b, cc in cons:
        used.update(a, b, cc)
    assert used | {0} == set(range(c.W))
    fx = st.load_fixture(*shape)
    first = None
    for i, (name, _, s) in enumerate(fx["cases"]):
        if s == 0 and not (name.startswith("batch_") and int(name[6:]) % 13):
            w = _ints(fx["witness"][i])
            assert r1cs_util.first_violation(cons, w) is None, name
            first = w if first is None else first
    slot_of = {n: s for s, n in sym}
    targets = [] if kind == st.COUNT else ["main.selectSubArray.shifter.tmp[3]"]
    if kind == st.COUNT or u:
        pre = "main" if kind == st.COUNT else "main.countSubstringOccurrences"
        targets += [pre + ".matches[1].difference[0]", pre + ".matches[1].matchAccumulator[1]"]
    for t in targets:
        w = list(first)
        w[slot_of[t]] = (w[slot_of[t]] + 1) % P
        assert r1cs_util.first_violation(cons, w) is not None, t


def test_r1cs_export_of_the_reference_count_main_is_satisfied(tmp_path):
    """python -m zkwg.r1cs --main count-substring at (1024, 128): the product's `.r1cs` reader and check core (zkwg_r1cs.h, on the
    host: tests/native/hosttest.cpp) accept the fixture witnesses"""
    import hosttest
    out = tmp_path / "count.r1cs"
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "zk-email-verify_amd", "py"))
    subprocess.check_call([sys.executable, "-m", "zkwg.r1cs", "--main", "count-substring", "--max-length", "1024", "--max-substring", "128",
                           "-o", str(out), "--sym", str(tmp_path / "count.sym")], env=env)
    data = out.read_bytes()
    n_wires, _, _, _, _, n_cons = struct.unpack_from("<IIIIQI", data, 12 + 12 + 4 + 32)
    assert n_cons == 1024 * (4 * 128 + 3) + 1 and n_wires == 527490
    assert (tmp_path / "count.sym").read_text().splitlines()[0] == "1,1,0,main.count"
    lib = hosttest.load()
    fx = st.load_fixture(st.COUNT, 1024, 128, 0)
    for i in sorted(fx["witness"]):
        assert lib.ht_r1cs_first_bad(data, len(data), fx["witness"][i]) == -1, fx["cases"][i][0]
    bad = bytearray(fx["witness"][0])
    bad[32 * 1200] ^= 1
    assert lib.ht_r1cs_first_bad(data, len(data), bytes(bad)) >= 0


def test_configuration_bounds():
    ok = lambda **kw: zkwg.Circuit(device=-1, **kw).close()

    def refused(**kw):
        with pytest.raises(zkwg.ZkwgError):
            zkwg.Circuit(device=-1, **kw)
    R, CN = zkwg.MAIN_REVEAL_SUBSTRING, zkwg.MAIN_COUNT_SUBSTRING
    ok(main_kind=R, max_header=3, max_body=2, n=1, k=0)
    ok(main_kind=CN, max_header=2, max_body=2, n=0, k=0)
    ok(main_kind=R, max_header=65536, max_body=2, n=0, k=0)
    refused(main_kind=R, max_header=16, max_body=16, n=1, k=0)          # assert(maxSubstringLength < maxLength)
    refused(main_kind=R, max_header=16, max_body=1, n=1, k=0)
    refused(main_kind=R, max_header=65537, max_body=8, n=0, k=0)
    refused(main_kind=R, max_header=16, max_body=8, n=2, k=0)
    refused(main_kind=R, max_header=16, max_body=8, n=1, k=17)
    refused(main_kind=CN, max_header=16, max_body=17, n=0, k=0)         # assert(maxLen >= maxSubstringLen)
    refused(main_kind=CN, max_header=16, max_body=8, n=1, k=0)
    for flag in ("ignore_body_hash_check", "enable_header_masking", "enable_body_masking", "remove_soft_line_breaks"):
        refused(main_kind=R, max_header=16, max_body=8, n=1, k=0, **{flag: 1})
        refused(main_kind=CN, max_header=16, max_body=8, n=0, k=0, **{flag: 1})
    refused(main_kind=R, max_header=16, max_body=8, n=1, k=0, sym="1,1,0,main.substring[0]\n")   # no `.sym` layout for these mains
    # the other mains still insist on multiples of 64
    refused(main_kind=zkwg.MAIN_SHA256_BYTES, max_header=100, max_body=0)
    c = zkwg.Circuit(device=-1, main_kind=R, max_header=64, max_body=8, n=1, k=0)
    assert c.lib.zkwg_inverse_table_half(c.h) == 255 * 255
    c0 = zkwg.Circuit(device=-1, main_kind=R, max_header=64, max_body=8, n=0, k=0)     # no count part: no inverse beyond the default table
    assert c0.lib.zkwg_inverse_table_half(c0.h) == 256


def test_inputs_that_are_not_bytes_or_do_not_fit():
    c = _circuit((st.REVEAL, 64, 8, 1))
    inp = {"in": [1] * 64, "substringStartIndex": 0, "substringLength": 1}
    with pytest.raises(zkwg.ZkwgError, match="not a byte"):
        c.pack(dict(inp, **{"in": [256] + [1] * 63}))
    with pytest.raises(zkwg.ZkwgError, match="Not enough values"):
        c.pack(dict(inp, **{"in": [1] * 63}))
    # an index that does not fit its u32 slot: range flag, status 4 (it cannot pass the template's LessThan)
    recs = c.pack(dict(inp, substringStartIndex=1 << 32)) + c.pack(dict(inp, **{"in": [9] + [1] * 63}))
    _, status = st.host_images(c, recs)
    assert status == [4, 0]


def test_generate_witness_names_the_mains_by_their_template_parameters():
    from zkwg import generate_witness as gw
    assert gw.circuit_kwargs("RevealSubstring(256, 16, 1)") == dict(main_kind=zkwg.MAIN_REVEAL_SUBSTRING, max_header=256, max_body=16, n=1, k=0)
    assert gw.circuit_kwargs("CountSubstringOccurrences(1024,128)") == dict(main_kind=zkwg.MAIN_COUNT_SUBSTRING, max_header=1024, max_body=128, n=0, k=0)
    c = zkwg.Circuit(device=-1, **gw.circuit_kwargs("RevealSubstring(256, 16, 1)"))
    w = c.wtns(st.load_fixture(st.REVEAL, 256, 16, 1)["witness"][0])           # the `.wtns` writer
    assert w[:4] == b"wtns" and len(w) > 32 * c.W
    assert c.lib.zkwg_strerror(4).decode().endswith("Assert Failed") or "Assert Failed" in c.lib.zkwg_strerror(4).decode()


def test_core_under_the_sanitizers_as_a_stand_alone_program(tmp_path):
    exe = tmp_path / "substrtest_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSUBSTRTEST_MAIN",
                           "-I", os.path.join(ROOT, "zk-email-verify_amd", "csrc"), os.path.join(ROOT, "tests", "native", "substrtest.cpp"),
                           "-o", str(exe)])
    for shape in st.SHAPES:
        c = _circuit(shape)
        fx = st.load_fixture(*shape)
        cfg = c.cfg
        path = tmp_path / "cases.bin"
        recs = b"".join(c.pack(inp) for _, inp, _ in fx["cases"])
        path.write_bytes(struct.pack("<10I", cfg.main_kind, cfg.max_header, cfg.max_body, cfg.n, cfg.k, 0, 0, 0, 0, 0) +
                         struct.pack("<II", len(fx["cases"]), c.in_stride) + recs)
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        assert [int(x) for x in r.stdout.split()] == [s for _, _, s in fx["cases"]], shape
