"""The host core of the prover of witnesses (csrc/zkwg_zkey_core.h through tests/native/zkeytest.cpp; no GPU): the row evaluation that
zk_zkey_abc runs -- same function, host build, every limb-form bound counted (ZKWG_FR29_CHECK) -- against oracle.pyref.groth16.abc_rows,
the bound cases of the lazy accumulation, and the zkey / .wtns readers.  All comparisons are of integers mod r, exact.
Reference call site: snarkjs.groth16.prove(zkey, wtns), packages/helpers/src/chunked-zkey.ts:80-84."""
import ctypes as C
import struct

import pytest

import zkeytest
from oracle.pyref import groth16 as G
from zkeytest import R

BAD_CONFIG = -1


def _abc(lib, z, wits, n_vars, n_rows):
    out = (C.c_uint8 * (96 * n_rows * len(wits)))()
    raw = b"".join(zkeytest.wit_bytes(w) for w in wits)
    assert lib.zt_abc(z, len(z), raw, 32 * n_vars, len(wits), out, 96 * n_rows) == 0
    return [zkeytest.abc_ints(bytes(out)[96 * n_rows * e:96 * n_rows * (e + 1)], n_rows) for e in range(len(wits))]


def test_row_evaluation_equals_the_oracle_on_a_random_system():
    lib = zkeytest.load()
    n_public = 5
    n_wires, cons, w = zkeytest.random_system(seed=7, n_public=n_public)
    lens = sorted(len(a) + len(b) for a, b, _ in cons)
    thr = lib.zt_long_threshold()
    assert thr in lens and thr + 1 in lens and lens[-1] >= 4096 and {1, 2, 63, 64, 65} <= {len(a) for a, _, _ in cons}
    n_rows = len(cons) + n_public + 1
    key = zkeytest.StubKey(n_public, 1 << G.domain_power(len(cons), n_public))
    z = zkeytest.dummy_zkey(n_wires, n_public, key.n, zkeytest.section4(cons, n_public))
    info = (C.c_uint64 * 4)()
    assert lib.zt_zkey_check(z, len(z), info) == 0 and list(info)[:3] == [n_wires, n_public, n_rows]
    assert 0 < info[3] < len(cons)                       # both kernels' splits are exercised
    # the satisfying witness, and one with a wire changed (a constraint fails: the rows are evaluated all the same)
    w2 = list(w)
    w2[n_wires // 2] = (w2[n_wires // 2] + 1) % R
    v0 = lib.zt_violations()
    for wit, (a, b, c) in zip((w, w2), _abc(lib, z, [w, w2], n_wires, n_rows)):
        A, B, Cc = G.abc_rows(key, cons, wit)
        assert a == A[:n_rows] and b == B[:n_rows] and c == Cc[:n_rows]
    assert all(x * y % R == w[len(w) - len(cons) + k] for k, (x, y) in enumerate(zip(*_abc(lib, z, [w], n_wires, n_rows)[0][:2])) if k < len(cons))
    assert lib.zt_violations() == v0 == 0


@pytest.mark.parametrize("pattern", ["all_minus_one", "alternating", "generic"])
def test_a_row_of_the_maximum_length_stays_inside_the_bounds(pattern):
    """one row of ZK_ZKEY_MAX_ROW terms, the longest creation accepts, every witness value r - 1: coefficients all r - 1, alternating
    r - 1 / 1 (the unit-term blocks at their bounds), and all r - 2 (every term a product: the column accumulators at theirs; this case is
    beyond what the issue lists)"""
    lib = zkeytest.load()
    n, n_vars = lib.zt_max_row(), 8
    coef = {"all_minus_one": lambda t: R - 1, "alternating": lambda t: R - 1 if t % 2 == 0 else 1, "generic": lambda t: R - 2}[pattern]
    coeffs = [(0, 0, t % n_vars, coef(t)) for t in range(n)] + [(1, 0, 1, 1)]
    z = zkeytest.dummy_zkey(n_vars, 2, 4, coeffs)
    w = [R - 1] * n_vars
    v0 = lib.zt_violations()
    (a, b, c), = _abc(lib, z, [w], n_vars, 1)
    want = sum(coef(t) for t in range(n)) * (R - 1) % R
    assert a == [want] and b == [R - 1] and c == [want * (R - 1) % R]
    assert lib.zt_violations() == v0 == 0
    # one term more is refused
    z = zkeytest.dummy_zkey(n_vars, 2, 4, coeffs + [(0, 0, 0, 1)])
    assert lib.zt_zkey_check(z, len(z), None) == BAD_CONFIG


def test_values_that_are_not_reduced_keep_the_bounds():
    """a witness value >= r is reported (zk_zkey_range) and its witness gets no proof, but the evaluation neither drops the term nor leaves
    its bounds: 64 values of 2^256 - 1 in one block, all added resp. all subtracted"""
    lib = zkeytest.load()
    big = (1 << 256) - 1
    # (the last coefficient is stored in the table as 2^253 - 1: every limb of both operands of every product is at its maximum, the
    # input that overflows a column when one product too many is accumulated between two carries)
    for c0 in (1, R - 1, 5, ((1 << 253) - 1) * pow(1 << 517, -1, R) % R):
        w = [1, big, 0]
        assert lib.zt_range_ok(zkeytest.wit_bytes(w), 3) == 0 and lib.zt_range_ok(zkeytest.wit_bytes([1, R - 1, 0]), 3) == 1
        for terms in (62, 64 * 130):               # one lane (a full block and a short one), 64 lanes of 130 terms
            z = zkeytest.dummy_zkey(3, 1, 2, [(0, 0, 1, c0)] * terms + [(1, 0, 0, 1)])
            v0 = lib.zt_violations()
            (a, b, c), = _abc(lib, z, [w], 3, 1)
            assert a == [terms * c0 * big % R] and b == [1] and lib.zt_violations() == v0 == 0, (c0, terms)


def _sections(z):
    pos, out = 12, {}
    for _ in range(struct.unpack_from("<I", z, 8)[0]):
        sid, size = struct.unpack_from("<IQ", z, pos)
        out[sid] = (pos + 12, size)
        pos += 12 + size
    return out


def test_zkey_reader_round_trips_and_refuses_bad_files():
    from zkwg import zkey
    lib = zkeytest.load()
    n_vars, n_public, domain = 12, 3, 16
    coeffs = [(0, 0, 1, 5), (1, 0, 2, R - 1), (0, 1, 4, 1), (1, 1, 11, 7)] + [(0, 2 + s, s, 1) for s in range(n_public + 1)]
    good = zkeytest.dummy_zkey(n_vars, n_public, domain, coeffs)
    assert zkey.read_zkey(good)["coeffs"] == coeffs
    info = (C.c_uint64 * 4)()
    assert lib.zt_zkey_check(good, len(good), info) == 0 and list(info) == [12, 3, 6, 0]
    sec = _sections(good)
    check = lambda z: lib.zt_zkey_check(bytes(z), len(z), None)
    # section 1 of 0 .. 3 bytes as the LAST section of the buffer (nothing to read behind it)
    body = lambda sid: good[sec[sid][0] - 12:sec[sid][0] + sec[sid][1]]
    for k in range(4):
        z = good[:8] + struct.pack("<I", 10) + b"".join(body(s) for s in range(2, 11)) + struct.pack("<IQ", 1, k) + bytes([1, 0, 0, 0][:k])
        assert check(z) == BAD_CONFIG, k
    h = sec[2][0]
    z = bytearray(good)
    struct.pack_into("<I", z, h + 76, 0xFFFFFFFF)                      # nPublic + 1 wraps in 32 bits
    assert check(z) == BAD_CONFIG
    z = bytearray(good)
    struct.pack_into("<Q", z, sec[9][0] - 8, sec[9][1] + (1 << 40))   # a section length past the end
    assert check(z) == BAD_CONFIG
    assert check(good[:-70]) == BAD_CONFIG
    for bad in ((0, 0, n_vars, 1), (0, domain, 1, 1), (2, 0, 1, 1)):  # wire = nVars, row = domain, a third matrix
        z = zkeytest.dummy_zkey(n_vars, n_public, domain, coeffs + [bad])
        assert check(z) == BAD_CONFIG, bad
    z = bytearray(good)
    z[sec[4][0] + 4 + 12:sec[4][0] + 4 + 44] = R.to_bytes(32, "little")   # a stored coefficient = r
    assert check(z) == BAD_CONFIG
    z = bytearray(good)
    z[sec[6][0] + 64 * 5] = 1                                          # B1[5] no longer at infinity, B2[5] still is
    assert check(z) == BAD_CONFIG
    z[sec[7][0] + 128 * 5 + 3] = 9
    assert check(z) == 0
    assert check(b"zkex" + good[4:]) == BAD_CONFIG and check(good[:11]) == BAD_CONFIG and check(b"") == BAD_CONFIG


def test_wtns_reader():
    lib = zkeytest.load()
    n = 12
    vals = zkeytest.wit_bytes(range(1, n + 1))
    s1 = struct.pack("<I", 32) + R.to_bytes(32, "little") + struct.pack("<I", n)
    mk = lambda secs, magic=b"wtns", version=2: magic + struct.pack("<II", version, len(secs)) + b"".join(struct.pack("<IQ", i, len(p)) + p for i, p in secs)
    nw, off = C.c_uint64(), C.c_uint64()
    parse = lambda f: lib.zt_wtns_parse(f, len(f), C.byref(nw), C.byref(off))
    for f in (mk([(1, s1), (2, vals)]), mk([(2, vals), (1, s1)]), mk([(7, b"xyz"), (2, vals), (1, s1)])):      # sections in either order
        assert parse(f) == 0 and nw.value == n and f[off.value:off.value + 32 * n] == vals
    good = mk([(1, s1), (2, vals)])
    assert parse(mk([(1, s1), (2, vals)], magic=b"wtnz")) == BAD_CONFIG
    assert parse(mk([(1, s1), (2, vals)], version=1)) == BAD_CONFIG
    assert parse(mk([(1, struct.pack("<I", 32) + (R + 2).to_bytes(32, "little") + struct.pack("<I", n)), (2, vals)])) == BAD_CONFIG
    assert parse(mk([(1, s1), (2, vals[:-32])])) == BAD_CONFIG            # nWitness does not match section 2
    assert parse(good[:-5]) == BAD_CONFIG and parse(good[:30]) == BAD_CONFIG and parse(mk([(1, s1)])) == BAD_CONFIG
    # nWitness != the key's nVars is the prover's check (zkwg.prover.WitnessProver: tests/test_prove_wtns.py runs it on the device
    # path too); here through the Python reader
    from zkwg import wtns
    assert wtns.read_wtns(good) == (n, vals)
    with pytest.raises(ValueError):
        wtns.read_wtns(good, n_vars=n + 1)
    with pytest.raises(ValueError):
        wtns.read_wtns(good[:-5])


def test_the_library_exports_the_witness_prover():
    import os
    import re
    from conftest import ROOT
    from zkwg import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "zkwg.h")).read()
    for name in ("zkwg_prover_create_wtns", "zkwg_prover_witness_len", "zkwg_prover_num_public", "zkwg_prover_prove_witnesses",
                 "zkwg_prover_prove_witnesses_device", "zkwg_prover_abc_device", "zkwg_wtns_parse", "zkwg_zkey_check"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.zkwg_abi_version() == 3
    assert b"field order" in lib.zkwg_strerror(7) and "ZKWG_ERR_WITNESS_NOT_REDUCED = 7" in hdr
    # the product's own readers (no device needed) agree with the host build of the core
    z = zkeytest.dummy_zkey(6, 1, 4, [(0, 0, 1, 1), (1, 0, 2, 3), (0, 1, 0, 1), (0, 2, 1, 1)])
    nv, npub, nr = C.c_uint64(), C.c_uint32(), C.c_uint64()
    assert lib.zkwg_zkey_check(z, len(z), C.byref(nv), C.byref(npub), C.byref(nr)) == 0 and (nv.value, npub.value, nr.value) == (6, 1, 3)
    assert lib.zkwg_zkey_check(z[:-1], len(z) - 1, None, None, None) == BAD_CONFIG
    # the witness entry points refuse a missing prover
    assert lib.zkwg_prover_prove_witnesses(None, b"", 0, 0, b"", None, None) == -2
