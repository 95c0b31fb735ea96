"""The transforms the prover runs (csrc/zkwg_kernels_ntt.hip) without a GPU: the per-phase bodies of the kernels (csrc/zkwg_ntt_core.h)
executed thread by thread in launch order by the host mirror (tests/native/hosttest.cpp), against the O(n log n) oracle
(oracle/pyref/ntt.py fft_fast, pinned to the O(n^2) transform) over WHOLE arrays.  The host build counts every violated range
precondition of the lazy 9 x 29-bit limb form (csrc/zkwg_fr29.h, ZKWG_FR29_CHECK): it must stay 0 after every test, including the ones
that feed each pass lazy inputs at the top of its stated contract."""
import ctypes as C
import random

import pytest

import hosttest
from oracle.pyref import ntt

P = ntt.P
R = 1 << 256
RINV = pow(R, P - 2, P)
M261 = 1 << 261


@pytest.fixture(scope="module")
def lib():
    return hosttest.load()


@pytest.fixture(autouse=True)
def no_violations(lib):
    lib.ht_fr29_reset()
    yield
    assert lib.ht_fr29_violations() == 0


def _buf(b):
    b = bytearray(b)
    return b, (C.c_char * len(b)).from_buffer(b)


def _words(vals):
    return b"".join(v.to_bytes(32, "little") for v in vals)


def _unwords(raw):
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def _family(name, n, rng):
    """input words (Montgomery form, canonical) of one polynomial"""
    if name == "uniform":
        return [rng.randrange(P) for _ in range(n)]
    if name == "top":                                 # every word r - 1: every sum path as large as it can be
        return [P - 1] * n
    if name == "alternating":                         # 0 / r - 1: the difference paths
        return [0 if i % 2 == 0 else P - 1 for i in range(n)]
    # witness-like: mostly 0 / 1, some bytes, a few full-size values (in Montgomery form)
    out = []
    for _ in range(n):
        x = rng.random()
        v = 0 if x < 0.45 else 1 if x < 0.85 else rng.randrange(256) if x < 0.97 else rng.randrange(P)
        out.append(v * R % P)
    return out


FAMILIES = ("uniform", "top", "alternating", "witness")


def test_fast_oracle_matches_the_quadratic_one():
    rng = random.Random(7)
    for power in range(2, 9):
        n = 1 << power
        x = [rng.randrange(P) for _ in range(n)]
        assert ntt.fft_fast(x) == ntt.fft(x) and ntt.ifft_fast(x) == ntt.ifft(x)
        assert ntt.ifft_fast(ntt.fft_fast(x)) == x
        m = rng.randrange(1, n + 1)
        a, b, c = ([rng.randrange(P) for _ in range(m)] for _ in range(3))
        assert ntt.h_evaluations_fast(a, b, c, power) == ntt.h_evaluations(a, b, c, power)


def test_schedule_splits_the_stages_as_documented(lib):
    out = (C.c_uint32 * 20)()
    for L in range(2, 27):
        lib.ht_ntt_sched(L, out)
        np_, ng, g_row, tile = out[0], out[1], out[2], out[3]
        gs, lb = list(out[4:4 + np_]), list(out[12:12 + np_])
        assert np_ == -(-L // 7) and ng == np_ - 1 and sum(gs) == L and max(gs) - min(gs) <= 1 and max(gs) <= 7
        assert g_row == gs[-1] and tile == min(1 << L, 1024) and (1 << g_row) <= tile
        assert lb == [L - sum(gs[:i]) for i in range(np_)]
    lib.ht_ntt_sched(20, out)
    assert list(out[4:7]) == [7, 7, 6]
    lib.ht_ntt_sched(21, out)
    assert list(out[4:7]) == [7, 7, 7]


def _transform(lib, L, polys, inverse):
    raw, cbuf = _buf(_words([v for x in polys for v in x]))
    assert lib.ht_ntt_transform(L, len(polys), 1 if inverse else 0, cbuf) == 0
    got = _unwords(bytes(raw))
    n = 1 << L
    return [got[q * n:(q + 1) * n] for q in range(len(polys))]


@pytest.mark.parametrize("power", list(range(2, 17)))
def test_mirror_transforms_equal_the_oracle_over_whole_arrays(lib, power):
    """one row pass up to 2^7; a column pass + the row pass with uneven splits (2^8 .. 2^14, tiles below 1,024 points below 2^10);
    three passes at 2^15, 2^16.  Every output word is canonical (the raw words are compared, not their residues)."""
    rng = random.Random(power)
    n = 1 << power
    fams = FAMILIES if power <= 14 else ("uniform", "top")
    polys = [_family(f, n, rng) for f in fams]
    fwd = _transform(lib, power, polys, False)
    for x, y in zip(polys, fwd):
        assert y == ntt.fft_fast(x)                     # Montgomery words: the transform is linear, so it commutes with x R
    inv = _transform(lib, power, polys, True)
    for x, y in zip(polys, inv):
        assert y == ntt.ifft_fast(x)
    assert _transform(lib, power, fwd, True) == polys   # round trip


def _abc_records(rng, fam, m, E, pad):
    stride = 96 * m + pad
    buf = bytearray(E * stride)
    vals = []
    for e in range(E):
        rows = [_family(fam, m, rng) for _ in range(3)]
        vals.append(rows)
        buf[e * stride:e * stride + 96 * m] = _words(rows[0] + rows[1] + rows[2])
    return buf, stride, vals


def _h_mirror(lib, L, buf, stride, m, E):
    n = 1 << L
    out_stride = 32 * n + 96
    out = bytearray(E * out_stride)
    ab, cab = _buf(buf)
    assert lib.ht_h_evaluations(L, cab, stride, m, E, (C.c_char * len(out)).from_buffer(out), out_stride, None) == 0
    return [_unwords(bytes(out[e * out_stride:e * out_stride + 32 * n])) for e in range(E)]


def _h_oracle_words(rows, power):
    a, b, c = ([w * RINV % P for w in r] for r in rows)
    return [v * R % P for v in ntt.h_evaluations_fast(a, b, c, power)]


@pytest.mark.parametrize("power,m,E", [(2, 3, 2), (3, 8, 1), (5, 17, 3), (7, 128, 2), (8, 200, 2), (10, 1000, 2), (11, 2048, 1), (13, 5001, 2),
                                       (14, 16384, 1), (15, 20011, 1), (16, 40000, 1)])
def test_mirror_h_evaluations_equal_the_oracle_over_whole_arrays(lib, power, m, E):
    """groth16_prove.js on the coset, m <= n rows zero-padded to the domain, E emails with padded record strides, every input family"""
    rng = random.Random(1000 + power)
    fams = FAMILIES if power <= 13 else ("uniform", "witness")
    for fam in fams:
        buf, stride, vals = _abc_records(rng, fam, m, E, 64 * (power % 3))
        got = _h_mirror(lib, power, buf, stride, m, E)
        for e in range(E):
            assert got[e] == _h_oracle_words(vals[e], power), (fam, e)


def test_mirror_h_evaluations_on_the_headline_pass_structure(lib):
    """2^20 points (passes 7 / 7 / 6): one email of witness-shaped rows, spot checks through the barycentric evaluation on the coset"""
    power, m = 20, 1000003
    n = 1 << power
    rng = random.Random(20)
    vals = []
    for _ in range(3):
        row = [0] * m
        for i in rng.sample(range(m), 300):
            row[i] = rng.randrange(P) if rng.random() < 0.3 else rng.randrange(1, 256)
        vals.append(row)
    buf = bytearray(96 * m)
    for j, row in enumerate(vals):
        for i, v in enumerate(row):
            if v:
                buf[32 * (j * m + i):32 * (j * m + i + 1)] = (v * R % P).to_bytes(32, "little")
    got = _h_mirror(lib, power, buf, 96 * m, m, 1)[0]
    assert all(w < P for w in got)
    for k in (0, n // 2 + 3, n - 1):
        want = (ntt.coset_eval_direct(vals[0], power, k) * ntt.coset_eval_direct(vals[1], power, k) - ntt.coset_eval_direct(vals[2], power, k)) % P
        assert got[k] * RINV % P == want, k


# ---- lazy inputs at the top of each pass's stated contract ------------------------------------------------------------------------------
def _limbs(v, U):
    """limb form of the integer v with limbs 0 .. 7 in [(U - 1) 2^29 - U + 1, U 2^29): the widest limbs a [U, .] operand may have"""
    n = [(v >> (29 * i)) & (2 ** 29 - 1) for i in range(8)] + [v >> 232]
    d = U - 1
    out = [n[0] + (d << 29)] + [n[i] + (d << 29) - d for i in range(1, 8)] + [n[8] - d]
    assert all(0 <= x < 2 ** 32 for x in out) and sum(x << (29 * i) for i, x in enumerate(out)) == v
    return out


def _planar(elems, n):
    """planar work-buffer layout of one polynomial (limbs 0-3 | limbs 4-7 | top, 16 + 16 + 4 bytes per element)"""
    lo = b"".join(b"".join(x.to_bytes(4, "little") for x in e[0:4]) for e in elems)
    hi = b"".join(b"".join(x.to_bytes(4, "little") for x in e[4:8]) for e in elems)
    top = b"".join(e[8].to_bytes(4, "little") for e in elems)
    return lo + hi + top


def _unplanar(raw, n, polys):
    out = []
    for q in range(polys):
        p = raw[q * 36 * n:(q + 1) * 36 * n]
        for i in range(n):
            l = [int.from_bytes(p[16 * i + 4 * k:16 * i + 4 * k + 4], "little") for k in range(4)]
            l += [int.from_bytes(p[16 * n + 16 * i + 4 * k:16 * n + 16 * i + 4 * k + 4], "little") for k in range(4)]
            l.append(int.from_bytes(p[32 * n + 4 * i:32 * n + 4 * i + 4], "little"))
            out.append(sum(x << (29 * j) for j, x in enumerate(l)))
    return out


def _run_pass(lib, kind, dit, L, i, inv, scale, uni, elems_per_poly):
    n = 1 << L
    raw, cbuf = _buf(b"".join(_planar(e, n) for e in elems_per_poly))
    assert lib.ht_ntt_pass(kind, dit, L, i, inv, scale, uni, len(elems_per_poly), cbuf, None) == 0
    return _unplanar(bytes(raw), n, len(elems_per_poly))


# (kind, dit, L, pass, inverse roots, scale, 1 / n, input limb width U, input value bound V): what the pipeline feeds each pass
CONTRACTS = [
    (0, 0, 15, 1, 1, 0, 0, 1, 5),      # DIF column pass after a column pass: [1, 5]
    (0, 0, 9, 0, 1, 0, 0, 1, 5),
    (1, 0, 14, 0, 1, 1, 0, 1, 5),      # DIF row pass after a column pass, times the coset / 1 / n table
    (1, 0, 9, 0, 0, 0, 1, 1, 5),
    (1, 1, 14, 0, 0, 0, 0, 1, 5),      # DIT row pass on the inverse transforms' output: [1, 5]
    (1, 1, 6, 0, 0, 0, 0, 1, 5),
    (0, 1, 14, 0, 0, 0, 0, 6, 30),     # DIT column pass: limbs < 6 2^29, value < 30 r
    (0, 1, 15, 1, 0, 0, 0, 6, 30),
    (0, 1, 15, 0, 0, 0, 0, 6, 30),
]


@pytest.mark.parametrize("kind,dit,L,i,inv,scale,uni,U,V", CONTRACTS)
def test_each_pass_holds_its_bounds_on_lazy_inputs_at_the_top_of_its_contract(lib, kind, dit, L, i, inv, scale, uni, U, V):
    """value + k r with the largest k the contract allows, limbs at the largest U: the pass must compute the same residues as on the
    reduced inputs, and no precondition may break on the way (the checker counts)"""
    rng = random.Random(L * 100 + kind * 10 + dit)
    n = 1 << L
    polys = [_family(f, n, rng) for f in (FAMILIES if L < 15 else ("uniform", "top"))]
    lazy = []
    for q, x in enumerate(polys):
        # the largest representative below V r (value + (V - 1) r) for two elements in three, value + k r, 1 <= k < V - 1, between
        lazy.append([_limbs(v + ((V - 1) if (q + j) % 3 else 1 + j % (V - 1)) * P, U) for j, v in enumerate(x)])
    canon = [[_limbs(v, 1) for v in x] for x in polys]
    got_lazy = _run_pass(lib, kind, dit, L, i, inv, scale, uni, lazy)
    got_canon = _run_pass(lib, kind, dit, L, i, inv, scale, uni, canon)
    assert [v % P for v in got_lazy] == [v % P for v in got_canon]
    assert max(got_lazy) < 30 * P                       # what the next pass / the join accepts


def test_lazy_work_buffer_through_a_whole_forward_transform(lib):
    """the pipeline's forward transforms read the limb-form work buffer (values < 5 r): the full transform from inputs at that bound
    equals the oracle's over the whole array"""
    for L in (7, 13, 16):
        n = 1 << L
        rng = random.Random(L)
        polys = [_family(f, n, rng) for f in ("uniform", "top")]
        # bit-reversed input order (what the inverse transforms leave), values + 4 r
        elems = [[_limbs(x[ntt_bitrev(j, L)] + 4 * P, 1) for j in range(n)] for x in polys]
        raw, cbuf = _buf(b"".join(_planar(e, n) for e in elems))
        out = bytearray(32 * n * len(polys))
        # DIT: row pass, then the column passes in reverse; the last one writes canonical words
        sched = (C.c_uint32 * 20)()
        lib.ht_ntt_sched(L, sched)
        ng = sched[1]
        cout = (C.c_char * len(out)).from_buffer(out)
        assert lib.ht_ntt_pass(1, 1, L, 0, 0, 0, 0, len(polys), cbuf, cout if ng == 0 else None) == 0
        for i in range(ng - 1, -1, -1):
            assert lib.ht_ntt_pass(0, 1, L, i, 0, 0, 0, len(polys), cbuf, cout if i == 0 else None) == 0
        got = _unwords(bytes(out))
        for q, x in enumerate(polys):
            assert got[q * n:(q + 1) * n] == ntt.fft_fast(x), (L, q)


def ntt_bitrev(j, L):
    return int(format(j, "0%db" % L)[::-1], 2)


# ---- the join --------------------------------------------------------------------------------------------------------------------------
def _mul29(x, y):
    """the value fr29_mul returns (exact: q = -x y r^-1 mod 2^261)"""
    q = (-x * y * pow(P, -1, M261)) % M261
    return (x * y + q * P) // M261


def _join(lib, a, b, c):
    out = C.create_string_buffer(32)
    arr = lambda v: (C.c_uint32 * 9)(*v)
    lib.ht_ntt_join(arr(a), arr(b), arr(c), out)
    return int.from_bytes(out.raw, "little")


def test_join_emits_canonical_words_at_its_contract_boundary(lib):
    """a, b < 30 r, c = 0 (inside the join's contract: limb-form values below 30 r): when mul(mul(a, b), 2^266) lands in [r, 1.04 r),
    ab - c + 31 r is at least 32 r -- a conversion for values below 32 r emitted a word >= r there"""
    rng = random.Random(266)
    k266 = pow(2, 266, P)
    found = []
    while len(found) < 4:
        a, b = rng.randrange(30 * P), rng.randrange(30 * P)
        if _mul29(_mul29(a, b), k266) >= P:
            found.append((a, b))
    found.append((30 * P - 1, 30 * P - 1))
    for a, b in found:
        for c in (0, 1, P - 1, 30 * P - 1):
            got = _join(lib, _limbs(a, 1), _limbs(b, 1), _limbs(c, 1))
            assert got < P and got == (a * b * RINV - c) % P, (a, b, c)


def test_join_on_random_lazy_inputs(lib):
    rng = random.Random(5)
    for _ in range(3000):
        a, b, c = (rng.randrange(30 * P) for _ in range(3))
        got = _join(lib, _limbs(a, rng.randrange(1, 4)), _limbs(b, 1), _limbs(c, rng.randrange(1, 4)))
        assert got < P and got == (a * b * RINV - c) % P


# ---- the checker counts -----------------------------------------------------------------------------------------------------------------
def test_the_range_checker_is_not_vacuous(lib):
    arr = lambda v: (C.c_uint32 * 9)(*v)
    out = (C.c_uint32 * 9)()
    lib.ht_fr29_op(0, arr(_limbs(31 * P + 5, 1)), arr([0] * 9), out)         # inside: < 32 r
    lib.ht_fr29_op(1, arr(_limbs(7, 1)), arr(_limbs(3 * P - 1, 1)), out)     # inside: b <= 3 r
    assert lib.ht_fr29_violations() == 0
    lib.ht_fr29_op(0, arr(_limbs(32 * P + 5, 1)), arr([0] * 9), out)         # fr29_to_fr_v<32> of a value >= 32 r
    n1 = lib.ht_fr29_violations()
    assert n1 > 0
    lib.ht_fr29_op(1, arr(_limbs(7, 1)), arr(_limbs(3 * P + 12345, 1)), out)  # fr29_sub<4, 1>: subtrahend above 3 r
    n2 = lib.ht_fr29_violations()
    assert n2 > n1
    lib.ht_fr29_op(1, arr(_limbs(7, 1)), arr(_limbs(P, 3)), out)              # limbs wider than the constant's
    n3 = lib.ht_fr29_violations()
    assert n3 > n2
    lib.ht_fr29_op(2, arr([2 ** 32 - 1] * 9), arr([2 ** 32 - 1] * 9), out)    # product columns past 2^64
    n4 = lib.ht_fr29_violations()
    assert n4 > n3
    lib.ht_fr29_op(3, arr([2 ** 32 - 1] * 9), arr([0] * 9), out)              # normalisation wraps a limb
    assert lib.ht_fr29_violations() > n4
    lib.ht_fr29_reset()
