"""The bound checker of csrc/zkwg_fq29.h.  Under ZKWG_FQ29_CHECK a limb-form value carries upper bounds beside its limbs, every fq29_*
operation checks its preconditions against the operands' BOUNDS and derives the result's by the rules of the header, and ZKQ29_CLAIM widens
a value to its stated contract: one execution of a straight-line formula then proves it for every input.  Here: the checker is not vacuous
(tiny values, bounds that break a rule), it is sound and as tight as the header's rules at operands placed AT their bounds, and every point
formula and every piece of the Miller loop runs once from the top of its contract with all three counters at zero and the oracle's result."""
import ctypes as C
import random
from fractions import Fraction

import pytest

import hosttest
import pairtest
from oracle.pyref import bn254_g1 as G
from oracle.pyref import bn254_g2 as H
from oracle.pyref import bn254_pairing as P

Q = G.Q
RINV = pow(1 << 261, -1, Q)
MUL, SQR, DOT2, ADD, NORM, SUB_2_1, SUB_3_1, SUB_5_2, SUB_12_1, SUB_8_1, TOFQ_2, TOFQ_3, TOFQ_16, SUM_NORM = range(14)
SUBS = {SUB_2_1: (2, 1), SUB_3_1: (3, 1), SUB_5_2: (5, 2), SUB_12_1: (12, 1), SUB_8_1: (8, 1)}


@pytest.fixture(scope="module")
def lib():
    lib = hosttest.load()
    lib.ht_fq29_counters.restype = None
    lib.ht_fq29_counters.argtypes = [C.c_void_p]
    lib.ht_fq29_counters_set.restype = None
    lib.ht_fq29_counters_set.argtypes = [C.c_void_p]
    lib.ht_fq29_bound_op.restype = None
    lib.ht_fq29_bound_op.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ht_ec29_g1_op.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_char_p]
    lib.ht_ec29_g2_op.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_char_p]
    return lib


def _counters(lib):
    out = (C.c_ulonglong * 3)()
    lib.ht_fq29_counters(out)
    return tuple(out)


def _limbs(v):
    """plain limbs of v < 2^261"""
    return [(v >> (29 * i)) & ((1 << 29) - 1) for i in range(8)] + [v >> 232]


def _value(l):
    return sum(x << (29 * i) for i, x in enumerate(l))


def _op(lib, op, operands, claims, reps=0):
    """operands: up to 4 lists of 9 limbs; claims: (U, V) or None each -> (result limbs, its limb bounds, its value bound as a multiple of q)"""
    ops = list(operands) + [[0] * 9] * (4 - len(operands))
    cl = [c or (0, 0) for c in claims] + [(0, 0)] * (4 - len(claims))
    a = (C.c_uint32 * 36)(*[x for l in ops for x in l])
    c = (C.c_uint32 * 8)(*[x for uv in cl for x in uv])
    out, sh = (C.c_uint32 * 9)(), (C.c_ulonglong * 10)()
    lib.ht_fq29_bound_op(op, reps, a, c, out, sh)
    return list(out), list(sh[:9]), Fraction(sh[9], 1 << 20)


# ---- the checker is not vacuous -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,op,operands,claims,reps", [
    ("8 x [1, 1] summed, then norm: limbs [8, *] can wrap with the carry", SUM_NORM, [_limbs(1)], [(1, 1)], 8),
    ("sub<2, 1> of a subtrahend claimed [1, 2]: 2 q does not dominate it", SUB_2_1, [_limbs(5), _limbs(3)], [(1, 1), (1, 2)], 0),
    ("mul of [3, 1] x [3, 1]: 9 x 9 x 2^58 passes the accumulator", MUL, [_limbs(2), _limbs(3)], [(3, 1), (3, 1)], 0),
    ("to_fq<2> of a value claimed [1, 3]", TOFQ_2, [_limbs(7)], [(1, 3)], 0),
])
def test_the_bound_checker_is_not_vacuous(lib, name, op, operands, claims, reps):
    """the actual values are tiny, so the value counter stays where it is; the BOUNDS break a rule, so the bound counter rises (the mirror of
    test_the_range_checker_is_not_vacuous in tests/test_ntt_cpu.py)"""
    before = _counters(lib)
    _op(lib, op, operands, claims, reps)
    after = _counters(lib)
    assert after[0] == before[0] and after[2] == before[2], name
    assert after[1] > before[1], name
    # the same calls with bounds inside the rules leave every counter alone
    ok = {SUM_NORM: ([(1, 1)], 7), SUB_2_1: ([(1, 1), (1, 1)], 0), MUL: ([(3, 1), (2, 1)], 0), TOFQ_2: ([(1, 2)], 0)}[op]
    _op(lib, op, operands, ok[0], ok[1])
    assert _counters(lib) == after, name
    lib.ht_fq29_counters_set((C.c_ulonglong * 3)(*before))          # the violations made on purpose are not this library's findings


# ---- sound, and as tight as the header's rules, at operands placed AT their bounds -----------------------------------------------------------
def _at_bounds(rng, U, V):
    """limbs of a value inside [U, V] with limbs 0 .. 6 at U 2^29 - 1 or a little below, and limbs 7, 8 as large as value < V q allows"""
    l = [(U << 29) - 1 - (rng.randrange(8) if rng.random() < 0.5 else 0) for _ in range(7)]
    rest = V * Q - 1 - _value(l)
    l8 = rest >> 232
    l7 = min((rest - (l8 << 232)) >> 203, (U << 29) - 1)
    l += [l7, l8]
    assert _value(l) < V * Q and l8 < 1 << 32
    return l


def _cases(rng, op):
    """-> (operand claims, the header's [U, V] of the result, the expected value mod q as a function of the operand values)"""
    if op == MUL:
        ua, ub = rng.choice([(1, 1), (1, 6), (6, 1), (2, 3), (3, 2), (2, 2), (1, 3)])
        va = rng.randrange(1, 170)
        vb = rng.randrange(1, 169 // va + 1)
        return [(ua, va), (ub, vb)], (1, Fraction(va * vb, 169) + 1), lambda a, b: a * b * RINV
    if op == SQR:
        u, v = rng.choice([1, 2]), rng.randrange(1, 14)
        return [(u, v)], (1, Fraction(v * v, 169) + 1), lambda a: a * a * RINV
    if op == DOT2:
        ua, ub, uc, ud = rng.choice([(1, 1, 1, 1), (2, 2, 1, 2), (1, 3, 1, 3), (1, 5, 1, 1), (3, 1, 1, 3), (1, 2, 2, 2)])
        va, vc = rng.randrange(1, 15), rng.randrange(1, 15)
        vb, vd = rng.randrange(1, 16), rng.randrange(1, 16)
        return [(ua, va), (ub, vb), (uc, vc), (ud, vd)], (1, Fraction(va * vb + vc * vd, 169) + 1), lambda a, b, c, d: (a * b + c * d) * RINV
    if op == ADD:
        ua = rng.randrange(1, 8)
        ub = rng.randrange(1, 9 - ua)
        va, vb = rng.randrange(1, 80), rng.randrange(1, 80)
        return [(ua, va), (ub, vb)], (ua + ub, va + vb), lambda a, b: a + b
    if op == NORM:
        u, v = rng.randrange(1, 8), rng.randrange(1, 170)
        return [(u, v)], (1, v), lambda a: a
    if op in SUBS:
        M, U = SUBS[op]
        ua, va = rng.randrange(1, 8 - U - 1 + 1), rng.randrange(1, 100)
        return [(ua, va), (U, M - 1)], (ua + U + 1, va + M), lambda a, b: a - b
    # the canonical words come back through fq29_from_fq, whose bounds are those of ANY 256-bit word: limbs < 2^29, the top one < 2^24, value
    # < 2^256 (in units of q / 2^20, rounded up); that the words are below q is asserted on the value itself
    V = {TOFQ_2: 2, TOFQ_3: 3, TOFQ_16: 16}[op]
    return [(rng.randrange(1, 8), V)], (1, Fraction(1 << 256, Q) + Fraction(2, 1 << 20)), lambda a: a


@pytest.mark.parametrize("op", [MUL, SQR, DOT2, ADD, NORM, SUB_2_1, SUB_3_1, SUB_5_2, SUB_12_1, SUB_8_1, TOFQ_2, TOFQ_3, TOFQ_16],
                         ids=["mul", "sqr", "dot2", "add", "norm", "sub<2,1>", "sub<3,1>", "sub<5,2>", "sub<12,1>", "sub<8,1>", "to_fq<2>", "to_fq<3>", "to_fq<16>"])
def test_the_bounds_are_sound_and_inside_the_headers_rules_at_operands_on_their_bounds(lib, op):
    rng = random.Random(2900 + op)
    before = _counters(lib)
    for k in range(2000):
        claims, (ru, rv), want = _cases(rng, op)
        operands = [_at_bounds(rng, u, v) for u, v in claims]
        got, ub, vb = _op(lib, op, operands, claims)
        assert _value(got) % Q == want(*[_value(l) for l in operands]) % Q, (op, k, claims)
        assert all(got[i] < ub[i] for i in range(9)) and _value(got) <= vb * Q, (op, k, claims)
        assert all(b <= ru << 29 for b in ub[:8]) and vb <= rv, (op, k, claims, ub, float(vb), ru, float(rv))
        if op in (TOFQ_2, TOFQ_3, TOFQ_16):
            assert _value(got) < Q and ub[8] <= 1 << 24
    assert _counters(lib) == before          # no precondition violated, by value or by bound, and no result above its bounds


# ---- every formula from the top of its contract ------------------------------------------------------------------------------------------------
def _b(x):
    return int(x).to_bytes(32, "little")


def _pt(p):
    return bytes(64) if p is None else _b(p[0]) + _b(p[1])


def _unpt(b):
    x, y = int.from_bytes(b[:32], "little"), int.from_bytes(b[32:64], "little")
    return None if x == 0 and y == 0 else (x, y)


def _p2(p):
    return bytes(128) if p is None else _b(p[0][0]) + _b(p[0][1]) + _b(p[1][0]) + _b(p[1][1])


def _unp2(b):
    v = [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(4)]
    return None if not any(v) else ((v[0], v[1]), (v[2], v[3]))


def test_every_point_formula_from_the_top_of_its_contract(lib):
    """ec29_add_mixed, ec29_add, ec29_dbl_affine, ec29_dbl claim the Xyzz29 / Aff29 contract on their operands, which WIDENS the bounds to it:
    each call below is the formula at X [1, 11], Y [1, 7] (G1 [1, 2]), ZZ, ZZZ [1, 2], x [1, 1], y [2, 2], in every branch"""
    rng = random.Random(2950)
    p, q = G.random_points(2, 2951)
    p2, q2 = H.random_points(2, 2952)
    before = _counters(lib)
    out = C.create_string_buffer(64)
    for a, b in ((p, q), (p, p), (p, G.neg(p)), (p, None), (None, q), (None, None)):      # generic, equal, opposite, infinity on either side
        s = _b(rng.randrange(1, Q))
        for op in (0, 1):
            lib.ht_ec29_g1_op(op, _pt(a), _pt(b), s, 1, out)
            assert _unpt(out.raw) == G.add(a, b), (op, a, b)
        for op in (2, 3):
            lib.ht_ec29_g1_op(op, _pt(a), _pt(b), s, 1, out)
            assert _unpt(out.raw) == G.add(a, a), (op, a)
    out = C.create_string_buffer(128)
    for a, b in ((p2, q2), (p2, p2), (p2, H.neg(p2)), (p2, None), (None, q2), (None, None)):
        s = _b(rng.randrange(1, Q)) + _b(rng.randrange(Q))
        for op in (0, 1):
            lib.ht_ec29_g2_op(op, _p2(a), _p2(b), s, 1, out)
            assert _unp2(out.raw) == H.add(a, b), (op, a, b)
        for op in (2, 3):
            lib.ht_ec29_g2_op(op, _p2(a), _p2(b), s, 1, out)
            assert _unp2(out.raw) == H.add(a, a), (op, a)
    assert _counters(lib) == before


def _f2s(v):
    return [tuple(v[i:i + 2]) for i in range(0, len(v), 2)]


def _flat(*f2):
    return [c for x in f2 for c in x]


def test_every_piece_of_the_miller_loop_from_the_top_of_its_contract():
    """one zk_pair_dbl_step, one zk_pair_add_step, one zk_f12_sqr, one zk_f12_mul_line with a tangent and one with a chord, one zk_f12_mul:
    each widens its operands to its entry claims; the results are the formulas of csrc/zkwg_pair_core.h on Python integers, and T is the
    oracle's point"""
    rng = random.Random(2960)
    m, a, s, n = H.f2_mul, H.f2_add, H.f2_sub, H.f2_neg
    t_aff, q_aff = H.random_points(2, 2961)
    z = (rng.randrange(1, Q), rng.randrange(Q))
    zz, zzz = m(z, z), m(m(z, z), z)
    X, Y = m(t_aff[0], zz), m(t_aff[1], zzz)
    xP, yP = G.random_points(1, 2962)[0]
    before = pairtest.counters()
    # the doubling step
    got = _f2s(pairtest.pair_piece(0, _flat(X, Y, zz, zzz) + [yP, xP], 14))
    U = a(Y, Y); V = m(U, U); W = m(U, V); S = m(X, V); X2 = m(X, X); M = a(a(X2, X2), X2)
    X3 = s(m(M, M), a(S, S)); Y3 = s(m(M, s(S, X3)), m(W, Y))
    tangent = [m(m(U, zzz), H.f2(2 * yP % Q)), m(m(M, zz), H.f2(-2 * xP % Q)), s(a(m(M, X), m(M, X)), V)]
    assert got == [X3, Y3, m(V, zz), m(W, zzz)] + tangent
    zi = H.f2_inv(got[2]); zi3 = H.f2_inv(got[3])
    assert (m(got[0], zi), m(got[1], zi3)) == H.add(t_aff, t_aff)
    # the addition step
    x2, y2 = q_aff
    got = _f2s(pairtest.pair_piece(1, _flat(X, Y, zz, zzz, x2, y2) + [yP, xP], 14))
    Pp = s(m(x2, zz), X); R = s(m(y2, zzz), Y); D = m(Pp, zzz); E = m(R, zz); PP = m(Pp, Pp); Qq = m(X, PP); PPP = m(Pp, PP)
    X3 = s(s(m(R, R), PPP), a(Qq, Qq)); Y3 = s(m(R, s(Qq, X3)), m(Y, PPP))
    chord = [m(D, H.f2(yP)), m(E, H.f2(-xP % Q)), s(m(E, x2), m(D, y2))]
    assert got == [X3, Y3, m(zz, PP), m(zzz, PPP)] + chord
    assert (m(got[0], H.f2_inv(got[2])), m(got[1], H.f2_inv(got[3]))) == H.add(t_aff, q_aff)
    # the Fq12 pieces
    f = tuple((rng.randrange(Q), rng.randrange(Q)) for _ in range(6))
    g = tuple((rng.randrange(Q), rng.randrange(Q)) for _ in range(6))
    flat12 = lambda x: [c for k in x for c in k]
    assert tuple(_f2s(pairtest.pair_piece(2, flat12(f), 12))) == P.f12_mul(f, f)
    for line in (tangent, chord):
        sparse = (line[0], line[1], (0, 0), line[2], (0, 0), (0, 0))
        assert tuple(_f2s(pairtest.pair_piece(3, flat12(f) + _flat(*line), 12))) == P.f12_mul(f, sparse)
    assert tuple(_f2s(pairtest.pair_piece(4, flat12(f) + flat12(g), 12))) == P.f12_mul(f, g)
    assert pairtest.counters() == before


def test_no_counter_moved_in_either_library(lib):
    assert pairtest.counters() == (0, 0, 0) and _counters(lib) == (0, 0, 0)
