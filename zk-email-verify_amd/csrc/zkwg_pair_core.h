// One Miller loop of the BN254 optimal ate pairing per LANE PAIR: the per-pair body of batched groth16 verification, shared by the kernels
// (csrc/zkwg_kernels_pair.hip) and by the host build of the CPU tests (tests/native/pairtest.cpp, ZKWG_FQ29_CHECK counting every violated
// limb-form bound).  The host pairing (csrc/zkwg_pairing.h: affine lines, one Fq2 inversion each) stays the yardstick: this file computes
// the same Miller function up to a factor in Fq2, which the final exponentiation removes, so FE(core) == FE(host) word for word.
//
//   tower     Fq12 = Fq2[w] / (w^6 - xi), xi = 9 + i: six Fq2 coefficients of w^0 .. w^5, the order of zkwg_pairing.h
//   layout    a coefficient is one ZkF2::E (zkwg_ec29.h): on the device the two halves of an Fq2 sit on a lane pair, 9 limbs each, so an
//             Fq12 is 54 registers per lane.  Values are in the tables' form (x 2^261 mod q) and stay in lazy limb form through the loop.
//   T         the running point on the twist in XYZZ coordinates (x = X / ZZ, y = Y / ZZZ): the formulas of ec29_dbl / ec29_add_mixed,
//             restated here WITHOUT their equal / opposite / infinity branches so that every lane pair runs one instruction stream
//   lines     no inversion.  The tangent at T, times 2 U ZZZ (U = 2 Y):       l0 = 2 U ZZZ y_P    l1 = -2 M ZZ x_P    l3 = 2 M X - U^2   (M = 3 X^2)
//             the chord through T and Q = (x2, y2), times D = P ZZZ:          l0 = D y_P          l1 = -E x_P         l3 = E x2 - D y2
//             (P = x2 ZZ - X, R = y2 ZZZ - Y, E = R ZZ: the slope is E / D).  l = l0 + l1 w + l3 w^3 as in zk_pair_line.
//   loop      6 u + 2 over its 65 bits, binary as the host walks it (64 doublings, 36 additions: the constant is known at compile time,
//             so the branch on a bit is uniform), then the lines through psi(Q) and -psi^2(Q) (constants: zkwg_verify_core.h).
//   control   FIXED trip count and no branch on the points.  A Q outside the subgroup (T = +-Q can happen there), or zeros, run the same
//             instructions on meaningless values: nothing is indexed or looped on data, so such a pair cannot fault or hang; its value is
//             ignored by the caller (the `inside` flag) or replaced by 1 (infinity on either side: f = 1 exactly).
//
// BOUNDS ([U, V] of zkwg_fq29.h), as the host check build PROVES them: every function below claims its operands' and its results' bounds
// (ZKQ29_CLAIM / ZKQ29_CLAIM_IN: checked, then widened to exactly the claim), so one call is the function at the top of its contract, and
// tests/test_fq29_bounds_cpu.py makes that call for each of them.  An Fq2 product F::mul<VB>(a, b) is one reduced two-product dot product
// per half, and the even half negates the partner's half with (VB + 1) q WHATEVER b's own bound is: its value is below
// (Va Vb + Va (VB + 1)) / 169.28 + 1 q (169.28 = 2^261 / q) -- 1.18 q for [1, 2] x [1, 2] under mul<12>, 2.77 q for [1, 12] x [1, 12], not
// "[1, 2] whenever Va Vb <= 169".  Per function:
//     zk_f12_sqr       operand c0 .. c2 [1, 2], c3 .. c5 [1, 6] (what zk_f12_mul_line returns); result c0 .. c4 [1, 2], c5 [1, 12]
//     zk_f12_mul_line  operand c0 .. c4 [1, 6], c5 [1, 12] (f^2, or an earlier f l); l0, l1 [1, 2], l3 [1, 9]; result c0 .. c2 [1, 2], c3 .. c5 [1, 6]
//     zk_f12_mul       operands AND result c0 .. c4 [1, 2], c5 [1, 8] (ZK_F12_MUL_V5): closed under itself, which the loop of zk_pair_product
//                      needs (zk_f12_load gives [1, 2]; the accumulator is claimed after every product).  NOT [1, 12]: six such terms reach
//                      16.7 q in lo, and c5 = norm(lo) with them.
//     c_k = lo_k + xi hi_k,  lo_k = sum of the products a_i b_j with i + j = k (at most 6),  hi_k those with i + j = k + 6 (at most 5, below
//     10 q, normalised).  xi a = 9 a + i a for a = [1, V]: 4 a normalised [1, 4 V], 8 a + a [3, 9 V], plus the partner's half or its
//     negation [2, V + 1]: [5, 10 V + 1], normalised.  So lo_k + xi hi_k stays below 169 q, normalised, and ONE product with the constant 1
//     (an Fq product per lane: half an Fq2 product) brings it back to [1, 2].  c_5 has no hi part: lo normalised, no product.
// The sparse product has hi parts only for k < 3 (at most 2 terms -> xi<4>); k >= 3 are sums of 3: [1, 6].
// T: X [1, 10.25], Y [1, 7], ZZ, ZZZ [1, 2], an invariant of both steps (a doubling leaves X below 6.8 q, an addition below 10.1 q).  With
// Xyzz29's X [1, 11] the tangent's l3 = 2 M X - U^2 + 5 q could reach 9.006 q, above the 9 q that mul<9> (its negation constant 10 q) allows: the claim
// on T.X is what makes l3 [1, 9] true.  Line coefficients are right operands: l0, l1 [1, 2], l3 [1, 9] (tangent) / [1, 5] (chord).  The
// bound of every intermediate is written beside it.
//
// COST PER PAIR in Fq2 products (counted as zkwg_verify_core.h counts: a square = a product, the two-product dot product = 2, a product
// with an Fq value = 1/2):
//     doubling step  9 (ec29_dbl) + 3 (U ZZZ, M ZZ, M X) + 2 x 1/2                              = 13
//     addition step  10 (ec29_add_mixed) + 4 (D, E, E x2 - D y2) + 2 x 1/2                      = 15
//     f^2            15 cross products + 6 squares (the symmetry a_i a_j = a_j a_i) + 5 x 1/2   = 23.5   (36 + 2.5 without the symmetry)
//     f l            18 + 3 x 1/2                                                               = 19.5
//     64 x (13 + 23.5 + 19.5) + (36 + 2) x (15 + 19.5) + 2.5 (psi) + 3 (the store)             = 3,584 + 1,311 + 5.5 = 4,900.5
//     + 848 for the subgroup flag (zkwg_verify_core.h)                                          = 5,748.5
// Not built: the signed form of 6 u + 2 (fewer additions), a 2-3-2 tower squaring, dot products of more than two terms per reduction
// (fq29 columns have room for six: the 2.5 and 1.5 products with 1 and most reductions of f^2 would go).
#pragma once
#include "zkwg_verify_core.h"

#define ZK_PAIR_MAX (1u << 20)        // pairs per launch
#define ZK_F12_MUL_V5 8               // the value bound of coefficient 5 of zk_f12_mul's operands and result (BOUNDS below)
#define ZK_PAIR_FOLD 4u               // values one lane pair of zk_pair_product multiplies
#define ZK_PAIR_LOOP_LOW (6ull * ZK_VERIFY_U + 2ull)      // bits 0 .. 63 of 6 u + 2 (the product wraps: bit 64, the top one, is implied)

struct ZkF12 { ZkF2::E c[6]; };
struct ZkPairLine { ZkF2::E l0, l1, l3; };

// xi a = (9 a0 - a1) + (9 a1 + a0) i for a = [1, V]: [1, 10 V + 1]
#if defined(__HIP_DEVICE_COMPILE__)
template <int V> __device__ __forceinline__ Fq29 zk_pair_xi(const Fq29& a) {
  const Fq29 o = zk_pair_xchg(a);
  const Fq29 a4 = fq29_norm(fq29_dbl(fq29_dbl(a)));               // [1, 4 V]
  const Fq29 a9 = fq29_add(fq29_dbl(a4), a);                      // [3, 9 V]
  const Fq29 n = fq29_neg<V + 1, 1>(o);                           // [2, V + 1]
  Fq29 t;
#pragma unroll
  for (int i = 0; i < 9; ++i) t.l[i] = ZkF2::odd() ? o.l[i] : n.l[i];
  return fq29_norm(fq29_add(a9, t));                              // [5, 10 V + 1] -> [1, 10 V + 1]
}
#else
template <int V> static inline Fq29x2 zk_pair_xi(const Fq29x2& a) {
  Fq29 a9[2];
  for (int h = 0; h < 2; ++h) a9[h] = fq29_add(fq29_dbl(fq29_norm(fq29_dbl(fq29_dbl(a.c[h])))), a.c[h]);
  return Fq29x2{{fq29_norm(fq29_add(a9[0], fq29_neg<V + 1, 1>(a.c[1]))), fq29_norm(fq29_add(a9[1], a.c[0]))}};
}
#endif
// a = [1, <= 169] -> the same value as [1, 2]
static ZK_HD ZkF2::E zk_pair_red(const ZkF2::E& a) { return ZkF2::scale(a, fq29_one()); }
// lo + xi hi for lo = [<= 6, <= 12], hi = [<= 5, <= VH]: [1, 2]
template <int VH> ZK_HD ZkF2::E zk_pair_fold(const ZkF2::E& lo, const ZkF2::E& hi) {
  typedef ZkF2 F;
  return zk_pair_red(F::norm(F::add(lo, zk_pair_xi<VH>(F::norm(hi)))));
}

// the stated bounds of an Fq12's coefficients as claims (host check build; nothing elsewhere): coefficients 0 .. N - 1 [1, VLO], the others [1, VHI]
#define ZKF12_CLAIM(f, N, VLO, VHI) do { ZKQ29_CLAIM((f).c[0], 1, 0 < (N) ? (VLO) : (VHI)); ZKQ29_CLAIM((f).c[1], 1, 1 < (N) ? (VLO) : (VHI)); ZKQ29_CLAIM((f).c[2], 1, 2 < (N) ? (VLO) : (VHI)); \
    ZKQ29_CLAIM((f).c[3], 1, 3 < (N) ? (VLO) : (VHI)); ZKQ29_CLAIM((f).c[4], 1, 4 < (N) ? (VLO) : (VHI)); ZKQ29_CLAIM((f).c[5], 1, 5 < (N) ? (VLO) : (VHI)); } while (0)
#define ZKF12_CLAIM_IN(f, N, VLO, VHI) ZKQ29_CLAIM_IN((f).c[0], 1, 0 < (N) ? (VLO) : (VHI)); ZKQ29_CLAIM_IN((f).c[1], 1, 1 < (N) ? (VLO) : (VHI)); ZKQ29_CLAIM_IN((f).c[2], 1, 2 < (N) ? (VLO) : (VHI)); \
    ZKQ29_CLAIM_IN((f).c[3], 1, 3 < (N) ? (VLO) : (VHI)); ZKQ29_CLAIM_IN((f).c[4], 1, 4 < (N) ? (VLO) : (VHI)); ZKQ29_CLAIM_IN((f).c[5], 1, 5 < (N) ? (VLO) : (VHI))
#define ZKPAIR_CLAIM_T(t) do { ZKQ29_CLAIM((t).x, 1, 10.25); ZKQ29_CLAIM((t).y, 1, 7); ZKQ29_CLAIM((t).zz, 1, 2); ZKQ29_CLAIM((t).zzz, 1, 2); } while (0)

static ZK_HD ZkF12 zk_f12_one() {
  ZkF12 r;
#pragma unroll
  for (int k = 0; k < 6; ++k) r.c[k] = k ? ZkF2::zero() : ZkF2::one();
  return r;
}
// The products are written per output coefficient K and per term I, both template arguments: no loop is left for the compiler to unroll
// (it does not unroll one whose body holds six products, and an Fq12 indexed by a loop variable would live in scratch memory).
// term a_I b_(K - I) of coefficient K of a b, to lo, or a_I b_(K + 6 - I), to hi
template <int K, int I> ZK_HD void zk_f12_mul_term(const ZkF12& a, const ZkF12& b, ZkF2::E& lo, ZkF2::E& hi) {
  typedef ZkF2 F;
  if constexpr (I <= K) lo = F::add(lo, F::mul<12>(a.c[I], b.c[K - I]));          // <= [6, 8] (operands as zk_f12_mul states them)
  else hi = F::add(hi, F::mul<12>(a.c[I], b.c[K + 6 - I]));                       // <= [5, 7]
}
// coefficient K of a b, both c0 .. c4 [1, 2], c5 [1, 8]: K < 5 [1, 2], K = 5 [1, 8]
template <int K> ZK_HD ZkF2::E zk_f12_mul_coeff(const ZkF12& a, const ZkF12& b) {
  typedef ZkF2 F;
  F::E lo = F::zero(), hi = F::zero();
  zk_f12_mul_term<K, 0>(a, b, lo, hi); zk_f12_mul_term<K, 1>(a, b, lo, hi); zk_f12_mul_term<K, 2>(a, b, lo, hi);
  zk_f12_mul_term<K, 3>(a, b, lo, hi); zk_f12_mul_term<K, 4>(a, b, lo, hi); zk_f12_mul_term<K, 5>(a, b, lo, hi);
  if constexpr (K == 5) return F::norm(lo);
  else return zk_pair_fold<10>(lo, hi);
}
static ZK_HD ZkF12 zk_f12_mul(const ZkF12& a, const ZkF12& b) {
  ZkF12 r;
  ZKF12_CLAIM_IN(a, 5, 2, ZK_F12_MUL_V5);
  ZKF12_CLAIM_IN(b, 5, 2, ZK_F12_MUL_V5);
  r.c[0] = zk_f12_mul_coeff<0>(a, b); r.c[1] = zk_f12_mul_coeff<1>(a, b); r.c[2] = zk_f12_mul_coeff<2>(a, b);
  r.c[3] = zk_f12_mul_coeff<3>(a, b); r.c[4] = zk_f12_mul_coeff<4>(a, b); r.c[5] = zk_f12_mul_coeff<5>(a, b);
  ZKF12_CLAIM(r, 5, 2, ZK_F12_MUL_V5);
  return r;
}
// the cross products a_I a_J, I < J, of coefficient K of a a: J = K - I to lo, J = K + 6 - I to hi
template <int K, int I> ZK_HD void zk_f12_sqr_term(const ZkF12& a, ZkF2::E& lo, ZkF2::E& hi) {
  typedef ZkF2 F;
  if constexpr (K - I > I && K - I < 6) lo = F::add(lo, F::mul<12>(a.c[I], a.c[K - I]));           // <= 3 terms: [3, 6]
  if constexpr (K + 6 - I > I && K + 6 - I < 6) hi = F::add(hi, F::mul<12>(a.c[I], a.c[K + 6 - I]));   // <= 2 terms: [2, 4]
}
template <int K> ZK_HD ZkF2::E zk_f12_sqr_coeff(const ZkF12& a) {
  typedef ZkF2 F;
  F::E lo = F::zero(), hi = F::zero();
  zk_f12_sqr_term<K, 0>(a, lo, hi); zk_f12_sqr_term<K, 1>(a, lo, hi); zk_f12_sqr_term<K, 2>(a, lo, hi);
  zk_f12_sqr_term<K, 3>(a, lo, hi); zk_f12_sqr_term<K, 4>(a, lo, hi);
  lo = F::dbl(lo); hi = F::dbl(hi);                                                                // [6, 12], [4, 8]
  if constexpr (K % 2 == 0) {
    lo = F::add(lo, F::sqr<12>(a.c[K / 2]));                                                       // (K = 0, 2, 4: two cross terms at most) <= [5, 10]
    hi = F::add(hi, F::sqr<12>(a.c[K / 2 + 3]));                                                   // <= [5, 10]
  }
  if constexpr (K == 5) return F::norm(lo);
  else return zk_pair_fold<10>(lo, hi);
}
static ZK_HD ZkF12 zk_f12_sqr(const ZkF12& a) {
  ZkF12 r;
  ZKF12_CLAIM_IN(a, 3, 2, 6);
  r.c[0] = zk_f12_sqr_coeff<0>(a); r.c[1] = zk_f12_sqr_coeff<1>(a); r.c[2] = zk_f12_sqr_coeff<2>(a);
  r.c[3] = zk_f12_sqr_coeff<3>(a); r.c[4] = zk_f12_sqr_coeff<4>(a); r.c[5] = zk_f12_sqr_coeff<5>(a);
  ZKF12_CLAIM(r, 5, 2, 12);
  return r;
}
// coefficient K of f (l0 + l1 w + l3 w^3) for f = c0 .. c4 [1, 6], c5 [1, 12], l = [1, <= 9]: K < 3 [1, 2], K >= 3 [1, 6]
template <int K> ZK_HD ZkF2::E zk_f12_line_coeff(const ZkF12& f, const ZkPairLine& l) {
  typedef ZkF2 F;
  F::E lo = F::mul<9>(f.c[K], l.l0), hi = F::zero();
  if constexpr (K >= 1) lo = F::add(lo, F::mul<9>(f.c[K - 1], l.l1)); else hi = F::add(hi, F::mul<9>(f.c[5], l.l1));
  if constexpr (K >= 3) lo = F::add(lo, F::mul<9>(f.c[K - 3], l.l3)); else hi = F::add(hi, F::mul<9>(f.c[K + 3], l.l3));
  if constexpr (K >= 3) return F::norm(lo);                       // [3, 6] -> [1, 6]
  else return zk_pair_fold<4>(lo, hi);                            // hi <= [2, 4]
}
static ZK_HD ZkF12 zk_f12_mul_line(const ZkF12& f, const ZkPairLine& l) {
  ZkF12 r;
  ZKF12_CLAIM_IN(f, 5, 6, 12);
  ZKQ29_CLAIM_IN(l.l0, 1, 2); ZKQ29_CLAIM_IN(l.l1, 1, 2); ZKQ29_CLAIM_IN(l.l3, 1, 9);
  r.c[0] = zk_f12_line_coeff<0>(f, l); r.c[1] = zk_f12_line_coeff<1>(f, l); r.c[2] = zk_f12_line_coeff<2>(f, l);
  r.c[3] = zk_f12_line_coeff<3>(f, l); r.c[4] = zk_f12_line_coeff<4>(f, l); r.c[5] = zk_f12_line_coeff<5>(f, l);
  ZKF12_CLAIM(r, 3, 2, 6);
  return r;
}

// T <- 2 T and the tangent at T evaluated at P.  yP = [1, 1], nxP = -x_P = [1, 2]
static ZK_HD ZkPairLine zk_pair_dbl_step(Xyzz29<ZkF2>& t, const Fq29& yP, const Fq29& nxP) {
  typedef ZkF2 F;
  typedef F::E E;
  ZKPAIR_CLAIM_T(t);
  ZKQ29_CLAIM_IN(yP, 1, 1); ZKQ29_CLAIM_IN(nxP, 1, 2);
  const E U = F::norm(F::dbl(t.y));                               // [1, 14]
  const E V = F::sqr<14>(U);                                      // [1, 4]
  const E W = F::mul<4>(U, V);                                    // [1, 2]
  const E S = F::mul<4>(t.x, V);                                  // [1, 2]
  const E X2 = F::sqr<11>(t.x);                                   // [1, 3]
  const E M = F::norm(F::add(F::dbl(X2), X2));                    // [1, 9]
  const E MM = F::sqr<9>(M);                                      // [1, 3]
  ZkPairLine l;
  l.l0 = F::scale(F::mul<2>(U, t.zzz), fq29_norm(fq29_dbl(yP)));  // [1, 2] x [1, 2] -> [1, 2]
  l.l1 = F::scale(F::mul<2>(M, t.zz), fq29_norm(fq29_dbl(nxP)));  // [1, 2] x [1, 4] -> [1, 2]
  l.l3 = F::norm(F::sub<5, 1>(F::dbl(F::mul<11>(M, t.x)), V));    // [2, 4] - [1, 4] -> [4, 9] -> [1, 9]
  Xyzz29<F> r;
  r.x = F::norm(F::sub<5, 2>(MM, F::dbl(S)));                     // [1, 8]
  const E T = F::sub<12, 1>(S, r.x);                              // [3, 14]
  r.y = F::msub<14, 7>(M, T, W, t.y);                             // [1, 7]
  r.zz = F::mul<2>(V, t.zz);
  r.zzz = F::mul<2>(W, t.zzz);
  t = r;
  ZKPAIR_CLAIM_T(t);
  ZKQ29_CLAIM(l.l0, 1, 2); ZKQ29_CLAIM(l.l1, 1, 2); ZKQ29_CLAIM(l.l3, 1, 9);
  return l;
}
// T <- T + Q and the chord through them at P, Q = (x2, y2) affine, both [1, <= 2]
static ZK_HD ZkPairLine zk_pair_add_step(Xyzz29<ZkF2>& t, const ZkF2::E& x2, const ZkF2::E& y2, const Fq29& yP, const Fq29& nxP) {
  typedef ZkF2 F;
  typedef F::E E;
  ZKPAIR_CLAIM_T(t);
  ZKQ29_CLAIM_IN(x2, 1, 2); ZKQ29_CLAIM_IN(y2, 1, 2); ZKQ29_CLAIM_IN(yP, 1, 1); ZKQ29_CLAIM_IN(nxP, 1, 2);
  const E P = F::norm(F::sub<12, 1>(F::mul<2>(x2, t.zz), t.x));   // [1, 14]
  const E Rr = F::norm(F::sub<8, 1>(F::mul<2>(y2, t.zzz), t.y));  // [1, 10]
  const E D = F::mul<2>(P, t.zzz), Ee = F::mul<2>(Rr, t.zz);      // [1, 2]
  ZkPairLine l;
  l.l0 = F::scale(D, yP);                                         // [1, 2]
  l.l1 = F::scale(Ee, nxP);                                       // [1, 2]
  l.l3 = F::msub<2, 2>(Ee, x2, D, y2);                            // [1, 5]
  Xyzz29<F> r;
  const E PP = F::sqr<14>(P);                                     // [1, 4]
  r.zz = F::mul<4>(t.zz, PP);
  const E Q = F::mul<4>(t.x, PP);                                 // [1, 2]
  const E PPP = F::mul<4>(P, PP);                                 // [1, 2]
  r.zzz = F::mul<2>(t.zzz, PPP);
  const E RR = F::sqr<10>(Rr);                                    // [1, 3]
  r.x = F::norm(F::sub<5, 2>(F::sub<3, 1>(RR, PPP), F::dbl(Q)));  // [1, 11]
  const E T = F::sub<12, 1>(Q, r.x);                              // [3, 14]
  r.y = F::msub<14, 2>(Rr, T, t.y, PPP);                          // [1, 7]
  t = r;
  ZKPAIR_CLAIM_T(t);
  ZKQ29_CLAIM(l.l0, 1, 2); ZKQ29_CLAIM(l.l1, 1, 2); ZKQ29_CLAIM(l.l3, 1, 5);
  return l;
}

// f_{6u+2, Q}(P) with the two correction lines, up to a factor in Fq2.  Q: x, y [1, 1] (a table-form point), xP, yP [1, 1]
static ZK_HD ZkF12 zk_pair_miller_loop(const ZkF2::E& qx, const ZkF2::E& qy, const Fq29& xP, const Fq29& yP) {
  typedef ZkF2 F;
  const Fq29 nxP = fq29_norm(fq29_neg<2, 1>(xP));                 // [1, 2]
  Xyzz29<F> t{qx, qy, F::one(), F::one()};
  ZkF12 f = zk_f12_one();
  const u64 loop = ZK_PAIR_LOOP_LOW;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int i = 63; i >= 0; --i) {
    f = zk_f12_mul_line(zk_f12_sqr(f), zk_pair_dbl_step(t, yP, nxP));
    if ((loop >> i) & 1ull) f = zk_f12_mul_line(f, zk_pair_add_step(t, qx, qy, yP, nxP));
  }
  const F::E q1x = F::mul<1>(zk_verify_conj<1>(qx), zk_verify_const(zk_verify_cx1_c0(), zk_verify_cx1_c1()));     // psi(Q): [1, 2]
  const F::E q1y = F::mul<1>(zk_verify_conj<1>(qy), zk_verify_const(zk_verify_cy1_c0(), zk_verify_cy1_c1()));
  f = zk_f12_mul_line(f, zk_pair_add_step(t, q1x, q1y, yP, nxP));
  const F::E q2x = F::scale(qx, zk_verify_gamma());               // -psi^2(Q) = (gamma x, y)
  return zk_f12_mul_line(f, zk_pair_add_step(t, q2x, qy, yP, nxP));
}

// ---- memory: 12 Fq of canonical Montgomery words (x 2^256), the image of the host's Fq12; half h of a lane pair owns words 2 k + h --------
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ ZkF12 zk_f12_load(const Fq* w, u32 h) {
  ZkF12 r;
#pragma unroll
  for (int k = 0; k < 6; ++k) r.c[k] = fq29_mul(fq29_from_fq(zk_ld_fq(w + 2 * k + h)), fq29_t266());       // [1, 2]
  return r;
}
__device__ __forceinline__ void zk_f12_store(Fq* w, const ZkF12& f, u32 h) {
#pragma unroll
  for (int k = 0; k < 6; ++k) w[2 * k + h] = fq29_to_fq<2>(fq29_mul(f.c[k], fq29_r256()));
}
// first ? a : b, by masks (a select of two addresses would keep both values in memory)
__device__ __forceinline__ ZkF12 zk_f12_select(bool first, const ZkF12& a, const ZkF12& b) {
  ZkF12 r;
  const u32 m = first ? 0xffffffffu : 0u;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
#pragma unroll
    for (int i = 0; i < 9; ++i) r.c[k].l[i] = (a.c[k].l[i] & m) | (b.c[k].l[i] & ~m);
  }
  return r;
}
#else
static ZK_HD ZkF12 zk_f12_load(const Fq* w, u32 h) {
  ZkF12 r;
  for (int k = 0; k < 6; ++k) r.c[k] = Fq29x2{{fq29_mul(fq29_from_fq(w[2 * k]), fq29_t266()), fq29_mul(fq29_from_fq(w[2 * k + 1]), fq29_t266())}};
  return r;
}
static ZK_HD void zk_f12_store(Fq* w, const ZkF12& f, u32 h) {
  for (int k = 0; k < 6; ++k) for (int j = 0; j < 2; ++j) w[2 * k + j] = fq29_to_fq<2>(fq29_mul(f.c[k].c[j], fq29_r256()));
}
static ZK_HD ZkF12 zk_f12_select(bool first, const ZkF12& a, const ZkF12& b) {
  ZkF12 r = first ? a : b;
  for (int k = 0; k < 6; ++k) for (int j = 0; j < 2; ++j) ZKQ29_SELECT(r.c[k].c[j], a.c[k].c[j], b.c[k].c[j]);
  return r;
}
#endif

// the pair (p, q) of table-form points, half h of a lane pair: out = the Miller value (1 when either is infinity); returns whether q is
// in the subgroup of order r (infinity is).  Du: zk_verify_u_digits()
static ZK_HD bool zk_pair_miller_point(const G1Affine* p, const G2Affine* q, u32 h, const ZkPhase2Digits& Du, Fq* out) {
  typedef ZkF2 F;
  const Fq px = zk_ld_fq(&p->x), py = zk_ld_fq(&p->y);
  const Aff29<F> Q = ZkEcG2::load(q, h, false);                   // x [1, 1], y [1, 1]
  const bool inf = Q.inf || (fq_is_zero(px) && fq_is_zero(py));
  const ZkF12 f = zk_pair_miller_loop(Q.x, Q.y, zk_q29_base(px), zk_q29_base(py));
  zk_f12_store(out, zk_f12_select(inf, zk_f12_one(), f), h);
  return zk_verify_g2_in_subgroup(q, h, Du);
}
