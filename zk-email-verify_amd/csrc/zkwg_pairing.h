// BN254 optimal ate pairing on the HOST, over the canonical-word field code (zkwg_fq.h, zkwg_g2.h): the few dozen pairings of a
// `powersoftau verify` (zkwg/ptau.py) -- the millions of points in front of them are folded into two points per check on the device
// (zkwg_point_rlc_device), so nothing here is a hot path and nothing here runs on the device.  Model and yardstick:
// oracle/pyref/bn254_pairing.py (test infrastructure; the product does not import it).
//
//   tower       Fq12 = Fq2[w] / (w^6 - xi), xi = 9 + i: six Fq2 coefficients, schoolbook product (zero coefficients of the left operand
//               are skipped: a line has three)
//   lines       affine: l(P) = y_P - lambda x_P w + (lambda x_T - y_T) w^3 with the slope lambda on the twist (one Fq2 inversion a line)
//   loop        6 u + 2 (65 bits), u = 4965661367192848881, then the two Frobenius lines through psi(Q) and -psi^2(Q)
//   final       f^((q^12 - 1) / r) by square-and-multiply over the 2,790-bit exponent: ONE per call, whatever the number of pairs
// Every G2 argument must be in the subgroup of order r (zkwg_verify_core.h, the host build of the kernel's per-point body): outside it
// the value is not bilinear, and the loop's "T = +-Q never happens" rests on the order.
#pragma once
#include <string>
#include "zkwg_verify_core.h"

#if !defined(__HIP_DEVICE_COMPILE__)          // host only: nothing of this file exists in the device pass

struct Fq12 { Fq2 c[6]; };
static inline Fq12 fq12_one() { Fq12 r; for (int i = 0; i < 6; ++i) r.c[i] = fq2_zero(); r.c[0] = fq2_one(); return r; }
static inline bool fq12_eq(const Fq12& a, const Fq12& b) { bool e = true; for (int i = 0; i < 6; ++i) e = e && fq2_eq(a.c[i], b.c[i]); return e; }
// a (9 + i)
static inline Fq2 fq2_mul_xi(const Fq2& a) {
  const Fq2 a2 = fq2_dbl(a), a4 = fq2_dbl(a2), a9 = fq2_add(fq2_dbl(a4), a);
  return Fq2{fq_sub(a9.c0, a.c1), fq_add(a9.c1, a.c0)};
}
static inline Fq12 fq12_mul(const Fq12& a, const Fq12& b) {
  Fq2 t[11];
  for (int k = 0; k < 11; ++k) t[k] = fq2_zero();
  for (int i = 0; i < 6; ++i) {
    if (fq2_is_zero(a.c[i])) continue;
    for (int j = 0; j < 6; ++j) t[i + j] = fq2_add(t[i + j], fq2_mul(a.c[i], b.c[j]));
  }
  Fq12 r;
  for (int k = 0; k < 6; ++k) r.c[k] = k < 5 ? fq2_add(t[k], fq2_mul_xi(t[k + 6])) : t[k];
  return r;
}
// xi^((q-1)/3), xi^((q-1)/2), xi^((q^2-1)/3) in the zkey's form (x 2^256 mod q)
static inline Fq2 zk_pair_frob_x() {
  return Fq2{Fq{{0xb5773b104563ab30ULL, 0x347f91c8a9aa6454ULL, 0x7a007127242e0991ULL, 0x1956bcd8118214ecULL}},
             Fq{{0x6e849f1ea0aa4757ULL, 0xaa1c7b6d89f89141ULL, 0xb6e713cdfae0ca3aULL, 0x26694fbb4e82ebc3ULL}}};
}
static inline Fq2 zk_pair_frob_y() {
  return Fq2{Fq{{0xe4bbdd0c2936b629ULL, 0xbb30f162e133bacbULL, 0x31a9d1b6f9645366ULL, 0x253570bea500f8ddULL}},
             Fq{{0xa1d77ce45ffe77c7ULL, 0x07affd117826d1dbULL, 0x6d16bd27bb7edc6bULL, 0x2c87200285defeccULL}}};
}
static inline Fq zk_pair_gamma() { return Fq{{0x3350c88e13e80b9cULL, 0x7dce557cdb5e56b9ULL, 0x6001b4b8b615564aULL, 0x2682e617020217e0ULL}}; }

// the line through t and q (the tangent when they are equal) at p, and t + q
static inline Fq12 zk_pair_line(const G2Affine& t, const G2Affine& q, const G1Affine& p, G2Affine& sum) {
  Fq2 lam;
  if (fq2_eq(t.x, q.x) && fq2_eq(t.y, q.y)) {
    const Fq2 x2 = fq2_sqr(t.x);
    lam = fq2_mul(fq2_add(fq2_dbl(x2), x2), fq2_inv(fq2_dbl(t.y)));
  } else {
    lam = fq2_mul(fq2_sub(q.y, t.y), fq2_inv(fq2_sub(q.x, t.x)));
  }
  const Fq2 x3 = fq2_sub(fq2_sub(fq2_sqr(lam), t.x), q.x);
  const Fq2 y3 = fq2_sub(fq2_mul(lam, fq2_sub(t.x, x3)), t.y);
  Fq12 l;
  for (int i = 0; i < 6; ++i) l.c[i] = fq2_zero();
  l.c[0] = Fq2{p.y, fq_zero()};
  l.c[1] = fq2_neg(Fq2{fq_mont_mul(lam.c0, p.x), fq_mont_mul(lam.c1, p.x)});
  l.c[3] = fq2_sub(fq2_mul(lam, t.x), t.y);
  sum = G2Affine{x3, y3};                           // (last: callers pass t itself)
  return l;
}
// f_{6u+2, Q}(P) with the two correction lines; p, q: not infinity, on their curves, q in the subgroup
static inline Fq12 zk_pair_miller(const G1Affine& p, const G2Affine& q) {
  const unsigned __int128 loop = 6 * (unsigned __int128)ZK_VERIFY_U + 2;
  Fq12 f = fq12_one();
  G2Affine t = q;
  for (int i = 63; i >= 0; --i) {                   // (bit 64 is the top one)
    const Fq12 l = zk_pair_line(t, t, p, t);
    f = fq12_mul(l, fq12_mul(f, f));
    if ((u64)(loop >> i) & 1) f = fq12_mul(zk_pair_line(t, q, p, t), f);
  }
  const Fq2 q1x = fq2_mul(Fq2{q.x.c0, fq_neg(q.x.c1)}, zk_pair_frob_x()), q1y = fq2_mul(Fq2{q.y.c0, fq_neg(q.y.c1)}, zk_pair_frob_y());
  const G2Affine q1{q1x, q1y};                                                                            // psi(Q)
  const G2Affine q2{Fq2{fq_mont_mul(q.x.c0, zk_pair_gamma()), fq_mont_mul(q.x.c1, zk_pair_gamma())}, q.y};  // -psi^2(Q) = (gamma x, y)
  f = fq12_mul(zk_pair_line(t, q1, p, t), f);
  G2Affine unused;
  return fq12_mul(zk_pair_line(t, q2, p, unused), f);
}
// (q^12 - 1) / r, little-endian words
static const u64 ZK_PAIR_FINAL_EXP[44] = {
  0x86964b64ca86f120ULL, 0x40a4efb7e54523a4ULL, 0x837fa97896e84abbULL, 0x361102b6b9b2b918ULL,
  0xc0de81def35692daULL, 0xbe04c7e8a6c3c760ULL, 0xd766f9c9d570bb7fULL, 0xc230974d83561841ULL,
  0x5bba1668c3be69a3ULL, 0x7f3811c410526294ULL, 0x29baee7ddadda71cULL, 0xbf813b8d145da900ULL,
  0x641bbadf423f9a2cULL, 0xa80bb4ea44eacc5eULL, 0xcd65664814fde37cULL, 0x4a0364b9580291d2ULL,
  0xee93dfb10826f0ddULL, 0x6b42db8dc5514724ULL, 0xbb10cf430b0f3785ULL, 0x40494e406f804216ULL,
  0x55cfe107acf3aafbULL, 0x2088ec80e0ebae87ULL, 0x846a3ed011a337a0ULL, 0x48a45a4a1e3a5195ULL,
  0xe5664568dfc50e16ULL, 0xab6a41294c0cc4ebULL, 0x82d0d602d268c7daULL, 0x6668449aed3cc48aULL,
  0x5062cd0fb2015dfcULL, 0x7f2940a8b1ddb3d1ULL, 0x77f5b63a2a226448ULL, 0xfef0781361e443aeULL,
  0xf977870e88d5c6c8ULL, 0x790364a61f676baaULL, 0x5887e72eceaddea3ULL, 0x1377e563a09a1b70ULL,
  0x0c54efee1bd8c3b2ULL, 0x3ec3d15ad524d8f7ULL, 0xdaf15466b2383a5dULL, 0xe1e30a73bb94fec0ULL,
  0x6a1c71015f3f7be2ULL, 0x842d43bf6369b1ffULL, 0x20fddadf107d20bcULL, 0x0000002f4b6dc970ULL};
static inline Fq12 zk_pair_final_exp(const Fq12& f) {
  Fq12 r = fq12_one();
  bool started = false;
  for (int i = 44 * 64 - 1; i >= 0; --i) {
    if (started) r = fq12_mul(r, r);
    if ((ZK_PAIR_FINAL_EXP[i >> 6] >> (i & 63)) & 1) { r = started ? fq12_mul(r, f) : f; started = true; }
  }
  return r;
}
// out = prod_i e(g1[i], g2[i]) (the reduced pairing; a pair with a point at infinity contributes 1).  Points in the zkey's form.
// ZKWG_RC_BAD_CONFIG + err: a word >= q or a point off its curve ("curve"), a G2 point outside the subgroup of order r ("subgroup").
static inline int zk_pairing_product(const u8* g1, const u8* g2, u32 n, Fq12& out, std::string& err) {
  Fq12 f = fq12_one();
  for (u32 i = 0; i < n; ++i) {
    G1Affine p;
    G2Affine q;
    memcpy((void*)&p, g1 + 64 * (u64)i, 64);
    memcpy((void*)&q, g2 + 128 * (u64)i, 128);
    u8 inside = 0;
    if (!zk_setup_prepare_point_g1(&p, nullptr, 0) || !zk_verify_g2_subgroup_host(&q, 1, &inside)) {
      err = "pairing: pair " + std::to_string(i) + ": a point is not on its curve (or not reduced)";
      return ZKWG_RC_BAD_CONFIG;
    }
    if (!inside) {
      err = "pairing: pair " + std::to_string(i) + ": the G2 point is outside the subgroup of order r";
      return ZKWG_RC_BAD_CONFIG;
    }
    if (g1_is_inf(p) || g2_is_inf(q)) continue;
    f = fq12_mul(f, zk_pair_miller(p, q));
  }
  out = zk_pair_final_exp(f);
  return ZKWG_RC_OK;
}
#endif
