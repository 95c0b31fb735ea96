// Is a point of the twist in G2, the subgroup of order r?  The per-point body of `powersoftau verify`'s hot path, shared by the kernel
// (csrc/zkwg_kernels_verify.hip), by zkwg_pairing_check's handful of G2 arguments (csrc/zkwg_pairing.h) and by the host build of the CPU
// tests (tests/native/verifytest.cpp, ZKWG_FQ29_CHECK counting every violated limb-form bound).
//
// THE CRITERION [EXT: El Housni, Guillevic, Piellard, "Co-factor clearing and subgroup membership testing on pairing-friendly curves",
// the BN case; PAPERS.md].  With A = [u] Q, u = 4965661367192848881 the curve's parameter:
//
//     Q in G2   <=>   A + Q + psi(A) + psi^2(A) = psi^3([2] A)
//
// psi = twist^-1 o Frobenius o twist:  psi(x, y) = (conj(x) xi^((q-1)/3), conj(y) xi^((q-1)/2)), xi = 9 + i; on G2 it is multiplication by q,
// so the left side minus the right is [(u + 1) + u q + u q^2 - 2 u q^3] Q, and that integer is 0 modulo r (checked numerically; the
// forward direction).  The converse rests on the paper; the tests compare the verdict with the DEFINITION [r] Q = infinity on subgroup
// points, raw twist points, points of order 10069, 5864401 and their product (the prime factors of the cofactor 2 q - r besides the big
// one) and those added to subgroup points (tests/test_verify_cpu.py, tests/test_verify_gpu.py).
//
// THE WALK.  [u] Q is ONE shared 63-bit scalar: the lockstep non-adjacent-form walk of phase 2 (zk_phase2_scale_point: 62 doublings and 23
// mixed additions for this u).  psi works on the accumulator as it is: x = X / ZZ, y = Y / ZZZ, and conjugation is a field automorphism, so
//     psi(X, Y, ZZ, ZZZ) = (conj(X) cx, conj(Y) cy, conj(ZZ), conj(ZZZ))             (ZZ^3 = ZZZ^2 is kept)
//     psi^2(X, Y, ZZ, ZZZ) = (gamma X, -Y, ZZ, ZZZ),  gamma = xi^((q^2-1)/3) in Fq,  xi^((q^2-1)/2) = -1
// No inversion anywhere: the final equality is cross-multiplied.  The three additions and the doubling are ec29_add_mixed / ec29_add /
// ec29_dbl with their equal / opposite / infinity cases (a point of small order meets them), not excluded.
//
// BOUNDS ([U, V] of zkwg_fq29.h).  A conjugated half is M q - a, normalised: [1, V + 1] for a = [1, V].  X [1, 11] -> [1, 12], Y [1, 7]
// -> [1, 8]: both are LEFT operands of the constant products that follow (12 x 1 <= 169), whose results are [1, 2].  ZZ, ZZZ [1, 2] ->
// [1, 3] is outside what ec29_add accepts for a ZZ (it negates the partner's half with 3 q), so they take a product with 1 and are [1, 2]
// again: two products per psi, 0.5 % of the walk, instead of a second set of point formulas.  -Y of psi^2 is a product with -1 for the
// same reason (Y must stay [1, 7] for the doubling ec29_add falls back to).  So psi(A), psi^2(A), psi^3(2 A) are X, Y, ZZ, ZZZ = [1, 2],
// inside Xyzz29's bounds, and every sum is what zkwg_ec29.h states: X [1, 11], Y [1, 7], ZZ, ZZZ [1, 2].
//
// COST PER POINT, in Fq2 products (zkwg_ec29.h, squares counted as products, the two-product dot product as 2: ec29_dbl 9,
// ec29_add_mixed 10, ec29_add 14; a product with an Fq constant counts 1/2):
//     62 ec29_dbl + 23 ec29_add_mixed  (the walk)  + 1 mixed + 2 full additions + 1 doubling + (4 + 1 + 4) constant products + 4 for the
//     comparison  =  558 + 230 + 47 + 9 + 4 = 848, against (254 x 9 + 73 x 10 =) 3,016 of [r] Q by the same walk over the non-adjacent
//     form of r (254 doublings, 73 additions): ratio 0.28.
#pragma once
#include "zkwg_phase2_core.h"

#define ZK_VERIFY_PIECE (1u << 20)    // points per launch of the subgroup test
#define ZK_VERIFY_U 0x44e992b44a6909f1ULL

static inline ZkPhase2Digits zk_verify_u_digits() {
  u8 s[32] = {0};
  const u64 u = ZK_VERIFY_U;
  memcpy(s, &u, 8);
  return zk_phase2_recode(s);
}

// the constants of psi, psi^2, psi^3 in the tables' form (x 2^261 mod q; Python: oracle/pyref/bn254_pairing._FROB_X, _FROB_Y and their powers)
ZK_HD Fq29 zk_verify_cx1_c0() { return Fq29{{0x04a59190u, 0x06f504d9u, 0x0bf870bbu, 0x171ffd5cu, 0x1ac4d17du, 0x04be36d5u, 0x0bceec27u, 0x1a83a513u, 0x002492b3u}}; }   // xi^((q-1)/3)
ZK_HD Fq29 zk_verify_cx1_c1() { return Fq29{{0x11142ef1u, 0x0b31acc7u, 0x1d5818bcu, 0x180afc17u, 0x1a63177eu, 0x15765b3bu, 0x118f742eu, 0x063a509au, 0x00135e4eu}}; }
ZK_HD Fq29 zk_verify_cy1_c0() { return Fq29{{0x1b1f0678u, 0x0373fb06u, 0x13170fbdu, 0x185d74b7u, 0x0241131fu, 0x16e18435u, 0x1ef3b6ceu, 0x01f06f02u, 0x001d46bdu}}; }   // xi^((q-1)/2)
ZK_HD Fq29 zk_verify_cy1_c1() { return Fq29{{0x19a647d5u, 0x19fdefabu, 0x1d925d1au, 0x0d1f6c5fu, 0x08ac6cc5u, 0x1fa5621au, 0x134f06feu, 0x09a72816u, 0x0015871du}}; }
ZK_HD Fq29 zk_verify_cx3_c0() { return Fq29{{0x136caecdu, 0x19c70818u, 0x1dae30d1u, 0x028eb786u, 0x0bee8f49u, 0x1a51d4beu, 0x135c7d00u, 0x11fdec39u, 0x000cad5fu}}; }   // xi^((q^3-1)/3)
ZK_HD Fq29 zk_verify_cx3_c1() { return Fq29{{0x06e485d6u, 0x1a0e1cafu, 0x10aa918bu, 0x04618e04u, 0x07ab5997u, 0x1790c244u, 0x06cbab85u, 0x1ee779f9u, 0x00266696u}}; }
ZK_HD Fq29 zk_verify_cy3_c0() { return Fq29{{0x1d5df6cfu, 0x1d9065afu, 0x095b9391u, 0x0a77ae19u, 0x1344c658u, 0x0bf9bc8bu, 0x01b32a72u, 0x0c6bb731u, 0x00131d91u}}; }   // xi^((q^3-1)/2)
ZK_HD Fq29 zk_verify_cy3_c1() { return Fq29{{0x1ed6b572u, 0x0706710au, 0x1ee04634u, 0x15b5b670u, 0x0cd96cb2u, 0x0335dea6u, 0x0d57da42u, 0x04b4fe1du, 0x001add31u}}; }
ZK_HD Fq29 zk_verify_gamma() { return Fq29{{0x18ccb791u, 0x175b1c3au, 0x0b83d6e2u, 0x0e8ed071u, 0x1282bee2u, 0x04220e84u, 0x1fe4017fu, 0x15084d4au, 0x00169119u}}; }    // xi^((q^2-1)/3), in Fq
ZK_HD Fq29 zk_verify_minus_one() { return Fq29{{0x03003126u, 0x0ce8395eu, 0x0420727bu, 0x01891eb7u, 0x0ae269bfu, 0x0598fff2u, 0x0ed19539u, 0x09315e8bu, 0x00229c18u}}; }

// an Fq2 constant as ZkF2 holds an element, and the conjugate of a = [1, <= V]: [1, V + 1]
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ Fq29 zk_verify_const(const Fq29& c0, const Fq29& c1) {
  Fq29 r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = ZkF2::odd() ? c1.l[i] : c0.l[i];
  return r;
}
template <int V> __device__ __forceinline__ Fq29 zk_verify_conj(const Fq29& a) {
  const Fq29 n = fq29_norm(fq29_neg<V + 1, 1>(a));
  Fq29 r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = ZkF2::odd() ? n.l[i] : a.l[i];
  return r;
}
#else
static inline Fq29x2 zk_verify_const(const Fq29& c0, const Fq29& c1) { return Fq29x2{{c0, c1}}; }
template <int V> static inline Fq29x2 zk_verify_conj(const Fq29x2& a) { return Fq29x2{{a.c[0], fq29_norm(fq29_neg<V + 1, 1>(a.c[1]))}}; }
#endif

// psi (K = 1) and psi^3 (K = 3) of an accumulator: X, Y, ZZ, ZZZ = [1, 2]
template <int K>
ZK_HD Xyzz29<ZkF2> zk_verify_psi(const Xyzz29<ZkF2>& a) {
  typedef ZkF2 F;
  ZKEC29_CLAIM_XYZZ_IN(F, a);
  if (ec29_is_inf<F>(a)) return a;
  const F::E cx = K == 1 ? zk_verify_const(zk_verify_cx1_c0(), zk_verify_cx1_c1()) : zk_verify_const(zk_verify_cx3_c0(), zk_verify_cx3_c1());
  const F::E cy = K == 1 ? zk_verify_const(zk_verify_cy1_c0(), zk_verify_cy1_c1()) : zk_verify_const(zk_verify_cy3_c0(), zk_verify_cy3_c1());
  Xyzz29<F> r;
  r.x = F::mul<1>(zk_verify_conj<11>(a.x), cx);                   // [1, 12] x [1, 1] -> [1, 2]
  r.y = F::mul<1>(zk_verify_conj<7>(a.y), cy);                    // [1, 8] x [1, 1] -> [1, 2]
  r.zz = F::mul<1>(zk_verify_conj<2>(a.zz), F::one());            // [1, 3] x 1 -> [1, 2]
  r.zzz = F::mul<1>(zk_verify_conj<2>(a.zzz), F::one());
  return r;
}
// psi^2: (gamma X, -Y, ZZ, ZZZ)
static ZK_HD Xyzz29<ZkF2> zk_verify_psi2(const Xyzz29<ZkF2>& a) {
  typedef ZkF2 F;
  ZKEC29_CLAIM_XYZZ_IN(F, a);
  if (ec29_is_inf<F>(a)) return a;
  return Xyzz29<F>{F::scale(a.x, zk_verify_gamma()), F::scale(a.y, zk_verify_minus_one()), a.zz, a.zzz};      // [1, 11] x [1, 1], [1, 7] x [1, 1] -> [1, 2]
}
// a == b as points: X1 ZZ2 = X2 ZZ1 and Y1 ZZZ2 = Y2 ZZZ1
static ZK_HD bool zk_verify_same_point(const Xyzz29<ZkF2>& a, const Xyzz29<ZkF2>& b) {
  typedef ZkF2 F;
  const bool ia = ec29_is_inf<F>(a), ib = ec29_is_inf<F>(b);
  ZKEC29_CLAIM_XYZZ_IN(F, a);
  ZKEC29_CLAIM_XYZZ_IN(F, b);
  if (ia || ib) return ia && ib;
  const F::E ex = F::sub<3, 1>(F::mul<2>(a.x, b.zz), F::mul<2>(b.x, a.zz));            // [1, 2] - [1, 2] -> [3, 5]
  const F::E ey = F::sub<3, 1>(F::mul<2>(a.y, b.zzz), F::mul<2>(b.y, a.zzz));
  const bool zx = F::is_zero_mod<5>(ex), zy = F::is_zero_mod<5>(ey);                   // (both evaluated: the lanes of a pair stay together)
  return zx && zy;
}
// the table-form point at p (half h of a lane pair) is in the subgroup of order r; infinity is.  Du: zk_verify_u_digits()
static ZK_HD bool zk_verify_g2_in_subgroup(const G2Affine* p, u32 h, const ZkPhase2Digits& Du) {
  typedef ZkF2 F;
  const Aff29<F> Q = ZkEcG2::load(p, h, false);                   // x [1, 1], y [1, 1]
  if (Q.inf) return true;
  const Xyzz29<F> A = zk_phase2_scale_point<ZkEcG2>(p, h, Du);    // [u] Q: X [1, 11], Y [1, 7]
  ZKEC29_CLAIM_XYZZ(F, A);
  Xyzz29<F> L = ec29_add_mixed<F>(A, Q);                          // X [1, 11], Y [1, 7]
  L = ec29_add<F>(L, zk_verify_psi<1>(A));                        // X [1, 10], Y [1, 7]
  L = ec29_add<F>(L, zk_verify_psi2(A));
  ZKEC29_CLAIM_XYZZ(F, L);
  const Xyzz29<F> Rr = zk_verify_psi<3>(ec29_dbl<F>(A));
  ZKEC29_CLAIM_XYZZ(F, Rr);
  return zk_verify_same_point(L, Rr);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// host: n points in the zkey's form -> verdicts (1 = inside); false: a point is not on the curve (or not reduced)
static inline bool zk_verify_g2_subgroup_host(const G2Affine* in, u64 n, u8* inside) {
  const ZkPhase2Digits Du = zk_verify_u_digits();
  bool ok = true;
  for (u64 i = 0; i < n; ++i) {
    G2Affine t;
    if (!zk_setup_prepare_point_g2(in + i, &t, 0)) { ok = false; inside[i] = 0; continue; }
    inside[i] = zk_verify_g2_in_subgroup(&t, 0, Du) ? 1 : 0;
  }
  return ok;
}
#endif
