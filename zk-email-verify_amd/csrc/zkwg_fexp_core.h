// The final exponentiation of the BN254 pairing per LANE PAIR, FE(f) = f^((q^12 - 1) / r), and the sum of a proof's public-input points:
// the per-value bodies of per-proof groth16 verification (zkwg_groth16_verify_each), shared by the kernels (csrc/zkwg_kernels_fexp.hip),
// by the host path of the call (device = -1, and e(alpha, beta) of every call) and by the host build of the CPU tests
// (tests/native/fexptest.cpp, ZKWG_FQ29_CHECK counting every violated limb-form bound).  The value is EXACT: word for word what
// zk_pair_final_exp (csrc/zkwg_pairing.h, 2,790-bit square-and-multiply) returns, not a fixed power of it.
//
//   exponent  (q^12 - 1) / r = (q^6 - 1) (q^2 + 1) h,  h = (q^4 - q^2 + 1) / r = q^3 + l2 q^2 + l1 q + l0 with u = 4965661367192848881,
//             l2 = 6 u^2 + 1,  l1 = -(36 u^3 + 18 u^2 + 12 u - 1),  l0 = -(36 u^3 + 30 u^2 + 18 u + 2)   (tests/test_fexp_cpu.py checks the identity)
//   easy      g = conj(f) f^-1, g <- g^(q^2) g.  conj negates c1, c3, c5 (it is f^(q^6)).  The inverse goes down the tower by norms:
//             n = f conj(f) lies in Fq6 = Fq2[w^2], N = n^(q^2) n^(q^4), m = n N lies in Fq2, m^-1 = conj(m) / (m0^2 + m1^2) with ONE Fq
//             inversion (zk_setup_fq29_inv, the fixed-trip Fermat power), f^-1 = conj(f) N m^-1.  f = 0 gives 0 through every step.
//   after it  g is in the cyclotomic subgroup: conj(g) = g^-1 (negative exponents and the signed form of u are free), and the
//             Granger-Scott squaring holds.  With g_k = (c_k, c_(k+3)) in Fq4 = Fq2[s] / (s^2 - xi), s = w^3:
//                 g^2 = (3 g0^2 - 2 conj(g0)) + (3 s g2^2 + 2 conj(g1)) w + (3 g1^2 - 2 conj(g2)) w^2
//             (conj negates the s half; s (x, y) = (xi y, x)): three Fq4 squares of three Fq2 products each.
//   g^u       the non-adjacent form of u, 63 digits, 24 of them non-zero: 62 cyclotomic squarings, 23 products with g or conj(g)
//   hard      Devegili-Scott-Dahab: with a = g^u, b = g^(u^2), c = g^(u^3) and F_k the Frobenius map x -> x^(q^k)
//                 y0 = F1(g) F2(g) F3(g)   y1 = conj(g)   y2 = F2(b)   y3 = conj(F1(a))   y4 = conj(a F1(b))   y5 = conj(b)   y6 = conj(c F1(c))
//                 g^h = y0 y1^2 y2^6 y3^12 y4^18 y5^30 y6^36
//             by the chain T0 = y6^2 y4 y5, T1 = y3 y5 T0, T0 <- T0 y2, T1 <- (T1^2 T0)^2, T0 <- (T1 y1)^2, T1 <- T1 y0, result T0 T1:
//             13 steps of one product each, the last 13 of ZK_FEXP_PROGRAM below.
//   Frobenius F_k, k = 1, 2, 3: coefficient j is conjugated (k odd) and multiplied by xi^(j (q^k - 1) / 6) -- the table zk_fexp_frob_c,
//             which tests/test_fexp_cpu.py derives again from the oracle's field arithmetic.  For k = 2 the constants lie in Fq.
//   control   FIXED: every trip count is a compile-time constant, the digits of u are constants, a step's operations are chosen by the
//             launch, never by a value; nothing is indexed by data.  Zeros and values outside every subgroup run the same instructions.
//
// THE CUT INTO LAUNCHES.  The chain wants g, a, b, c and their Frobenius images at once: six or seven Fq12 of 54 registers a lane, which
// do not fit beside the temporaries of a product (the easy part in one piece did not either: 584 bytes of scratch memory a lane).  So the
// exponentiation is a PROGRAM of 22 small steps (ZK_FEXP_PROGRAM), each one launch, and a value travels between them through device
// memory as 384 bytes of canonical Montgomery words (zk_f12_store), which is nothing beside the arithmetic:
//     zk_fexp_fold_value   the product of k adjacent values (k = 3: the three pairs of a proof; k = 1 needs no launch)
//     zk_fexp_step_value   out = post(pre_a(x) pre_b(y)): ONE product, with conj / Frobenius / cyclotomic squaring before and after it
//     zk_fexp_ninv_value   the step of the inversion that leaves the tower: m = (n N)_0 in Fq2, its inverse, N / m
//     zk_fexp_pow_u_value  g -> g^u, three times
//
// BOUNDS ([U, V] of zkwg_fq29.h; the rule of zkwg_pair_core.h: every function claims its operands' and results' bounds, so one call is the
// function at the top of its contract, and tests/test_fexp_cpu.py makes that call for each).  Two forms of an Fq12 occur:
//     M   c0 .. c4 [1, 2], c5 [1, 8]: the operands and the result of zk_f12_mul (zkwg_pair_core.h), closed under it
//     S   every coefficient [1, 2]: what zk_f12_load, zk_fexp_conj, zk_fexp_frob, zk_fexp_cyc_sqr and zk_fexp_scale return; S is inside M
// Every function here takes M and returns M or S.  The bound of each intermediate is written beside it.
//
// COST PER VALUE in Fq2 products (counted as zkwg_pair_core.h counts: the two-product dot product per lane = 1, a product with an Fq
// value = 1/2, load and store 3 each):
//     zk_f12_mul 36 + 5 x 1/2 = 38.5     zk_fexp_cyc_sqr 9 + 6 x 1/2 = 12     conj 1.5     F1, F3 6     F2 2.5
//     a product step = load 6 + 38.5 + store 3 = 47.5 beside what it does before and after the product
//     easy           5 product steps 237.5, conj three times 4.5, F2 four times 10, the inversion step: load 6, m 6.5, the Fq inversion (253
//                    squares + 109 products per lane) 181, the norm and conj(m) / d 1, the scaling 6, store 3 = 203.5         = 455.5
//     fold (k = 3)   load 9, two products 77, store 3                                                                        = 89
//     g^u            load 3, 62 x 12, 23 x 38.5, conj(g) at the 12 negative digits 18, store 3                        = 1,653.5   (three times: 4,960.5)
//     hard           13 product steps 617.5, F1 four times 24, F2 twice 5, F3 6, conj five times 7.5, four cyclotomic squarings 48   = 708
//     FE of one value 455.5 + 4,960.5 + 708 = 6,124; of a proof's three Miller values 6,213 -- a little above one Miller loop with its
//     subgroup flag (5,748.5)
// Not built: fused kernels (they would save the 18 x 9 of the product steps' loads and stores, 3 % of the whole), compressed squarings
// (Karabina), the symmetry of the products by conj(g) in g^u.
#pragma once
#include "zkwg_pair_core.h"

#define ZK_FEXP_MAX (1u << 20)                      // values per launch
#define ZK_FEXP_U_POS 0x450a14044a890a01ULL         // the non-adjacent form of u: the digits +1 ...
#define ZK_FEXP_U_NEG 0x0020815000200010ULL         // ... and -1 (POS - NEG = u; the top digit is bit 62, +1)

// THE PROGRAM: what is launched, in order, on the values F (the input, or the product of a proof's three values), G = g, A = g^u,
// B = g^(u^2), C = g^(u^3), three temporaries and OUT.  A step reads one or two values from memory and writes one (which may be an operand).
//     MUL     dst = post(pre_a(a) pre_b(b))       pre: none, conj, F1, F2, F3, F2 twice (F4), the cyclotomic square; post: none, conj, square, both
//     NINV    dst = b / (a b)_0 for a = n in Fq6 and b = N = n^(q^2) n^(q^4): n^-1, through the Fq2 inversion
//     POW_U   dst = a^u
enum { ZK_FEXP_OP_MUL = 0, ZK_FEXP_OP_NINV = 1, ZK_FEXP_OP_POW_U = 2 };
enum { ZK_FEXP_PRE_NONE = 0, ZK_FEXP_PRE_CONJ = 1, ZK_FEXP_PRE_F1 = 2, ZK_FEXP_PRE_F2 = 3, ZK_FEXP_PRE_F3 = 4, ZK_FEXP_PRE_F4 = 5, ZK_FEXP_PRE_SQR = 6 };
enum { ZK_FEXP_POST_NONE = 0, ZK_FEXP_POST_CONJ = 1, ZK_FEXP_POST_SQR = 2, ZK_FEXP_POST_CONJ_SQR = 3 };
enum { ZK_FEXP_F = 0, ZK_FEXP_G = 1, ZK_FEXP_A = 2, ZK_FEXP_B = 3, ZK_FEXP_C = 4, ZK_FEXP_T0 = 5, ZK_FEXP_T1 = 6, ZK_FEXP_Y = 7, ZK_FEXP_OUT = 8, ZK_FEXP_SLOTS = 9 };
struct ZkFexpStep { u8 op, dst, a, b, pre_a, pre_b, post; };
#define ZK_FEXP_EASY_STEPS 6          // the first steps of the program: F -> G (after step 4, T1 holds 1 / F)
#define ZK_FEXP_STEPS 22
#define ZKFX_MUL(dst, a, pa, b, pb, post) {ZK_FEXP_OP_MUL, ZK_FEXP_##dst, ZK_FEXP_##a, ZK_FEXP_##b, ZK_FEXP_PRE_##pa, ZK_FEXP_PRE_##pb, ZK_FEXP_POST_##post}
static const ZkFexpStep ZK_FEXP_PROGRAM[ZK_FEXP_STEPS] = {
  ZKFX_MUL(T0, F, NONE, F, CONJ, NONE),                           // n = f conj(f), in Fq6
  ZKFX_MUL(T1, T0, F2, T0, F4, NONE),                             // N = n^(q^2) n^(q^4)
  {ZK_FEXP_OP_NINV, ZK_FEXP_T0, ZK_FEXP_T0, ZK_FEXP_T1, 0, 0, 0}, // 1 / n = N / (n N)
  ZKFX_MUL(T1, F, CONJ, T0, NONE, NONE),                          // 1 / f = conj(f) / n
  ZKFX_MUL(T0, F, CONJ, T1, NONE, NONE),                          // f^(q^6 - 1)
  ZKFX_MUL(G, T0, F2, T0, NONE, NONE),                            // g = f^((q^6 - 1)(q^2 + 1))
  {ZK_FEXP_OP_POW_U, ZK_FEXP_A, ZK_FEXP_G, ZK_FEXP_G, 0, 0, 0},
  {ZK_FEXP_OP_POW_U, ZK_FEXP_B, ZK_FEXP_A, ZK_FEXP_A, 0, 0, 0},
  {ZK_FEXP_OP_POW_U, ZK_FEXP_C, ZK_FEXP_B, ZK_FEXP_B, 0, 0, 0},
  ZKFX_MUL(T0, C, NONE, C, F1, CONJ_SQR),                         // y6^2 = conj(c F1(c))^2
  ZKFX_MUL(T1, A, NONE, B, F1, CONJ),                             // y4 = conj(a F1(b))
  ZKFX_MUL(T0, T0, NONE, T1, NONE, NONE),                         // y6^2 y4
  ZKFX_MUL(T0, T0, NONE, B, CONJ, NONE),                          // T0 = y6^2 y4 y5
  ZKFX_MUL(T1, A, F1, B, NONE, CONJ),                             // y3 y5 = conj(F1(a) b)
  ZKFX_MUL(T1, T1, NONE, T0, NONE, NONE),                         // T1 = y3 y5 T0
  ZKFX_MUL(T0, T0, NONE, B, F2, NONE),                            // T0 <- T0 y2
  ZKFX_MUL(T1, T1, SQR, T0, NONE, SQR),                           // T1 <- (T1^2 T0)^2
  ZKFX_MUL(T0, T1, NONE, G, CONJ, SQR),                           // T0 <- (T1 y1)^2
  ZKFX_MUL(Y, G, F1, G, F2, NONE),                                // F1(g) F2(g)
  ZKFX_MUL(Y, Y, NONE, G, F3, NONE),                              // y0
  ZKFX_MUL(T1, T1, NONE, Y, NONE, NONE),                          // T1 <- T1 y0
  ZKFX_MUL(OUT, T0, NONE, T1, NONE, NONE),                        // g^h
};

// xi^(J (q^K - 1) / 6), half H, in the tables' form (x 2^261 mod q).  J = 0 is 1; for K = 2 the odd halves are 0.
template <int K, int J, int H> ZK_HD Fq29 zk_fexp_frob_c() {
  static_assert(K >= 1 && K <= 3 && J >= 0 && J < 6 && (H == 0 || H == 1), "no such constant");
  if constexpr (J == 0 && H == 0) return fq29_one();
  if constexpr (K == 1 && J == 1 && H == 0) return Fq29{{0x0a0c2399u, 0x1aa2357cu, 0x0149b22du, 0x0487bf1bu, 0x0b89bb5eu, 0x1313c7e1u, 0x1d61fdb5u, 0x060c56b5u, 0x002e0560u}};
  if constexpr (K == 1 && J == 1 && H == 1) return Fq29{{0x1bc6cc33u, 0x177dfb71u, 0x161dd8abu, 0x0180969du, 0x058d47f5u, 0x1ab975b5u, 0x01c26a2du, 0x1cd88219u, 0x00009b83u}};
  if constexpr (K == 1 && J == 2 && H == 0) return Fq29{{0x04a59190u, 0x06f504d9u, 0x0bf870bbu, 0x171ffd5cu, 0x1ac4d17du, 0x04be36d5u, 0x0bceec27u, 0x1a83a513u, 0x002492b3u}};
  if constexpr (K == 1 && J == 2 && H == 1) return Fq29{{0x11142ef1u, 0x0b31acc7u, 0x1d5818bcu, 0x180afc17u, 0x1a63177eu, 0x15765b3bu, 0x118f742eu, 0x063a509au, 0x00135e4eu}};
  if constexpr (K == 1 && J == 3 && H == 0) return Fq29{{0x1b1f0678u, 0x0373fb06u, 0x13170fbdu, 0x185d74b7u, 0x0241131fu, 0x16e18435u, 0x1ef3b6ceu, 0x01f06f02u, 0x001d46bdu}};
  if constexpr (K == 1 && J == 3 && H == 1) return Fq29{{0x19a647d5u, 0x19fdefabu, 0x1d925d1au, 0x0d1f6c5fu, 0x08ac6cc5u, 0x1fa5621au, 0x134f06feu, 0x09a72816u, 0x0015871du}};
  if constexpr (K == 1 && J == 4 && H == 0) return Fq29{{0x1081f85eu, 0x139a3585u, 0x124aed48u, 0x034ce260u, 0x19e166e5u, 0x0b172958u, 0x0d2df880u, 0x0de46877u, 0x00167751u}};
  if constexpr (K == 1 && J == 4 && H == 1) return Fq29{{0x0f616a78u, 0x05940429u, 0x181bb386u, 0x066e257bu, 0x00e66254u, 0x0c12b5cdu, 0x0ef6c029u, 0x1c2232e3u, 0x0006f9f8u}};
  if constexpr (K == 1 && J == 5 && H == 0) return Fq29{{0x07461d8cu, 0x0434a6b0u, 0x14f8b697u, 0x0b0aa80fu, 0x118b92dfu, 0x0471333du, 0x18c6d066u, 0x07d8f7b0u, 0x0010a3f0u}};
  if constexpr (K == 1 && J == 5 && H == 1) return Fq29{{0x1eb54987u, 0x08d56d1eu, 0x0c80f1d8u, 0x1536f380u, 0x06b4b4a7u, 0x082bcd3cu, 0x19349170u, 0x17aea9fcu, 0x000817f6u}};
  if constexpr (K == 2 && J == 1 && H == 0) return Fq29{{0x0e4983b2u, 0x0b774393u, 0x03d607b6u, 0x0fdad48bu, 0x1d262e9bu, 0x01644f52u, 0x11b94d87u, 0x1a3314f3u, 0x0024594fu}};
  if constexpr (K == 2 && J == 2 && H == 0) return Fq29{{0x18ccb791u, 0x175b1c3au, 0x0b83d6e2u, 0x0e8ed071u, 0x1282bee2u, 0x04220e84u, 0x1fe4017fu, 0x15084d4au, 0x00169119u}};
  if constexpr (K == 2 && J == 3 && H == 0) return Fq29{{0x03003126u, 0x0ce8395eu, 0x0420727bu, 0x01891eb7u, 0x0ae269bfu, 0x0598fff2u, 0x0ed19539u, 0x09315e8bu, 0x00229c18u}};
  if constexpr (K == 2 && J == 4 && H == 0) return Fq29{{0x0a337995u, 0x158d1d23u, 0x189c9b98u, 0x12fa4e45u, 0x185faadcu, 0x0176f16du, 0x0eed93bau, 0x14291140u, 0x000c0afeu}};
  if constexpr (K == 2 && J == 5 && H == 0) return Fq29{{0x1fb045b6u, 0x09a9447bu, 0x10eecc6cu, 0x1446525fu, 0x03031a95u, 0x1eb9323cu, 0x00c2dfc1u, 0x1953d8e9u, 0x0019d334u}};
  if constexpr (K == 3 && J == 1 && H == 0) return Fq29{{0x0e6a3d3du, 0x0e0034bcu, 0x1d2fc927u, 0x167e071du, 0x07ccd695u, 0x04b45d3du, 0x0e70688eu, 0x1e41c930u, 0x00103828u}};
  if constexpr (K == 3 && J == 1 && H == 1) return Fq29{{0x0f4e6b31u, 0x05dd85eau, 0x16ca0ad7u, 0x19d17c36u, 0x1bae3e83u, 0x01bf781fu, 0x030191b5u, 0x10c0063eu, 0x00133cf9u}};
  if constexpr (K == 3 && J == 2 && H == 0) return Fq29{{0x136caecdu, 0x19c70818u, 0x1dae30d1u, 0x028eb786u, 0x0bee8f49u, 0x1a51d4beu, 0x135c7d00u, 0x11fdec39u, 0x000cad5fu}};
  if constexpr (K == 3 && J == 2 && H == 1) return Fq29{{0x06e485d6u, 0x1a0e1cafu, 0x10aa918bu, 0x04618e04u, 0x07ab5997u, 0x1790c244u, 0x06cbab85u, 0x1ee779f9u, 0x00266696u}};
  if constexpr (K == 3 && J == 3 && H == 0) return Fq29{{0x1d5df6cfu, 0x1d9065afu, 0x095b9391u, 0x0a77ae19u, 0x1344c658u, 0x0bf9bc8bu, 0x01b32a72u, 0x0c6bb731u, 0x00131d91u}};
  if constexpr (K == 3 && J == 3 && H == 1) return Fq29{{0x1ed6b572u, 0x0706710au, 0x1ee04634u, 0x15b5b670u, 0x0cd96cb2u, 0x0335dea6u, 0x0d57da42u, 0x04b4fe1du, 0x001add31u}};
  if constexpr (K == 3 && J == 4 && H == 0) return Fq29{{0x0af866c4u, 0x068222a0u, 0x1d8c6ce8u, 0x0028befbu, 0x12de19ccu, 0x1193e6bau, 0x09d0a776u, 0x1b6142e1u, 0x0014766fu}};
  if constexpr (K == 3 && J == 4 && H == 1) return Fq29{{0x09d402f7u, 0x0a994a07u, 0x169567b7u, 0x09218b7fu, 0x1b0b8541u, 0x032ce2a0u, 0x0f936727u, 0x16ad3976u, 0x000baf8cu}};
  if constexpr (K == 3 && J == 5 && H == 0) return Fq29{{0x0314d9feu, 0x0e0dd877u, 0x18eb90b3u, 0x06a988e8u, 0x0d6b9fe0u, 0x025b9f1eu, 0x161fcb32u, 0x0ed57bb5u, 0x0014445bu}};
  if constexpr (K == 3 && J == 5 && H == 1) return Fq29{{0x1b3b7638u, 0x1086ac9cu, 0x057c4a00u, 0x1b93c320u, 0x022ad2d0u, 0x0cace295u, 0x0226f886u, 0x0ee880a1u, 0x0012c9d7u}};
  return fq29_zero();
}

// coefficient J of f^(q^K) from coefficient J of f, c = [1, 2] (J = 5: [1, 8]): [1, 2]
template <int K, int J> ZK_HD ZkF2::E zk_fexp_frob_coeff(const ZkF2::E& c) {
  typedef ZkF2 F;
  ZKQ29_CLAIM_IN(c, 1, J == 5 ? ZK_F12_MUL_V5 : 2);
  if constexpr (K == 2 && J == 0) return c;                                               // (c0 is [1, 2] in both forms)
  else if constexpr (K == 2) return F::scale(c, zk_fexp_frob_c<2, J, 0>());               // [1, 8] x [1, 1] -> [1, 2]
  else return F::mul<1>(zk_verify_conj<8>(c), zk_verify_const(zk_fexp_frob_c<K, J, 0>(), zk_fexp_frob_c<K, J, 1>()));       // [1, 9] x [1, 1] -> [1, 2]
}
// f^(q^K), K = 1, 2, 3: M -> S
template <int K> ZK_HD ZkF12 zk_fexp_frob(const ZkF12& f) {
  ZkF12 r;
  ZKF12_CLAIM_IN(f, 5, 2, ZK_F12_MUL_V5);
  r.c[0] = zk_fexp_frob_coeff<K, 0>(f.c[0]); r.c[1] = zk_fexp_frob_coeff<K, 1>(f.c[1]); r.c[2] = zk_fexp_frob_coeff<K, 2>(f.c[2]);
  r.c[3] = zk_fexp_frob_coeff<K, 3>(f.c[3]); r.c[4] = zk_fexp_frob_coeff<K, 4>(f.c[4]); r.c[5] = zk_fexp_frob_coeff<K, 5>(f.c[5]);
  ZKF12_CLAIM(r, 6, 2, 2);
  return r;
}
// f^(q^6): c1, c3, c5 negated (a product with -1 each, so that they stay [1, 2]; c0, c2, c4 as they are).  M -> S
static ZK_HD ZkF12 zk_fexp_conj(const ZkF12& f) {
  typedef ZkF2 F;
  ZkF12 r;
  ZKF12_CLAIM_IN(f, 5, 2, ZK_F12_MUL_V5);
  r.c[0] = f.c[0]; r.c[2] = f.c[2]; r.c[4] = f.c[4];
  r.c[1] = F::scale(f.c[1], zk_verify_minus_one()); r.c[3] = F::scale(f.c[3], zk_verify_minus_one());       // [1, 2] x [1, 1] -> [1, 2]
  r.c[5] = F::scale(f.c[5], zk_verify_minus_one());                                                         // [1, 8] x [1, 1] -> [1, 2]
  ZKF12_CLAIM(r, 6, 2, 2);
  return r;
}
// every coefficient times k = [1, 3] (an Fq2 value).  M -> S
static ZK_HD ZkF12 zk_fexp_scale(const ZkF12& f, const ZkF2::E& k) {
  typedef ZkF2 F;
  ZkF12 r;
  ZKF12_CLAIM_IN(f, 5, 2, ZK_F12_MUL_V5);
  ZKQ29_CLAIM_IN(k, 1, 3);
  r.c[0] = F::mul<3>(f.c[0], k); r.c[1] = F::mul<3>(f.c[1], k); r.c[2] = F::mul<3>(f.c[2], k);       // (Va 3 + Va 4) / 169.28 + 1 <= 1.34 for Va <= 8
  r.c[3] = F::mul<3>(f.c[3], k); r.c[4] = F::mul<3>(f.c[4], k); r.c[5] = F::mul<3>(f.c[5], k);
  ZKF12_CLAIM(r, 6, 2, 2);
  return r;
}

// 1 / m for m = [1, 2] in Fq2 (0 for m = 0): conj(m) / (m0^2 + m1^2) with one Fq inversion; [1, 3]
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ Fq29 zk_fexp_f2_norm(const Fq29& m) {
  const Fq29 s = fq29_sqr(m);                                     // this half squared: [1, 2]
  return fq29_norm(fq29_add(s, zk_pair_xchg(s)));                 // [2, 4] -> [1, 4]
}
#else
static inline Fq29 zk_fexp_f2_norm(const Fq29x2& m) { return fq29_norm(fq29_add(fq29_sqr(m.c[0]), fq29_sqr(m.c[1]))); }
#endif
static ZK_HD ZkF2::E zk_fexp_f2_inv(const ZkF2::E& m) {
  ZKQ29_CLAIM_IN(m, 1, 2);
  const Fq29 d = zk_fexp_f2_norm(m);                              // [1, 4]
  ZKQ29_CLAIM(d, 1, 4);
  const Fq29 di = zk_setup_fq29_inv(d);                           // d^(q - 2): [1, 2]; 0 for d = 0
  ZKQ29_CLAIM(di, 1, 2);
  const ZkF2::E r = zk_setup_iz3(ZkEcG2(), m, di);                // (m0 di, -m1 di): [1, 3]
  ZKQ29_CLAIM(r, 1, 3);
  return r;
}
// 1 / n for n in Fq6 (its c1, c3, c5 are 0 modulo q), given N = n^(q^2) n^(q^4): m = n N lies in Fq2 (only its coefficient 0 is
// computed), 1 / n = N / m.  0 for n = 0.  M, M -> S
static ZK_HD ZkF12 zk_fexp_ninv(const ZkF12& n, const ZkF12& N) {
  ZKF12_CLAIM_IN(n, 5, 2, ZK_F12_MUL_V5);
  ZKF12_CLAIM_IN(N, 5, 2, ZK_F12_MUL_V5);
  const ZkF2::E m = zk_f12_mul_coeff<0>(n, N);                    // [1, 2]
  ZKQ29_CLAIM(m, 1, 2);
  const ZkF12 r = zk_fexp_scale(N, zk_fexp_f2_inv(m));
  ZKF12_CLAIM(r, 6, 2, 2);
  return r;
}

// (x + y s)^2 = (x^2 + xi y^2) + 2 x y s for x = [1, 2], y = [1, <= VY]: p = x^2 + xi y^2 [1, 23], m = x y [1, 2]
template <int VY> ZK_HD void zk_fexp_f4_sqr(const ZkF2::E& x, const ZkF2::E& y, ZkF2::E& p, ZkF2::E& m) {
  typedef ZkF2 F;
  ZKQ29_CLAIM_IN(x, 1, 2); ZKQ29_CLAIM_IN(y, 1, VY);
  p = F::norm(F::add(F::sqr<2>(x), zk_pair_xi<2>(F::sqr<VY>(y))));          // [1, 2] + [1, 21] -> [1, 23]
  m = F::mul<VY>(x, y);                                                     // (2 x 8 + 2 x 9) / 169.28 + 1: [1, 2]
  ZKQ29_CLAIM(p, 1, 23); ZKQ29_CLAIM(m, 1, 2);
}
// 3 p - 2 x for p = [1, 23], x = [1, 2]: [1, 2]
static ZK_HD ZkF2::E zk_fexp_3p_less_2x(const ZkF2::E& p, const ZkF2::E& x) {
  typedef ZkF2 F;
  ZKQ29_CLAIM_IN(p, 1, 23); ZKQ29_CLAIM_IN(x, 1, 2);
  const F::E t = F::norm(F::add(F::dbl(p), p));                   // [3, 69] -> [1, 69]
  const F::E r = zk_pair_red(F::norm(F::sub<5, 2>(t, F::dbl(x))));        // - [2, 4]: [4, 74] -> [1, 74] -> [1, 2]
  ZKQ29_CLAIM(r, 1, 2);
  return r;
}
// 6 m + 2 y for m = [1, <= 21], y = [1, <= 8]: [1, 2]
static ZK_HD ZkF2::E zk_fexp_6m_plus_2y(const ZkF2::E& m, const ZkF2::E& y) {
  typedef ZkF2 F;
  ZKQ29_CLAIM_IN(m, 1, 21); ZKQ29_CLAIM_IN(y, 1, ZK_F12_MUL_V5);
  const F::E m2 = F::dbl(m);                                      // [2, 42]
  const F::E m6 = F::norm(F::add(F::dbl(m2), m2));                // [6, 126] -> [1, 126]
  const F::E r = zk_pair_red(F::norm(F::add(m6, F::dbl(y))));     // + [2, 16]: [3, 142] -> [1, 2]
  ZKQ29_CLAIM(r, 1, 2);
  return r;
}
// g^2 for g in the cyclotomic subgroup (Granger-Scott; for any other g a meaningless value, 0 for 0).  M -> S
static ZK_HD ZkF12 zk_fexp_cyc_sqr(const ZkF12& g) {
  typedef ZkF2 F;
  ZkF12 r;
  ZKF12_CLAIM_IN(g, 5, 2, ZK_F12_MUL_V5);
  F::E p0, m0, p1, m1, p2, m2;
  zk_fexp_f4_sqr<2>(g.c[0], g.c[3], p0, m0);                      // g0^2 = (p0, 2 m0)
  zk_fexp_f4_sqr<2>(g.c[1], g.c[4], p1, m1);
  zk_fexp_f4_sqr<ZK_F12_MUL_V5>(g.c[2], g.c[5], p2, m2);
  r.c[0] = zk_fexp_3p_less_2x(p0, g.c[0]);                        // 3 g0^2 - 2 conj(g0)
  r.c[3] = zk_fexp_6m_plus_2y(m0, g.c[3]);
  r.c[1] = zk_fexp_6m_plus_2y(zk_pair_xi<2>(m2), g.c[1]);         // 3 s g2^2 + 2 conj(g1): s (p2, 2 m2) = (2 xi m2, p2); xi m2 [1, 21]
  r.c[4] = zk_fexp_3p_less_2x(p2, g.c[4]);
  r.c[2] = zk_fexp_3p_less_2x(p1, g.c[2]);                        // 3 g1^2 - 2 conj(g2)
  r.c[5] = zk_fexp_6m_plus_2y(m1, g.c[5]);
  ZKF12_CLAIM(r, 6, 2, 2);
  return r;
}
// g^u for g in the cyclotomic subgroup.  M -> M
static ZK_HD ZkF12 zk_fexp_power_u(const ZkF12& g) {
  ZKF12_CLAIM_IN(g, 5, 2, ZK_F12_MUL_V5);
  ZkF12 acc = g;                                                  // digit 62
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int i = 61; i >= 0; --i) {
    acc = zk_fexp_cyc_sqr(acc);
    if (((ZK_FEXP_U_POS | ZK_FEXP_U_NEG) >> i) & 1ull) {          // (constants and the loop counter: uniform)
      ZkF12 b = g;
      if ((ZK_FEXP_U_NEG >> i) & 1ull) b = zk_fexp_conj(g);
      acc = zk_f12_mul(acc, b);
    }
    ZKF12_CLAIM(acc, 5, 2, ZK_F12_MUL_V5);
  }
  return acc;
}

// an operand of a step, as the step wants it.  M -> M (S but for PRE_NONE)
static ZK_HD ZkF12 zk_fexp_pre(const ZkF12& x, u32 pre) {
  ZKF12_CLAIM_IN(x, 5, 2, ZK_F12_MUL_V5);
  ZkF12 r = x;
  if (pre == ZK_FEXP_PRE_CONJ) r = zk_fexp_conj(x);
  else if (pre == ZK_FEXP_PRE_F1) r = zk_fexp_frob<1>(x);
  else if (pre == ZK_FEXP_PRE_F2) r = zk_fexp_frob<2>(x);
  else if (pre == ZK_FEXP_PRE_F3) r = zk_fexp_frob<3>(x);
  else if (pre == ZK_FEXP_PRE_F4) r = zk_fexp_frob<2>(zk_fexp_frob<2>(x));
  else if (pre == ZK_FEXP_PRE_SQR) r = zk_fexp_cyc_sqr(x);
  ZKF12_CLAIM(r, 5, 2, ZK_F12_MUL_V5);
  return r;
}
// one step of the chain on values in memory (12 Fq each; out may be x or y), half h of a lane pair
static ZK_HD void zk_fexp_step_value(const Fq* x, const Fq* y, u32 pre_a, u32 pre_b, u32 post, Fq* out, u32 h) {
  const ZkF12 a = zk_fexp_pre(zk_f12_load(x, h), pre_a), b = zk_fexp_pre(zk_f12_load(y, h), pre_b);
  ZkF12 r = zk_f12_mul(a, b);
  if (post == ZK_FEXP_POST_CONJ || post == ZK_FEXP_POST_CONJ_SQR) r = zk_fexp_conj(r);
  if (post == ZK_FEXP_POST_SQR || post == ZK_FEXP_POST_CONJ_SQR) r = zk_fexp_cyc_sqr(r);
  ZKF12_CLAIM(r, 5, 2, ZK_F12_MUL_V5);
  zk_f12_store(out, r, h);
}
static ZK_HD void zk_fexp_ninv_value(const Fq* n, const Fq* N, Fq* out, u32 h) { zk_f12_store(out, zk_fexp_ninv(zk_f12_load(n, h), zk_f12_load(N, h)), h); }
// the product of the k >= 1 values at f (k x 12 Fq)
static ZK_HD void zk_fexp_fold_value(const Fq* f, u32 k, Fq* out, u32 h) {
  ZkF12 acc = zk_f12_load(f, h);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (u32 j = 1; j < k; ++j) {
    acc = zk_f12_mul(acc, zk_f12_load(f + 12ull * j, h));
    ZKF12_CLAIM(acc, 5, 2, ZK_F12_MUL_V5);
  }
  zk_f12_store(out, acc, h);
}
static ZK_HD void zk_fexp_pow_u_value(const Fq* g, Fq* out, u32 h) { zk_f12_store(out, zk_fexp_power_u(zk_f12_load(g, h)), h); }

// ---- the sum of a proof's public-input points ---------------------------------------------------------------------------------------------
// a G1 point in the zkey's form (x 2^256; zeros = infinity) as a base of the point formulas: x [1, 1], y [1, 1]
static ZK_HD Aff29<ZkF1> zk_g16_load_g1(const G1Affine* p) {
  const Fq x = zk_ld_fq(&p->x), y = zk_ld_fq(&p->y);
  return Aff29<ZkF1>{zk_q29_base(zk_fq_r256_to_r261(x)), zk_q29_neg_if(zk_q29_base(zk_fq_r256_to_r261(y)), false), fq_is_zero(x) && fq_is_zero(y)};
}
// out = -(ic0 + sum_j terms[j]), j < n_terms, affine in the zkey's form (zeros = infinity): the complete formulas of zkwg_ec29.h (a term at
// infinity, equal and opposite summands take their branches), then ONE Fermat inversion.  Every point on the curve, words below q.
static ZK_HD void zk_g16_vkx_point(const G1Affine* ic0, const G1Affine* terms, u32 n_terms, G1Affine* out) {
  typedef ZkF1 F;
  Xyzz29<F> acc = ec29_from_affine<F>(zk_g16_load_g1(ic0));
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (u32 j = 0; j < n_terms; ++j) acc = ec29_add_mixed<F>(acc, zk_g16_load_g1(terms + j));
  ZKEC29_CLAIM_XYZZ(F, acc);                                      // X [1, 11], Y [1, 2], ZZ, ZZZ [1, 2]
  acc.y = fq29_norm(fq29_neg<3, 1>(acc.y));                       // -Y: [2, 3] -> [1, 3]
  const Fq29 dinv = zk_setup_fq29_inv(zk_setup_den_of<ZkEcG1>(acc));      // 1 / ZZZ (1 for infinity): [1, 2]
  zk_setup_affine<ZkEcG1>(acc, dinv, out, 0);                     // y = [1, 3] x [1, 3]
}
