// Per-proof groth16 verification, the HOST part (include/zkwg.h "checking proofs", zkwg_groth16_verify_each): the per-proof checks and
// the key's checks of the batch verifier (csrc/zkwg_pair_host.h: zk_g16_check_key, zk_g16_read_proof), e(alpha, beta), the comparison, and
// the host mirror of the device stage.  Shared by csrc/zkwg_fexp_api.hip and by the host build of the CPU tests (tests/native/fexptest.cpp).
// Host only.
//
// THE EQUATION, per proof i that passed the host checks, with vkx_i = IC_0 + sum_j x_ij IC_j:
//     FE( f(A_i, B_i) . f(-vkx_i, gamma) . f(-C_i, delta) ) = e(alpha, beta)   and   B_i in the subgroup of order r
// (f the Miller function, FE the final exponentiation).  No random scalars, no product over proofs, no bisection: three Miller loops and
// one final exponentiation per proof, whatever the other proofs are.  The stage (device or host mirror) returns FE(...) and the subgroup
// flag of every proof; e(alpha, beta) is made once per call on the host, by the SAME final exponentiation (zk_fexp_host: the bodies of
// csrc/zkwg_fexp_core.h in the order the device launches them), so no call of zk_pair_final_exp is on this path.
#pragma once
#include "zkwg_fexp_core.h"
#include "zkwg_pair_host.h"

#if !defined(__HIP_DEVICE_COMPILE__)
// steps [first, last) of ZK_FEXP_PROGRAM on one value's slots, as the device launches them
static inline void zk_fexp_run_host(Fq slot[ZK_FEXP_SLOTS][12], u32 first, u32 last) {
  for (u32 k = first; k < last; ++k) {
    const ZkFexpStep& s = ZK_FEXP_PROGRAM[k];
    if (s.op == ZK_FEXP_OP_MUL) zk_fexp_step_value(slot[s.a], slot[s.b], s.pre_a, s.pre_b, s.post, slot[s.dst], 0);
    else if (s.op == ZK_FEXP_OP_NINV) zk_fexp_ninv_value(slot[s.a], slot[s.b], slot[s.dst], 0);
    else zk_fexp_pow_u_value(slot[s.a], slot[s.dst], 0);
  }
}
// FE of the product of the k values at f
static inline Fq12 zk_fexp_host(const Fq12* f, u32 k) {
  Fq slot[ZK_FEXP_SLOTS][12];
  zk_fexp_fold_value((const Fq*)(const void*)f, k, slot[ZK_FEXP_F], 0);
  zk_fexp_run_host(slot, 0, ZK_FEXP_STEPS);
  Fq12 r;
  memcpy((void*)&r, (const void*)slot[ZK_FEXP_OUT], 384);
  return r;
}

// the stage on the host: fe[i] = FE(f(A_i, B_i) f(-vkx_i, gamma) f(-C_i, delta)), inside[i]; x: m x n_public scalars, standard form, below r
static inline int zk_g16_each_host(const ZkG16Key& K, const std::vector<G1Affine>& A, const std::vector<G2Affine>& B, const std::vector<G1Affine>& C,
                                   const std::vector<Fr>& x, std::vector<Fq12>& fe, std::vector<u8>& inside, ZkG16Stats& S) {
  const u64 m = A.size(), np = K.ic.size() - 1;
  fe.resize(m); inside.assign(m, 0);
  std::vector<G1Affine> nvkx(m), terms(np);
  double t = zk_g16_now();
  for (u64 i = 0; i < m; ++i) {
    for (u64 j = 0; j < np; ++j) terms[j] = g1_to_affine(zk_g16_mul(K.ic[j + 1], x[np * i + j]));
    zk_g16_vkx_point(&K.ic[0], terms.data(), (u32)np, &nvkx[i]);
  }
  S.seconds[1] += zk_g16_now() - t; t = zk_g16_now();
  zk_verify_g2_subgroup_host(B.data(), m, inside.data());
  std::vector<Fq12> f(3 * m, fq12_one());
  for (u64 i = 0; i < m; ++i) {
    if (!inside[i]) continue;                                     // (the value of such a proof means nothing: 1 stands in)
    f[3 * i] = zk_pair_miller(A[i], B[i]);
    if (!g1_is_inf(nvkx[i])) f[3 * i + 1] = zk_pair_miller(nvkx[i], K.gamma);
    f[3 * i + 2] = zk_pair_miller(g1_neg(C[i]), K.delta);
  }
  S.seconds[2] += zk_g16_now() - t; t = zk_g16_now();
  for (u64 i = 0; i < m; ++i) fe[i] = zk_fexp_host(&f[3 * i], 3);
  S.seconds[3] += zk_g16_now() - t;
  return ZKWG_RC_OK;
}

// ok[i] = 1 iff proof i verifies.  stage(A, B, C, x, fe, inside) -> rc: the values and flags of the m proofs that passed the host checks.
// S.seconds = {host checks + e(alpha, beta) (+ upload), vkx, Miller + subgroup, final exponentiation, (download +) compare, 0};
// S.counts = {pairs given to the Miller loop, values exponentiated by zkwg_fexp_core.h (the proofs and e(alpha, beta)), proofs excluded
// by the host checks, proofs found bad after them}
template <class Stage>
static inline int zk_g16_verify_each(const ZkG16Key& K, u64 n, const u8* proofs, const u8* publics, u8* ok, Stage stage, ZkG16Stats& S, std::string& err) {
  double t = zk_g16_now();
  int rc = zk_g16_check_key(K, err);
  if (rc != ZKWG_RC_OK) return rc;
  if (!n) return ZKWG_RC_OK;
  const u64 np = K.ic.size() - 1;
  std::vector<u64> idx;
  std::vector<G1Affine> A, C;
  std::vector<G2Affine> B;
  std::vector<Fr> x;
  for (u64 i = 0; i < n; ++i) {
    ok[i] = 0;
    G1Affine a, c;
    G2Affine b;
    bool good = zk_g16_read_proof(proofs + 256 * i, a, b, c);
    const u64 at = x.size();
    for (u64 j = 0; j < np && good; ++j) { Fr v; memcpy(v.l, publics + 32 * (np * i + j), 32); good = !fr_geq(v, fr_p()); x.push_back(v); }
    if (!good) { x.resize(at); ++S.counts[2]; continue; }
    idx.push_back(i); A.push_back(a); B.push_back(b); C.push_back(c);
  }
  const u64 m = idx.size();
  if (!m) { S.seconds[0] += zk_g16_now() - t; return ZKWG_RC_OK; }
  const Fq12 ab = zk_pair_miller(K.alpha, K.beta);
  const Fq12 want = zk_fexp_host(&ab, 1);                        // e(alpha, beta)
  S.counts[0] = 3 * m; S.counts[1] = m + 1;
  S.seconds[0] += zk_g16_now() - t;
  std::vector<Fq12> fe;
  std::vector<u8> inside;
  if ((rc = stage(A, B, C, x, fe, inside)) != ZKWG_RC_OK) return rc;
  t = zk_g16_now();
  for (u64 k = 0; k < m; ++k) {
    const bool good = inside[k] && fq12_eq(fe[k], want);
    ok[idx[k]] = good ? 1 : 0;
    if (!good) ++S.counts[3];
  }
  S.seconds[4] += zk_g16_now() - t;
  return ZKWG_RC_OK;
}
#endif
