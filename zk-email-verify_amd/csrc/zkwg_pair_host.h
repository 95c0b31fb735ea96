// Batched groth16 verification, the HOST part (include/zkwg.h "checking proofs"): the per-proof checks, the key's checks, the scalar sums,
// the three fixed pairs, the final exponentiation and the bisection.  Shared by csrc/zkwg_pair_api.hip -- which supplies the per-proof
// leaves from the device (csrc/zkwg_pair_core.h) or, for device = -1, from the host mirror below -- and by the host build of the CPU
// tests (tests/native/pairtest.cpp).  Host only; reference call: packages/helpers/src/chunked-zkey.ts:93-101 (snarkjs.groth16.verify).
//
// THE BATCH EQUATION.  Proof i with public inputs x_i is valid iff e(A_i, B_i) = e(alpha, beta) e(vkx_i, gamma) e(C_i, delta),
// vkx_i = IC_0 + sum_j x_ij IC_j.  With random 128-bit r_i != 0 the proofs of a set I are all valid, up to an error of about 2^-128, iff
//     FE( prod_{i in I} f(r_i A_i, B_i) . f(-S0 alpha, beta) . f(-V, gamma) . f(-Cs, delta) ) = 1
//     S0 = sum r_i mod r,   V = S0 IC_0 + sum_j (sum_i r_i x_ij mod r) IC_j,   Cs = sum_i r_i C_i
// (f the Miller function, FE the final exponentiation: zkwg_pairing.h).  That needs every B_i in the subgroup of order r -- outside it the
// pairing is not bilinear and the equation means nothing -- so a proof whose B is outside gets the verdict 0 and stays out of every
// product.  snarkjs does not test this; arkworks does when it deserialises a proof.
//
// THE LEAVES, per proof that passed the host checks: f_i = f(r_i A_i, B_i) (384 bytes), inside_i, and the point r_i C_i.  They are made
// once; a set's check multiplies its f_i, adds its points and recomputes its scalar sums.  The same r_i serve every set: whoever made
// the proofs never sees them.
//
// THE BISECTION.  The whole batch is checked first (1 final exponentiation when every proof is good).  A set that fails is cut in two
// halves: the left half is checked; when it passes, the right half is KNOWN to fail and is not checked, otherwise the left half is known to
// fail and the right half is checked.  A failing set of one proof is a bad proof.  Every set is checked at most once and a failing set costs at
// most 2 checks, so with k bad proofs among n the host makes at most  min(2 n - 1, 1 + 2 k ceil(log2 n))  checks, each 3 Miller loops and
// one final exponentiation.  A batch of mostly bad proofs is slow by design: csrc/zkwg_fexp_host.h (zkwg_groth16_verify_each) is the
// verifier whose work does not depend on the share of bad proofs.
#pragma once
#include <chrono>
#include <functional>
#include <vector>
#include "zkwg_pairing.h"

#if !defined(__HIP_DEVICE_COMPILE__)
struct ZkG16Key {
  G1Affine alpha;
  G2Affine beta, gamma, delta;
  std::vector<G1Affine> ic;            // n_public + 1
};
// the leaves of m proofs; fetch_f fills f (called only when the batch check fails, or by the host mirror at once)
struct ZkG16Leaves {
  std::vector<u8> inside;              // m
  std::vector<G1Affine> rc;            // m: r_i C_i
  Fq12 root;                           // the product of the f_i with inside_i
  std::vector<Fq12> f;                 // m, when fetched
  std::function<int()> fetch_f;
};
struct ZkG16Stats {
  double seconds[6];                   // host checks (+ upload), scalings, Miller + subgroup, product (+ download), the batch check, bisection
  u64 counts[4];                       // pairs the leaves were made of, final exponentiations, proofs excluded by the host checks, proofs found bad after them
};

static inline double zk_g16_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// 32 little-endian bytes, standard form, below q -> Montgomery words; false: not below q
static inline bool zk_g16_fq(const u8* b, Fq& out) {
  Fq v;
  memcpy(v.l, b, 32);
  if (fq_geq(v, fq_p())) return false;
  out = fq_to_mont(v);
  return true;
}
static inline G1Xyzz zk_g16_mul(const G1Affine& p, const Fr& k) {
  G1Xyzz acc = g1_xyzz_inf();
  if (g1_is_inf(p)) return acc;
  for (int b = 255; b >= 0; --b) { acc = g1_dbl(acc); if ((k.l[b >> 6] >> (b & 63)) & 1) acc = g1_add_mixed(acc, p); }
  return acc;
}
static inline Fr zk_g16_fr_mul(const Fr& a, const Fr& b) { return fr_mont_mul(fr_to_mont(a), b); }       // standard x standard -> standard
static inline Fr zk_g16_r(const u8* rand16, u64 i) { Fr k = fr_zero(); memcpy(k.l, rand16 + 16 * i, 16); return k; }

// the key: every point reduced, on its curve and not infinity, the G2 points in the subgroup
static inline int zk_g16_check_key(const ZkG16Key& K, std::string& err) {
  u8 inside[3] = {0, 0, 0};
  const G2Affine g2[3] = {K.beta, K.gamma, K.delta};
  bool ok = zk_setup_prepare_point_g1(&K.alpha, nullptr, 0) && !g1_is_inf(K.alpha);
  for (const G1Affine& p : K.ic) ok = ok && zk_setup_prepare_point_g1(&p, nullptr, 0) && !g1_is_inf(p);
  ok = ok && zk_verify_g2_subgroup_host(g2, 3, inside);
  for (const G2Affine& p : g2) ok = ok && !g2_is_inf(p);
  if (!ok) { err = "verification key: a point is not on its curve (or not reduced, or infinity)"; return ZKWG_RC_BAD_CONFIG; }
  if (!(inside[0] && inside[1] && inside[2])) { err = "verification key: a G2 point is outside the subgroup of order r"; return ZKWG_RC_BAD_CONFIG; }
  return ZKWG_RC_OK;
}
// proof i (256 bytes, standard form) -> points in the zkey's form; false: a coordinate >= q, an all-zero point, a point off its curve
static inline bool zk_g16_read_proof(const u8* p, G1Affine& A, G2Affine& B, G1Affine& C) {
  bool ok = zk_g16_fq(p, A.x) && zk_g16_fq(p + 32, A.y) && zk_g16_fq(p + 64, B.x.c0) && zk_g16_fq(p + 96, B.x.c1) && zk_g16_fq(p + 128, B.y.c0) &&
            zk_g16_fq(p + 160, B.y.c1) && zk_g16_fq(p + 192, C.x) && zk_g16_fq(p + 224, C.y);
  if (!ok || g1_is_inf(A) || g2_is_inf(B) || g1_is_inf(C)) return false;
  return g1_on_curve(A) && g2_on_curve(B) && g1_on_curve(C);
}

// the leaves on the host: the yardstick, and what a machine without a device runs
static inline int zk_g16_leaves_host(const std::vector<G1Affine>& A, const std::vector<G2Affine>& B, const std::vector<G1Affine>& C, const u8* r16,
                                     ZkG16Leaves& L, ZkG16Stats& S) {
  const u64 m = A.size();
  L.inside.assign(m, 0); L.rc.resize(m); L.f.resize(m);
  L.root = fq12_one();
  std::vector<G1Affine> ra(m);
  double t = zk_g16_now();
  for (u64 i = 0; i < m; ++i) { ra[i] = g1_to_affine(zk_g16_mul(A[i], zk_g16_r(r16, i))); L.rc[i] = g1_to_affine(zk_g16_mul(C[i], zk_g16_r(r16, i))); }
  S.seconds[1] += zk_g16_now() - t; t = zk_g16_now();
  zk_verify_g2_subgroup_host(B.data(), m, L.inside.data());
  for (u64 i = 0; i < m; ++i) L.f[i] = L.inside[i] && !g1_is_inf(ra[i]) ? zk_pair_miller(ra[i], B[i]) : fq12_one();
  S.seconds[2] += zk_g16_now() - t; t = zk_g16_now();
  for (u64 i = 0; i < m; ++i) if (L.inside[i]) L.root = fq12_mul(L.root, L.f[i]);
  S.seconds[3] += zk_g16_now() - t;
  L.fetch_f = []() { return (int)ZKWG_RC_OK; };
  return ZKWG_RC_OK;
}

// ok[i] = 1 iff proof i verifies.  leaves(A, B, C, r16 of the m proofs that passed the host checks, L) -> rc makes the leaves.
template <class Leaves>
static inline int zk_g16_verify_batch(const ZkG16Key& K, u64 n, const u8* proofs, const u8* publics, const u8* rand16, u8* ok, Leaves leaves,
                                      ZkG16Stats& S, std::string& err) {
  double t = zk_g16_now();
  int rc = zk_g16_check_key(K, err);
  if (rc != ZKWG_RC_OK) return rc;
  const u64 np = K.ic.size() - 1;
  for (u64 i = 0; i < n; ++i) {
    bool zero = true;
    for (int b = 0; b < 16; ++b) zero = zero && rand16[16 * i + b] == 0;
    if (zero) return ZKWG_RC_BAD_ARG;
  }
  if (!n) return ZKWG_RC_OK;
  // the host checks: idx = the proofs that go on
  std::vector<u64> idx;
  std::vector<G1Affine> A, C;
  std::vector<G2Affine> B;
  std::vector<u8> r16;
  for (u64 i = 0; i < n; ++i) {
    ok[i] = 0;
    G1Affine a, c;
    G2Affine b;
    bool good = zk_g16_read_proof(proofs + 256 * i, a, b, c);
    for (u64 j = 0; j < np && good; ++j) { Fr x; memcpy(x.l, publics + 32 * (np * i + j), 32); good = !fr_geq(x, fr_p()); }
    if (!good) { ++S.counts[2]; continue; }
    idx.push_back(i); A.push_back(a); B.push_back(b); C.push_back(c);
    r16.insert(r16.end(), rand16 + 16 * i, rand16 + 16 * i + 16);
  }
  const u64 m = idx.size();
  S.seconds[0] += zk_g16_now() - t;
  if (!m) return ZKWG_RC_OK;
  ZkG16Leaves L;
  S.counts[0] = m;
  if ((rc = leaves(A, B, C, r16.data(), L)) != ZKWG_RC_OK) return rc;
  t = zk_g16_now();
  // the check of a set [lo, hi) of the m proofs; use_root: the product of its values is L.root (the whole batch)
  auto check = [&](u64 lo, u64 hi, bool use_root) {
    Fq12 f = use_root ? L.root : fq12_one();
    Fr s0 = fr_zero();
    std::vector<Fr> w(np, fr_zero());
    G1Xyzz cs = g1_xyzz_inf();
    for (u64 k = lo; k < hi; ++k) {
      if (!L.inside[k]) continue;
      if (!use_root) f = fq12_mul(f, L.f[k]);
      const Fr r = zk_g16_r(r16.data(), k);
      s0 = fr_add(s0, r);
      for (u64 j = 0; j < np; ++j) { Fr x; memcpy(x.l, publics + 32 * (np * idx[k] + j), 32); w[j] = fr_add(w[j], zk_g16_fr_mul(r, x)); }
      cs = g1_add(cs, g1_from_affine(L.rc[k]));
    }
    G1Xyzz v = zk_g16_mul(K.ic[0], s0);
    for (u64 j = 0; j < np; ++j) v = g1_add(v, zk_g16_mul(K.ic[j + 1], w[j]));
    const G1Affine g1[3] = {g1_neg(g1_to_affine(zk_g16_mul(K.alpha, s0))), g1_neg(g1_to_affine(v)), g1_neg(g1_to_affine(cs))};
    const G2Affine g2[3] = {K.beta, K.gamma, K.delta};
    for (int k = 0; k < 3; ++k) if (!g1_is_inf(g1[k])) f = fq12_mul(f, zk_pair_miller(g1[k], g2[k]));
    ++S.counts[1];
    return fq12_eq(zk_pair_final_exp(f), fq12_one());
  };
  std::vector<u8> good(m, 1);
  for (u64 k = 0; k < m; ++k) if (!L.inside[k]) { good[k] = 0; ++S.counts[3]; }
  const bool all = check(0, m, true);
  S.seconds[4] += zk_g16_now() - t; t = zk_g16_now();
  if (!all) {
    if ((rc = L.fetch_f()) != ZKWG_RC_OK) return rc;
    // [lo, hi) is known to fail
    std::function<void(u64, u64)> split = [&](u64 lo, u64 hi) {
      if (hi - lo == 1) { if (good[lo]) { good[lo] = 0; ++S.counts[3]; } return; }
      const u64 mid = lo + (hi - lo) / 2;
      if (check(lo, mid, false)) { split(mid, hi); return; }
      split(lo, mid);
      if (!check(mid, hi, false)) split(mid, hi);
    };
    split(0, m);
    S.seconds[5] += zk_g16_now() - t;
  }
  for (u64 k = 0; k < m; ++k) ok[idx[k]] = good[k];
  return ZKWG_RC_OK;
}
#endif
