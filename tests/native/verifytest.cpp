// Host build of csrc/zkwg_verify_core.h and csrc/zkwg_pairing.h for the CPU tests (tests/test_verify_cpu.py): the G2 subgroup test as a
// lane pair of the kernel runs it, the pairing product, and the ratio sums as plain host sums, with the range checks of zkwg_fq29.h
// counting (ZKWG_FQ29_CHECK).  Test infrastructure only.
#define ZKWG_FQ29_CHECK
#include "zkwg_pairing.h"

static void vt_err(const std::string& e, char* err, u64 cap) {
  if (err && cap) { strncpy(err, e.c_str(), cap - 1); err[cap - 1] = 0; }
}

extern "C" {
unsigned long long vt_violations() { return zk_fq29_all_violations(); }
// the digits of u: positions and non-zero digits of the shared walk
void vt_u_digits(u32* len, u32* n_nz) { const ZkPhase2Digits D = zk_verify_u_digits(); *len = D.len; *n_nz = D.n_nz; }
// inside[i] = 1 when point i (the zkey's form) is in the subgroup of order r; 0, or -1 when a point is not on the curve
int vt_g2_subgroup(const u8* pts, u64 n, u8* inside) {
  std::vector<G2Affine> a(n);
  memcpy((void*)a.data(), pts, 128 * n);
  return zk_verify_g2_subgroup_host(a.data(), n, inside) ? 0 : -1;
}
// out: the product of the reduced pairings, 6 Fq2 coefficients of w^0 .. w^5 (w^6 = 9 + i), standard form, 12 x 32 bytes
int vt_pairing(const u8* g1, const u8* g2, u32 n, u8* out, char* err, u64 err_cap) {
  Fq12 f;
  std::string e;
  const int rc = zk_pairing_product(g1, g2, n, f, e);
  vt_err(e, err, err_cap);
  if (rc != ZKWG_RC_OK) return rc;
  for (int k = 0; k < 6; ++k) {
    const Fq c0 = fq_from_mont(f.c[k].c0), c1 = fq_from_mont(f.c[k].c1);
    memcpy(out + 64 * k, c0.l, 32); memcpy(out + 64 * k + 32, c1.l, 32);
  }
  return rc;
}
int vt_pairing_check(const u8* g1, const u8* g2, u32 n, int* is_one, char* err, u64 err_cap) {
  Fq12 f;
  std::string e;
  const int rc = zk_pairing_product(g1, g2, n, f, e);
  vt_err(e, err, err_cap);
  if (rc == ZKWG_RC_OK) *is_one = fq12_eq(f, fq12_one()) ? 1 : 0;
  return rc;
}
// out = sum_i s_i P_i over n points of one group (the zkey's form; s_i: scalar_bytes little-endian bytes each) by plain double-and-add
// over the canonical-word formulas: what zkwg_point_rlc_device must equal.  0, or -1 when a point is not on its curve
int vt_rlc(int group, const u8* pts, u64 n, const u8* scalars, u32 scalar_bytes, u8* out) {
  G1Xyzz s1 = g1_xyzz_inf();
  G2Xyzz s2 = g2_xyzz_inf();
  for (u64 i = 0; i < n; ++i) {
    const u8* k = scalars + (u64)scalar_bytes * i;
    if (group == 1) {
      G1Affine p;
      memcpy((void*)&p, pts + 64 * i, 64);
      if (!zk_setup_prepare_point_g1(&p, nullptr, 0)) return -1;
      G1Xyzz acc = g1_xyzz_inf();
      for (int b = 8 * (int)scalar_bytes - 1; b >= 0; --b) { acc = g1_dbl(acc); if ((k[b >> 3] >> (b & 7)) & 1) acc = g1_add_mixed(acc, p); }
      s1 = g1_add(s1, acc);
    } else {
      G2Affine p;
      memcpy((void*)&p, pts + 128 * i, 128);
      if (!zk_setup_prepare_point_g2(&p, nullptr, 0)) return -1;
      G2Xyzz acc = g2_xyzz_inf();
      for (int b = 8 * (int)scalar_bytes - 1; b >= 0; --b) { acc = g2_dbl(acc); if ((k[b >> 3] >> (b & 7)) & 1) acc = g2_add_mixed(acc, p); }
      s2 = g2_add(s2, acc);
    }
  }
  if (group == 1) { const G1Affine a = g1_to_affine(s1); memcpy(out, (const void*)&a, 64); }
  else { const G2Affine a = g2_to_affine(s2); memcpy(out, (const void*)&a, 128); }
  return 0;
}
}
