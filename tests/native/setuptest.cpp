// Host build of csrc/zkwg_setup_core.h for the CPU tests (tests/test_setup_core_cpu.py, tests/test_ptau.py): the ptau walker, the plans and
// the sums the kernels of zkwg_kernels_setup.hip compile, with the range checks of zkwg_fq29.h counting (ZKWG_FQ29_CHECK), and a host
// fixed-base multiply over zkwg_g1.h / zkwg_g2.h that turns a known trapdoor into points.  Test infrastructure only.
#define ZKWG_FQ29_CHECK
#include "zkwg_setup_core.h"

static void st_err(const std::string& e, char* err, u64 cap) {
  if (err && cap) { strncpy(err, e.c_str(), cap - 1); err[cap - 1] = 0; }
}

extern "C" {
unsigned long long st_violations() { return zk_fq29_all_violations(); }
// offsets[5]: tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, tau_g1_next as offsets into the file; points: alpha1 | beta1 | beta2
int st_ptau_parse(const u8* p, u64 len, u32 power, u64* offsets, u8* points, char* err, u64 err_cap) {
  zkwg_setup_slices S;
  std::string e;
  const int rc = zk_ptau_parse(p, len, power, S, e);
  st_err(e, err, err_cap);
  if (rc != ZKWG_RC_OK) return rc;
  const void* q[5] = {S.tau_g1, S.tau_g2, S.alpha_tau_g1, S.beta_tau_g1, S.tau_g1_next};
  for (int i = 0; i < 5; ++i) offsets[i] = (u64)((const u8*)q[i] - p);
  memcpy(points, S.alpha1, 64); memcpy(points + 64, S.beta1, 64); memcpy(points + 128, S.beta2, 128);
  return ZKWG_RC_OK;
}
int st_zkey_new_size(const u8* r1cs, u64 len, u32* power, u64* bytes, char* err, u64 err_cap) {
  ZkR1csHost R;
  if (!zk_r1cs_parse(r1cs, len, R)) { st_err(R.err, err, err_cap); return ZKWG_RC_BAD_CONFIG; }
  ZkSetupShape S;
  std::string e;
  const int rc = zk_setup_shape(R, S, e);
  st_err(e, err, err_cap);
  if (rc != ZKWG_RC_OK) return rc;
  *power = S.power; *bytes = S.zkey_bytes;
  return ZKWG_RC_OK;
}
// the whole set-up on the CPU (host slices); info[7]: zk_setup_host's
int st_zkey_new(const u8* r1cs, u64 len, const zkwg_setup_slices* sl, u8* out, u64 cap, u64* out_len, u64* info, char* err, u64 err_cap) {
  std::string e;
  const int rc = zk_setup_host(r1cs, len, *sl, out, cap, out_len, info, e);
  st_err(e, err, err_cap);
  return rc;
}
// out[i] = k_i G for n standard-form scalars (32 bytes each): group 1 -> 64-byte points, group 2 -> 128-byte points, the zkey's form
void st_fixed_base(int group, const u8* scalars, u64 n, u8* out) {
  std::vector<G1Affine> p1;
  std::vector<G2Affine> p2;
  if (group == 1) {
    G1Xyzz g = g1_from_affine(zk_setup_g1_generator());
    for (int i = 0; i < 254; ++i) { p1.push_back(g1_to_affine(g)); g = g1_dbl(g); }
  } else {
    const G2Affine a = zk_setup_g2_generator();
    G2Xyzz g{a.x, a.y, fq2_one(), fq2_one()};
    for (int i = 0; i < 254; ++i) { p2.push_back(g2_to_affine(g)); g = g2_dbl(g); }
  }
  for (u64 i = 0; i < n; ++i) {
    Fr k;
    memcpy(k.l, scalars + 32 * i, 32);
    if (group == 1) {
      G1Xyzz acc = g1_xyzz_inf();
      for (int b = 0; b < 254; ++b) if ((k.l[b >> 6] >> (b & 63)) & 1) acc = g1_add_mixed(acc, p1[b]);
      const G1Affine r = g1_to_affine(acc);
      memcpy(out + 64 * i, &r, 64);
    } else {
      G2Xyzz acc = g2_xyzz_inf();
      for (int b = 0; b < 254; ++b) if ((k.l[b >> 6] >> (b & 63)) & 1) acc = g2_add_mixed(acc, p2[b]);
      const G2Affine r = g2_to_affine(acc);
      memcpy(out + 128 * i, &r, 128);
    }
  }
}
unsigned st_long_threshold() { return ZK_SETUP_LONG; }
unsigned st_chunk() { return ZK_SETUP_CHUNK; }
}
