// Host build of csrc/zkwg_phase2_core.h for the CPU tests (tests/test_phase2_core_cpu.py): the recoder, the scaling series a lane of
// zk_phase2_scale and the set-up's conversion kernels run, and the file operation over it, with the range checks of zkwg_fq29.h counting
// (ZKWG_FQ29_CHECK).  Test infrastructure only.
#define ZKWG_FQ29_CHECK
#include "zkwg_phase2_core.h"

extern "C" {
unsigned long long p2_violations() { return zk_fq29_all_violations(); }
// scalar (32 bytes, little-endian) -> nz[9] | neg[9] | len | n_nz
void p2_recode(const u8* scalar, u32* out) {
  const ZkPhase2Digits D = zk_phase2_recode(scalar);
  memcpy(out, D.nz, 36); memcpy(out + 9, D.neg, 36);
  out[18] = D.len; out[19] = D.n_nz;
}
// out[i] = scalar * in[i], points in the zkey's form; 0, or -1 when a point is not on its curve
int p2_scale(int group, const u8* in, u64 n, const u8* scalar, u8* out) {
  const ZkPhase2Digits D = zk_phase2_recode(scalar);
  bool ok;
  if (group == 1) {
    std::vector<G1Affine> a(n), b(n);
    memcpy((void*)a.data(), in, 64 * n);
    ok = zk_phase2_scale_host<ZkEcG1>(a.data(), n, D, b.data());
    if (ok) memcpy(out, (const void*)b.data(), 64 * n);
  } else {
    std::vector<G2Affine> a(n), b(n);
    memcpy((void*)a.data(), in, 128 * n);
    ok = zk_phase2_scale_host<ZkEcG2>(a.data(), n, D, b.data());
    if (ok) memcpy(out, (const void*)b.data(), 128 * n);
  }
  return ok ? 0 : -1;
}
int p2_apply_size(const u8* z, u64 len, u64 s10_len, u64* bytes, char* err, u64 err_cap) {
  ZkPhase2Frame F;
  std::string e;
  const int rc = zk_phase2_frame(z, len, s10_len, F, e);
  if (err && err_cap) { strncpy(err, e.c_str(), err_cap - 1); err[err_cap - 1] = 0; }
  if (rc == ZKWG_RC_OK) *bytes = F.out_bytes;
  return rc;
}
int p2_apply(const u8* z, u64 len, const u8* k, const u8* s10, u64 s10_len, u8* out, u64 cap, u64* out_len, char* err, u64 err_cap) {
  std::string e;
  const int rc = zk_phase2_apply_host(z, len, k, s10, s10_len, out, cap, out_len, e);
  if (err && err_cap) { strncpy(err, e.c_str(), err_cap - 1); err[err_cap - 1] = 0; }
  return rc;
}
}
