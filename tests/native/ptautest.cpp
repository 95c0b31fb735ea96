// Host build of csrc/zkwg_ptau_core.h for the CPU tests (tests/test_ptau_prepare_cpu.py): the twiddle recoder, the transform over points
// as the launch series of zkwg_group_ntt_device runs it, and the file operation over it, with the range checks of zkwg_fq29.h counting
// (ZKWG_FQ29_CHECK).  Test infrastructure only.
#define ZKWG_FQ29_CHECK
#include "zkwg_ptau_core.h"

static void pt_err(const std::string& e, char* err, u64 cap) {
  if (err && cap) { strncpy(err, e.c_str(), cap - 1); err[cap - 1] = 0; }
}

extern "C" {
unsigned long long pt_violations() { return zk_fq29_all_violations(); }
// the table of a 2^L-point transform: out = 2^(L - 1) entries of nz[8] | neg[8] (one entry for L = 0)
void pt_table(u32 L, int inverse, u32* out) {
  ZkPtauTable T;
  zk_ptau_table(L, inverse != 0, T);
  memcpy(out, T.tw.data(), T.tw.size() * sizeof(ZkPtauTw));
}
// 2^L points in the zkey's form, in place; 0, or -1 when a point is not on its curve
int pt_ntt(int group, u8* pts, u32 L, int inverse) {
  const u64 n = 1ull << L;
  bool ok;
  if (group == 1) {
    std::vector<G1Affine> a(n);
    memcpy((void*)a.data(), pts, 64 * n);
    ok = zk_ptau_ntt_host<ZkEcG1>(a.data(), L, inverse != 0);
    if (ok) memcpy(pts, (const void*)a.data(), 64 * n);
  } else {
    std::vector<G2Affine> a(n);
    memcpy((void*)a.data(), pts, 128 * n);
    ok = zk_ptau_ntt_host<ZkEcG2>(a.data(), L, inverse != 0);
    if (ok) memcpy(pts, (const void*)a.data(), 128 * n);
  }
  return ok ? 0 : -1;
}
int pt_prepare_size(const u8* p, u64 len, u32 power, u64* bytes, char* err, u64 err_cap) {
  ZkPtauFrame F;
  std::string e;
  const int rc = zk_ptau_frame(p, len, power, F, e);
  pt_err(e, err, err_cap);
  if (rc == ZKWG_RC_OK) *bytes = F.out_bytes;
  return rc;
}
int pt_prepare(const u8* p, u64 len, u32 power, u8* out, u64 cap, u64* out_len, char* err, u64 err_cap) {
  std::string e;
  const int rc = zk_ptau_prepare_host(p, len, power, out, cap, out_len, e);
  pt_err(e, err, err_cap);
  return rc;
}
}
