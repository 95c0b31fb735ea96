// Host build of csrc/zkwg_ptau_key_core.h for the CPU tests (tests/test_ptau_key_cpu.py): the regular recoding, the per-lane scalars
// c t^k, "each point times its own scalar" as the launch series of zkwg_point_mul_device runs it, and the file operation over it, with the
// range checks of zkwg_fq29.h and zkwg_fr29.h counting (ZKWG_FQ29_CHECK, ZKWG_FR29_CHECK).  Test infrastructure only.
#define ZKWG_FQ29_CHECK
#define ZKWG_FR29_CHECK
#include "zkwg_ptau_key_core.h"

static void pk_err(const std::string& e, char* err, u64 cap) {
  if (err && cap) { strncpy(err, e.c_str(), cap - 1); err[cap - 1] = 0; }
}

extern "C" {
unsigned long long pk_violations() { return zk_fq29_all_violations() + zk_fr29_violations; }
u32 pk_window() { return ZK_KEY_W; }
// k (32 bytes, below r) -> out[0 .. 64): the digits from the LEAST significant window up, as the walk reads them; out[64]: 1 when P is subtracted
void pk_recode(const u8* k32, int* out) {
  Fr k;
  memcpy(k.l, k32, 32);
  ZkKeyScalar S = zk_key_recode(k);
  out[ZK_KEY_DIGITS] = (int)S.even;
  for (int i = (int)ZK_KEY_DIGITS - 1; i >= 0; --i) {
    const ZkKeyDigit g = zk_key_pop(S);
    out[i] = (g.neg ? -1 : 1) * (int)(2 * g.row + 1);
  }
}
// out[k] = c t^(first + k) mod r, k < n (32 bytes each); -1: c or t is 0 modulo r
int pk_powers(const u8* c32, const u8* t32, u64 first, u64 n, u8* out) {
  ZkKeyPowers T;
  if (!zk_key_powers_table(c32, t32, T)) return -1;
  for (u64 k = 0; k < n; ++k) {
    const Fr s = zk_key_power_scalar(&T, first + k, zk_key_bits(first + n - 1));
    memcpy(out + 32 * k, s.l, 32);
  }
  return 0;
}
// out[i] = scalars[i] in[i], n points in the zkey's form; 0, or -1 when a point is not on its curve
int pk_mul(int group, const u8* pts, u64 n, const u8* scalars, u8* out, u64 piece) {
  auto scalar = [&](u64 i) { Fr k; memcpy(k.l, scalars + 32 * i, 32); return zk_key_reduce(k); };
  bool ok;
  if (group == 1) {
    std::vector<G1Affine> a(n), b(n);
    memcpy((void*)a.data(), pts, 64 * n);
    ok = zk_key_mul_host<ZkEcG1>(a.data(), n, scalar, b.data(), piece);
    if (ok) memcpy(out, (const void*)b.data(), 64 * n);
  } else {
    std::vector<G2Affine> a(n), b(n);
    memcpy((void*)a.data(), pts, 128 * n);
    ok = zk_key_mul_host<ZkEcG2>(a.data(), n, scalar, b.data(), piece);
    if (ok) memcpy(out, (const void*)b.data(), 128 * n);
  }
  return ok ? 0 : -1;
}
int pk_apply_key_size(const u8* p, u64 len, u64 s7_len, u64* bytes, char* err, u64 err_cap) {
  ZkPtauKeyFrame F;
  std::string e;
  const int rc = zk_ptau_key_frame(p, len, s7_len, F, e);
  pk_err(e, err, err_cap);
  if (rc == ZKWG_RC_OK) *bytes = F.out_bytes;
  return rc;
}
int pk_apply_key(const u8* p, u64 len, const u8* tau, const u8* alpha, const u8* beta, const u8* s7, u64 s7_len, u8* out, u64 cap, u64* out_len, u64 piece,
                 char* err, u64 err_cap) {
  std::string e;
  const int rc = zk_ptau_apply_key_host(p, len, tau, alpha, beta, s7, s7_len, out, cap, out_len, piece, e);
  pk_err(e, err, err_cap);
  return rc;
}
}
