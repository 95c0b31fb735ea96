// Host build of csrc/zkwg_pair_core.h and csrc/zkwg_pair_host.h for the CPU tests (tests/test_pair_cpu.py): the Miller loop and the
// subgroup flag as a lane pair of the kernel runs them, the host pairing's pieces on 384-byte values, and batched groth16 verification
// with the leaves made on the host, with the range checks of zkwg_fq29.h counting (ZKWG_FQ29_CHECK).  Test infrastructure only.
#define ZKWG_FQ29_CHECK
#include "zkwg_pair_core.h"
#include "zkwg_pair_host.h"

extern "C" {
unsigned long long pt_violations() { return zk_fq29_violations; }
// the core's Miller value of one pair (points in the zkey's form) and its subgroup flag; -1: a point is not on its curve
int pt_core_miller(const u8* g1, const u8* g2, u8* out, u8* inside) {
  G1Affine p, tp;
  G2Affine q, tq;
  memcpy((void*)&p, g1, 64); memcpy((void*)&q, g2, 128);
  if (!zk_setup_prepare_point_g1(&p, &tp, 0) || !zk_setup_prepare_point_g2(&q, &tq, 0)) return -1;
  Fq f[12];
  *inside = zk_pair_miller_point(&tp, &tq, 0, zk_verify_u_digits(), f) ? 1 : 0;
  memcpy(out, (const void*)f, 384);
  return 0;
}
// the host's Miller value (zkwg_pairing.h); neither point at infinity, q in the subgroup
void pt_host_miller(const u8* g1, const u8* g2, u8* out) {
  G1Affine p;
  G2Affine q;
  memcpy((void*)&p, g1, 64); memcpy((void*)&q, g2, 128);
  const Fq12 f = zk_pair_miller(p, q);
  memcpy(out, (const void*)&f, 384);
}
void pt_final_exp(const u8* in, u8* out) {
  Fq12 f;
  memcpy((void*)&f, in, 384);
  f = zk_pair_final_exp(f);
  memcpy(out, (const void*)&f, 384);
}
// a b by the host's product (core = 0) or by the core's, through its load and store (core = 1)
void pt_f12_mul(const u8* a, const u8* b, int core, u8* out) {
  if (core) {
    Fq x[12], y[12], z[12];
    memcpy((void*)x, a, 384); memcpy((void*)y, b, 384);
    zk_f12_store(z, zk_f12_mul(zk_f12_load(x, 0), zk_f12_load(y, 0)), 0);
    memcpy(out, (const void*)z, 384);
  } else {
    Fq12 x, y;
    memcpy((void*)&x, a, 384); memcpy((void*)&y, b, 384);
    x = fq12_mul(x, y);
    memcpy(out, (const void*)&x, 384);
  }
}
// zkwg_groth16_verify_batch with device = -1, from the same header; key points in the zkey's form (alpha | beta | gamma | delta: 448 bytes)
int pt_verify_batch(const u8* key448, const u8* ic, u32 n_public, u64 n, const u8* proofs, const u8* publics, const u8* rand16, u8* ok,
                    double* seconds, unsigned long long* counts, char* err, u64 err_cap) {
  ZkG16Key K;
  memcpy((void*)&K.alpha, key448, 64); memcpy((void*)&K.beta, key448 + 64, 128); memcpy((void*)&K.gamma, key448 + 192, 128); memcpy((void*)&K.delta, key448 + 320, 128);
  K.ic.resize((u64)n_public + 1);
  memcpy((void*)K.ic.data(), ic, 64 * K.ic.size());
  ZkG16Stats S;
  memset(&S, 0, sizeof S);
  std::string e;
  const int rc = zk_g16_verify_batch(K, n, proofs, publics, rand16, ok, [&](const std::vector<G1Affine>& A, const std::vector<G2Affine>& B, const std::vector<G1Affine>& C,
                                     const u8* r16, ZkG16Leaves& L) { return zk_g16_leaves_host(A, B, C, r16, L, S); }, S, e);
  if (err && err_cap) { strncpy(err, e.c_str(), err_cap - 1); err[err_cap - 1] = 0; }
  for (int i = 0; i < 6; ++i) seconds[i] = S.seconds[i];
  for (int i = 0; i < 4; ++i) counts[i] = S.counts[i];
  return rc;
}
}
