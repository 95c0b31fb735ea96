// Host build of csrc/zkwg_pair_core.h and csrc/zkwg_pair_host.h for the CPU tests (tests/test_pair_cpu.py): the Miller loop and the
// subgroup flag as a lane pair of the kernel runs them, the host pairing's pieces on 384-byte values, and batched groth16 verification
// with the leaves made on the host, with the range checks of zkwg_fq29.h counting (ZKWG_FQ29_CHECK).  Test infrastructure only.
#define ZKWG_FQ29_CHECK
#include "zkwg_pair_core.h"
#include "zkwg_pair_host.h"

extern "C" {
unsigned long long pt_violations() { return zk_fq29_all_violations(); }
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
// One level of the product tree as a lane pair of zk_pair_product runs it (csrc/zkwg_kernels_pair.hip: the same loop, the same claim on the
// accumulator it carries): f = n x 384 bytes, use = n flags or null, out = ceil(n / ZK_PAIR_FOLD) x 384 bytes
void pt_pair_product(const u8* f, const u8* use, u32 n, u8* out) {
  for (u32 j = 0; j < (n + ZK_PAIR_FOLD - 1) / ZK_PAIR_FOLD; ++j) {
    ZkF12 acc = zk_f12_one();
    for (u32 k = 0; k < ZK_PAIR_FOLD; ++k) {
      const u32 i = j * ZK_PAIR_FOLD + k;
      const bool on = i < n && (!use || use[i] != 0);
      Fq w[12];
      memcpy((void*)w, f + 384ull * (on ? i : 0u), 384);
      acc = zk_f12_mul(acc, zk_f12_select(on, zk_f12_load(w, 0), zk_f12_one()));
      ZKF12_CLAIM(acc, 5, 2, ZK_F12_MUL_V5);
    }
    Fq z[12];
    zk_f12_store(z, acc, 0);
    memcpy(out + 384ull * j, (const void*)z, 384);
  }
}
// The pieces of the Miller loop one at a time, standard-form words (32 bytes each, below q) across this boundary; every piece widens its
// operands to its entry claims, so each call is checked from the top of its contract (tests/test_fq29_bounds_cpu.py).
//   op 0  zk_pair_dbl_step   in: T = X, Y, ZZ, ZZZ (8 words), yP, xP                  out: T (8), l0, l1, l3 (6)
//   op 1  zk_pair_add_step   in: T (8), x2, y2 (4), yP, xP                            out: T (8), l0, l1, l3 (6)
//   op 2  zk_f12_sqr         in: f (12)                                               out: 12
//   op 3  zk_f12_mul_line    in: f (12), l0, l1, l3 (6)                               out: 12
//   op 4  zk_f12_mul         in: a (12), b (12)                                       out: 12
void pt_pair_piece(int op, const u8* in, u8* out) {
  typedef ZkF2 F;
  auto rd1 = [&](u32 k) { Fq v; memcpy((void*)&v, in + 32 * k, 32); return zk_q29_base(zk_fq_r256_to_r261(fq_to_mont(v))); };
  auto rd2 = [&](u32 k) { return Fq29x2{{rd1(k), rd1(k + 1)}}; };
  auto wr1 = [&](u32 k, const Fq29& v) { const Fq s = fq_from_mont(fq29_to_fq<2>(fq29_mul(v, fq29_r256()))); memcpy(out + 32 * k, (const void*)&s, 32); };
  auto wr2 = [&](u32 k, const Fq29x2& v) { wr1(k, v.c[0]); wr1(k + 1, v.c[1]); };
  auto rd12 = [&](u32 k) { ZkF12 f; for (u32 i = 0; i < 6; ++i) f.c[i] = rd2(k + 2 * i); return f; };
  auto wr12 = [&](const ZkF12& f) { for (u32 i = 0; i < 6; ++i) wr2(2 * i, f.c[i]); };
  if (op == 0 || op == 1) {
    Xyzz29<F> t{rd2(0), rd2(2), rd2(4), rd2(6)};
    const u32 k = op == 0 ? 8 : 12;
    const Fq29 yP = rd1(k), nxP = fq29_norm(fq29_neg<2, 1>(rd1(k + 1)));
    const ZkPairLine l = op == 0 ? zk_pair_dbl_step(t, yP, nxP) : zk_pair_add_step(t, rd2(8), rd2(10), yP, nxP);
    wr2(0, t.x); wr2(2, t.y); wr2(4, t.zz); wr2(6, t.zzz); wr2(8, l.l0); wr2(10, l.l1); wr2(12, l.l3);
  } else if (op == 2) wr12(zk_f12_sqr(rd12(0)));
  else if (op == 3) wr12(zk_f12_mul_line(rd12(0), ZkPairLine{rd2(12), rd2(14), rd2(16)}));
  else wr12(zk_f12_mul(rd12(0), rd12(12)));
}
void pt_counters(unsigned long long* out) { out[0] = zk_fq29_violations; out[1] = zk_fq29_bound_violations; out[2] = zk_fq29_bound_unsound; }
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
