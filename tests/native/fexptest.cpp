// Host build of csrc/zkwg_fexp_core.h and csrc/zkwg_fexp_host.h for the CPU tests (tests/test_fexp_cpu.py): the steps of the final
// exponentiation as a lane pair of the kernels runs them, on 384-byte values, the sum of a proof's public-input points, and per-proof
// groth16 verification with its stage on the host -- with the range checks of zkwg_fq29.h counting (ZKWG_FQ29_CHECK).  Test
// infrastructure only.
#define ZKWG_FQ29_CHECK
#include "zkwg_fexp_core.h"
#include "zkwg_fexp_host.h"

namespace {
template <int K, int J> void frob_const(u8* out) {
  const Fq c[2] = {fq_from_mont(fq29_to_fq<2>(fq29_mul(zk_fexp_frob_c<K, J, 0>(), fq29_r256()))), fq_from_mont(fq29_to_fq<2>(fq29_mul(zk_fexp_frob_c<K, J, 1>(), fq29_r256())))};
  memcpy(out, (const void*)c, 64);
}
template <int K> void frob_const_k(int j, u8* out) {
  switch (j) {
    case 0: frob_const<K, 0>(out); break;
    case 1: frob_const<K, 1>(out); break;
    case 2: frob_const<K, 2>(out); break;
    case 3: frob_const<K, 3>(out); break;
    case 4: frob_const<K, 4>(out); break;
    default: frob_const<K, 5>(out); break;
  }
}
Fq29 rd1(const u8* in, u32 k) { Fq v; memcpy((void*)&v, in + 32 * k, 32); return zk_q29_base(zk_fq_r256_to_r261(fq_to_mont(v))); }
Fq29x2 rd2(const u8* in, u32 k) { return Fq29x2{{rd1(in, k), rd1(in, k + 1)}}; }
void wr1(u8* out, u32 k, const Fq29& v) { const Fq s = fq_from_mont(fq29_to_fq<3>(fq29_mul(v, fq29_r256()))); memcpy(out + 32 * k, (const void*)&s, 32); }
void wr2(u8* out, u32 k, const Fq29x2& v) { wr1(out, k, v.c[0]); wr1(out, k + 1, v.c[1]); }
}  // namespace

extern "C" {
void ft_counters(unsigned long long* out) { out[0] = zk_fq29_violations; out[1] = zk_fq29_bound_violations; out[2] = zk_fq29_bound_unsound; }
// the table's xi^(j (q^k - 1) / 6) as two standard-form words
void ft_frob_const(int k, int j, u8* out) {
  if (k == 1) frob_const_k<1>(j, out);
  else if (k == 2) frob_const_k<2>(j, out);
  else frob_const_k<3>(j, out);
}
// One function of csrc/zkwg_fexp_core.h on 384-byte values (Montgomery words), through zk_f12_load and zk_f12_store; each widens its
// operand to its entry claims, so every call is the function from the top of its contract.
//   op 0 zk_fexp_conj   1 .. 3 zk_fexp_frob<op>   4 zk_fexp_cyc_sqr   5 zk_fexp_power_u   6 zk_fexp_ninv (in: n | N, 768 bytes)
//   7 .. 12 zk_fexp_pre with pre = op - 6
void ft_f12_op(int op, const u8* in, u8* out) {
  Fq x[24], z[12];
  memcpy((void*)x, in, op == 6 ? 768 : 384);
  const ZkF12 f = zk_f12_load(x, 0);
  ZkF12 r;
  if (op == 0) r = zk_fexp_conj(f);
  else if (op == 1) r = zk_fexp_frob<1>(f);
  else if (op == 2) r = zk_fexp_frob<2>(f);
  else if (op == 3) r = zk_fexp_frob<3>(f);
  else if (op == 4) r = zk_fexp_cyc_sqr(f);
  else if (op == 5) r = zk_fexp_power_u(f);
  else if (op == 6) r = zk_fexp_ninv(f, zk_f12_load(x + 12, 0));
  else r = zk_fexp_pre(f, (u32)(op - 6));
  zk_f12_store(z, r, 0);
  memcpy(out, (const void*)z, 384);
}
// the small pieces on standard-form words (32 bytes each, below q):
//   op 0 zk_fexp_f2_inv         in: m (2)                 out: 2
//   op 1 zk_fexp_f4_sqr<2>      in: x, y (4)              out: p, m (4)         op 2: <8>
//   op 3 zk_fexp_3p_less_2x     in: p, x (4)              out: 2
//   op 4 zk_fexp_6m_plus_2y     in: m, y (4)              out: 2
//   op 5 zk_fexp_scale          in: f (12), k (2)         out: 12
void ft_piece(int op, const u8* in, u8* out) {
  if (op == 0) wr2(out, 0, zk_fexp_f2_inv(rd2(in, 0)));
  else if (op == 1 || op == 2) {
    Fq29x2 p, m;
    if (op == 1) zk_fexp_f4_sqr<2>(rd2(in, 0), rd2(in, 2), p, m); else zk_fexp_f4_sqr<ZK_F12_MUL_V5>(rd2(in, 0), rd2(in, 2), p, m);
    wr2(out, 0, zk_pair_red(p)); wr2(out, 2, m);
  } else if (op == 3) wr2(out, 0, zk_fexp_3p_less_2x(rd2(in, 0), rd2(in, 2)));
  else if (op == 4) wr2(out, 0, zk_fexp_6m_plus_2y(rd2(in, 0), rd2(in, 2)));
  else {
    ZkF12 f;
    for (u32 i = 0; i < 6; ++i) f.c[i] = rd2(in, 2 * i);
    const ZkF12 r = zk_fexp_scale(f, rd2(in, 12));
    for (u32 i = 0; i < 6; ++i) wr2(out, 2 * i, r.c[i]);
  }
}
// the product of the k values at in (zk_fexp_fold_value), then steps [0, last) of ZK_FEXP_PROGRAM; out = slot `slot` (384 bytes).
// last = 4, slot T1: 1 / f.  last = ZK_FEXP_EASY_STEPS, slot G: the easy part.  last = ZK_FEXP_STEPS, slot OUT: FE.
void ft_program(const u8* in, u32 k, u32 last, u32 slot, u8* out) {
  Fq f[36], s[ZK_FEXP_SLOTS][12];
  memset((void*)s, 0, sizeof s);
  memcpy((void*)f, in, 384ull * k);
  zk_fexp_fold_value(f, k, s[ZK_FEXP_F], 0);
  zk_fexp_run_host(s, 0, last);
  memcpy(out, (const void*)s[slot], 384);
}
// a^e on the host by square-and-multiply (csrc/zkwg_pairing.h fq12_mul); e: n little-endian bytes, not 0
void ft_host_pow(const u8* a, const u8* e, u32 n, u8* out) {
  Fq12 x, r = fq12_one();
  memcpy((void*)&x, a, 384);
  for (int i = 8 * (int)n - 1; i >= 0; --i) {
    r = fq12_mul(r, r);
    if ((e[i >> 3] >> (i & 7)) & 1) r = fq12_mul(r, x);
  }
  memcpy(out, (const void*)&r, 384);
}
// -(ic0 + the n terms), points in the zkey's form
void ft_vkx(const u8* ic0, const u8* terms, u32 n, u8* out) {
  G1Affine a, r;
  std::vector<G1Affine> t(n);
  memcpy((void*)&a, ic0, 64);
  if (n) memcpy((void*)t.data(), terms, 64ull * n);
  zk_g16_vkx_point(&a, t.data(), n, &r);
  memcpy(out, (const void*)&r, 64);
}
// zkwg_groth16_verify_each with device = -1, from the same header; key points in the zkey's form (alpha | beta | gamma | delta: 448 bytes)
int ft_verify_each(const u8* key448, const u8* ic, u32 n_public, u64 n, const u8* proofs, const u8* publics, u8* ok, double* seconds, unsigned long long* counts,
                   char* err, u64 err_cap) {
  ZkG16Key K;
  memcpy((void*)&K.alpha, key448, 64); memcpy((void*)&K.beta, key448 + 64, 128); memcpy((void*)&K.gamma, key448 + 192, 128); memcpy((void*)&K.delta, key448 + 320, 128);
  K.ic.resize((u64)n_public + 1);
  memcpy((void*)K.ic.data(), ic, 64 * K.ic.size());
  ZkG16Stats S;
  memset(&S, 0, sizeof S);
  std::string e;
  const int rc = zk_g16_verify_each(K, n, proofs, publics, ok, [&](const std::vector<G1Affine>& A, const std::vector<G2Affine>& B, const std::vector<G1Affine>& C,
                                    const std::vector<Fr>& x, std::vector<Fq12>& fe, std::vector<u8>& inside) { return zk_g16_each_host(K, A, B, C, x, fe, inside, S); }, S, e);
  if (err && err_cap) { strncpy(err, e.c_str(), err_cap - 1); err[err_cap - 1] = 0; }
  for (int i = 0; i < 6; ++i) seconds[i] = S.seconds[i];
  for (int i = 0; i < 4; ++i) counts[i] = S.counts[i];
  return rc;
}
}
