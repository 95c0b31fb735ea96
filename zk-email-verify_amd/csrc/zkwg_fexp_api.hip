// C-ABI of per-proof groth16 verification (include/zkwg.h "checking proofs"): zkwg_final_exp_device, zkwg_groth16_verify_each, _stats.
// The device runs everything that grows with the number of proofs: the scalings x_ij IC_j (zkwg_point_mul_device), their sum made affine
// (zk_g16_vkx), three Miller loops per proof (zkwg_miller_device) and the final exponentiation of their product (zk_fexp_fold, then the 22
// launches of ZK_FEXP_PROGRAM: csrc/zkwg_fexp_core.h); the host keeps the per-proof checks, the key's checks, e(alpha,
// beta) and the comparison (csrc/zkwg_fexp_host.h).  One-shot calls like zkwg_miller_device: they allocate their device buffers,
// synchronise and free everything before they return.
#include <string.h>
#include <algorithm>
#include "zkwg_fexp_core.h"
#include "zkwg_fexp_host.h"
#include "zkwg_points_host.h"

#if !defined(__HIP_DEVICE_COMPILE__)
namespace {
thread_local ZkG16Stats g_stats;

#define ZK_G16_EACH_PIECE (ZK_PAIR_MAX / 3)         // proofs per series of launches: their 3 pairs fit one Miller launch

// the values the program works on, n x 384 bytes each; OUT is the caller's, and so is F when a value is one value (k = 1)
struct Slots {
  void* p[ZK_FEXP_SLOTS];
  Slots(DevBufs& D, u64 n, const void* f, u32 k, void* out) {
    for (int s = 0; s < ZK_FEXP_SLOTS; ++s) p[s] = s == ZK_FEXP_OUT ? out : s == ZK_FEXP_F && k == 1 ? (void*)f : D.get(384 * n);
  }
};
// out[i] = FE(f[k i] .. f[k i + k - 1]) for n <= ZK_FEXP_MAX values
int fexp(const void* d_f, u32 n, u32 k, const Slots& S, hipStream_t st) {
  if (k != 1) zk_fexp_fold_launch(d_f, n, k, S.p[ZK_FEXP_F], st);
  for (const ZkFexpStep& s : ZK_FEXP_PROGRAM) {
    if (s.op == ZK_FEXP_OP_MUL) zk_fexp_step_launch(S.p[s.a], S.p[s.b], n, s.pre_a, s.pre_b, s.post, S.p[s.dst], st);
    else if (s.op == ZK_FEXP_OP_NINV) zk_fexp_ninv_launch(S.p[s.a], S.p[s.b], n, S.p[s.dst], st);
    else zk_fexp_pow_u_launch(S.p[s.a], n, S.p[s.dst], st);
  }
  return hipGetLastError() == hipSuccess ? ZKWG_RC_OK : ZKWG_RC_HIP_ERROR;
}

// the stage of proofs [first, first + m) on the device
int piece(int device, const ZkG16Key& K, const G1Affine* A, const G2Affine* B, const G1Affine* C, const Fr* x, u64 m, Fq12* fe, u8* inside) {
  const u64 np = K.ic.size() - 1;
  hipStream_t st = nullptr;
  ZkStageClock clock(st, g_stats.seconds);
  std::vector<G1Affine> g1(3 * m), terms(np * m);
  std::vector<G2Affine> g2(3 * m);
  for (u64 i = 0; i < m; ++i) {
    g1[3 * i] = A[i]; g1[3 * i + 1] = G1Affine{fq_zero(), fq_zero()}; g1[3 * i + 2] = g1_neg(C[i]);
    g2[3 * i] = B[i]; g2[3 * i + 1] = K.gamma; g2[3 * i + 2] = K.delta;
    for (u64 j = 0; j < np; ++j) terms[np * i + j] = K.ic[j + 1];
  }
  DevBufs D;
  void *d_g1 = D.get(64 * 3 * m), *d_g2 = D.get(128 * 3 * m), *d_terms = D.get(64 * np * m), *d_x = D.get(32 * np * m), *d_ic0 = D.get(64);
  void *d_f = D.get(384 * 3 * m), *d_out = D.get(384 * m);
  u8* d_inside = (u8*)D.get(3 * m);
  const Slots S(D, m, d_f, 3, d_out);
  if (D.oom) return ZKWG_RC_OOM;
  if (hipMemcpyAsync(d_g1, g1.data(), 64 * 3 * m, hipMemcpyHostToDevice, st) != hipSuccess || hipMemcpyAsync(d_g2, g2.data(), 128 * 3 * m, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(d_ic0, &K.ic[0], 64, hipMemcpyHostToDevice, st) != hipSuccess ||
      (np && (hipMemcpyAsync(d_terms, terms.data(), 64 * np * m, hipMemcpyHostToDevice, st) != hipSuccess || hipMemcpyAsync(d_x, x, 32 * np * m, hipMemcpyHostToDevice, st) != hipSuccess)) ||
      hipStreamSynchronize(st) != hipSuccess)
    return ZKWG_RC_HIP_ERROR;
  if (!clock.lap(0)) return ZKWG_RC_HIP_ERROR;
  int rc = np ? zkwg_point_mul_device(device, 1, d_terms, np * m, d_x, d_terms, st) : ZKWG_RC_OK;
  if (rc != ZKWG_RC_OK) return rc;
  zk_g16_vkx_launch(d_ic0, d_terms, (u32)np, (u32)m, d_g1, st);
  if (!clock.lap(1)) return ZKWG_RC_HIP_ERROR;
  if ((rc = zkwg_miller_device(device, d_g1, d_g2, 3 * m, d_f, d_inside, st)) != ZKWG_RC_OK) return rc;
  if (!clock.lap(2)) return ZKWG_RC_HIP_ERROR;
  if ((rc = fexp(d_f, (u32)m, 3, S, st)) != ZKWG_RC_OK) return rc;
  if (!clock.lap(3)) return ZKWG_RC_HIP_ERROR;
  std::vector<u8> ins(3 * m);
  if (hipMemcpyAsync((void*)fe, d_out, 384 * m, hipMemcpyDeviceToHost, st) != hipSuccess || hipMemcpyAsync(ins.data(), d_inside, 3 * m, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return ZKWG_RC_HIP_ERROR;
  for (u64 i = 0; i < m; ++i) inside[i] = ins[3 * i];            // (gamma and delta are inside: the key's check)
  return clock.lap(4) ? ZKWG_RC_OK : ZKWG_RC_HIP_ERROR;
}
}  // namespace

extern "C" {

int zkwg_final_exp_device(int device, const void* d_f, uint64_t n, void* d_out, void* hip_stream) {
  if (n > ZK_FEXP_MAX || (n && (!d_f || !d_out)) || ((uintptr_t)d_f & 15) || ((uintptr_t)d_out & 15)) return ZKWG_RC_BAD_ARG;
  if (device < 0) return ZKWG_RC_NO_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  if (!n) return ZKWG_RC_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  DevBufs D;
  const Slots S(D, n, d_f, 1, d_out);
  if (D.oom) return ZKWG_RC_OOM;
  const int rc = fexp(d_f, (u32)n, 1, S, st);
  if (rc != ZKWG_RC_OK) return rc;
  return hipStreamSynchronize(st) == hipSuccess ? ZKWG_RC_OK : ZKWG_RC_HIP_ERROR;
}

int zkwg_groth16_verify_each(int device, const zkwg_verification_key* vk, uint64_t n, const uint8_t* proofs, const uint8_t* publics, uint8_t* ok) {
  if (!vk || !vk->ic || (n && (!proofs || !ok || (vk->n_public && !publics))) || n > ZK_PAIR_MAX) return ZKWG_RC_BAD_ARG;
  try {
    memset(&g_stats, 0, sizeof g_stats);
    ZkG16Key K;
    memcpy((void*)&K.alpha, vk->alpha1, 64); memcpy((void*)&K.beta, vk->beta2, 128); memcpy((void*)&K.gamma, vk->gamma2, 128); memcpy((void*)&K.delta, vk->delta2, 128);
    K.ic.resize((u64)vk->n_public + 1);
    memcpy((void*)K.ic.data(), vk->ic, 64 * K.ic.size());
    std::string err;
    const int rc = zk_g16_verify_each(K, n, proofs, publics, ok, [&](const std::vector<G1Affine>& A, const std::vector<G2Affine>& B, const std::vector<G1Affine>& C,
                                      const std::vector<Fr>& x, std::vector<Fq12>& fe, std::vector<u8>& inside) {
      if (device < 0) return zk_g16_each_host(K, A, B, C, x, fe, inside, g_stats);
      if (hipSetDevice(device) != hipSuccess) return (int)ZKWG_RC_HIP_ERROR;
      const u64 m = A.size(), np = K.ic.size() - 1;
      fe.resize(m); inside.assign(m, 0);
      // a piece's pairs fit one Miller launch, and its n_public m scaled points stay near 2^20
      const u64 step = std::max<u64>(1, std::min<u64>(ZK_G16_EACH_PIECE, np ? ZK_PAIR_MAX / np : ZK_G16_EACH_PIECE));
      for (u64 first = 0; first < m; first += step) {
        const u64 cm = std::min<u64>(step, m - first);
        const int r = piece(device, K, A.data() + first, B.data() + first, C.data() + first, x.data() + np * first, cm, fe.data() + first, inside.data() + first);
        if (r != ZKWG_RC_OK) return r;
      }
      return (int)ZKWG_RC_OK;
    }, g_stats, err);
    if (rc == ZKWG_RC_BAD_CONFIG && !err.empty()) return fail(err);
    return rc;
  } catch (const std::bad_alloc&) {
    return ZKWG_RC_OOM;
  }
}

void zkwg_groth16_verify_each_stats(double seconds[6], uint64_t counts[4]) {
  if (seconds) for (int i = 0; i < 6; ++i) seconds[i] = g_stats.seconds[i];
  if (counts) for (int i = 0; i < 4; ++i) counts[i] = g_stats.counts[i];
}

}
#endif
