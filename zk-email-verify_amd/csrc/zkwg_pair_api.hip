// C-ABI of batched groth16 verification (include/zkwg.h "checking proofs"): zkwg_miller_device, zkwg_fq12_product_device,
// zkwg_groth16_verify_batch, _stats.  The device makes what grows with the number of proofs and cannot be folded away -- one Miller loop
// per proof (every pi_b is its own), the subgroup flag of that pi_b, the per-proof scalings r_i A_i and r_i C_i (zkwg_point_mul_device) and
// the product tree; the host keeps the per-proof checks, the key's checks, three Miller loops and one final exponentiation per check, and
// the bisection (csrc/zkwg_pair_host.h, which also holds the method and the bound on the number of checks).  One-shot calls like
// zkwg_point_mul_device: they allocate their device buffers, synchronise and free everything before they return.
#include <string.h>
#include <stdio.h>
#include <algorithm>
#include "zkwg_pair_core.h"
#include "zkwg_pair_host.h"
#include "zkwg_points_host.h"

#if !defined(__HIP_DEVICE_COMPILE__)
namespace {
thread_local ZkG16Stats g_stats;

// f[i], inside[i] of n <= ZK_PAIR_MAX pairs in the zkey's form on the device; t1, t2: room for the table-form points; bad: one flag word
int miller(const void* d_g1, const void* d_g2, u32 n, void* t1, void* t2, u32* d_bad, void* d_f, u8* d_inside, hipStream_t st) {
  if (hipMemsetAsync(d_bad, 0, 4, st) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  zk_setup_prepare_launch(1, d_g1, t1, n, d_bad, st);             // the curve checks; -> the tables' form
  zk_setup_prepare_launch(2, d_g2, t2, n, d_bad, st);
  u32 bad = 0;
  if (zk_read_flags(st, d_bad, &bad, 1) != ZKWG_RC_OK) return ZKWG_RC_HIP_ERROR;
  if (bad) return fail(NOT_ON_CURVE);
  zk_pair_miller_launch(t1, t2, n, zk_verify_u_digits(), d_f, d_inside, st);
  return hipGetLastError() == hipSuccess ? ZKWG_RC_OK : ZKWG_RC_HIP_ERROR;
}
// the product of the n values at d_f in use -> root; a, b: room for ceil(n / 4) and ceil(n / 16) values
int product(const void* d_f, const u8* d_use, u32 n, void* a, void* b, Fq12& root, hipStream_t st) {
  const void* src = d_f;
  void* dst = a;
  u32 m = n;
  do {                                                            // (n = 1 takes one level too: the value in use, or 1)
    zk_pair_product_launch(src, d_use, m, dst, st);
    d_use = nullptr;
    m = (m + ZK_PAIR_FOLD - 1) / ZK_PAIR_FOLD;
    src = dst;
    dst = dst == a ? b : a;
  } while (m > 1);
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync((void*)&root, src, 384, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return ZKWG_RC_HIP_ERROR;
  return ZKWG_RC_OK;
}
inline u64 level_bytes(u64 n) { return 384 * ((n + ZK_PAIR_FOLD - 1) / ZK_PAIR_FOLD); }

// the leaves of m proofs on the device
int leaves_device(int device, const std::vector<G1Affine>& A, const std::vector<G2Affine>& B, const std::vector<G1Affine>& C, const u8* r16, ZkG16Leaves& L,
                  DevBufs& D) {
  const u64 m = A.size();
  if (m > ZK_PAIR_MAX) return ZKWG_RC_BAD_ARG;
  if (hipSetDevice(device) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  hipStream_t st = nullptr;
  ZkStageClock clock(st, g_stats.seconds);
  void *dA = D.get(64 * m), *dC = D.get(64 * m), *dB = D.get(128 * m), *r = D.get(16 * m), *r32 = D.get(32 * m);
  void *t1 = D.get(64 * m), *t2 = D.get(128 * m), *f = D.get(384 * m), *pa = D.get(level_bytes(m)), *pb = D.get(level_bytes(level_bytes(m) / 384));
  u8* inside = (u8*)D.get(m);
  u32* d_bad = (u32*)D.get(4);
  if (D.oom) return ZKWG_RC_OOM;
  if (hipMemcpyAsync(dA, A.data(), 64 * m, hipMemcpyHostToDevice, st) != hipSuccess || hipMemcpyAsync(dC, C.data(), 64 * m, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(dB, B.data(), 128 * m, hipMemcpyHostToDevice, st) != hipSuccess || hipMemcpyAsync(r, r16, 16 * m, hipMemcpyHostToDevice, st) != hipSuccess)
    return ZKWG_RC_HIP_ERROR;
  zk_verify_widen_launch(r, r32, m, st);
  if (!clock.lap(0)) return ZKWG_RC_HIP_ERROR;
  int rc = zkwg_point_mul_device(device, 1, dA, m, r32, dA, st);
  if (rc == ZKWG_RC_OK) rc = zkwg_point_mul_device(device, 1, dC, m, r32, dC, st);
  if (rc != ZKWG_RC_OK) return rc;
  if (!clock.lap(1)) return ZKWG_RC_HIP_ERROR;
  if ((rc = miller(dA, dB, (u32)m, t1, t2, d_bad, f, inside, st)) != ZKWG_RC_OK) return rc;
  if (!clock.lap(2)) return ZKWG_RC_HIP_ERROR;
  if ((rc = product(f, inside, (u32)m, pa, pb, L.root, st)) != ZKWG_RC_OK) return rc;
  L.inside.resize(m); L.rc.resize(m);
  if (hipMemcpy(L.inside.data(), inside, m, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy((void*)L.rc.data(), dC, 64 * m, hipMemcpyDeviceToHost) != hipSuccess)
    return ZKWG_RC_HIP_ERROR;
  if (!clock.lap(3)) return ZKWG_RC_HIP_ERROR;
  L.fetch_f = [&L, f, m]() {
    L.f.resize(m);
    return hipMemcpy((void*)L.f.data(), f, 384 * m, hipMemcpyDeviceToHost) == hipSuccess ? (int)ZKWG_RC_OK : (int)ZKWG_RC_HIP_ERROR;
  };
  return ZKWG_RC_OK;
}
}  // namespace

extern "C" {

int zkwg_miller_device(int device, const void* d_g1, const void* d_g2, uint64_t n, void* d_f, uint8_t* d_inside, void* hip_stream) {
  if (n > ZK_PAIR_MAX || (n && (!d_g1 || !d_g2 || !d_f || !d_inside)) || ((uintptr_t)d_g1 & 15) || ((uintptr_t)d_g2 & 15) || ((uintptr_t)d_f & 15)) return ZKWG_RC_BAD_ARG;
  if (device < 0) return ZKWG_RC_NO_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  if (!n) return ZKWG_RC_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  DevBufs D;
  void *t1 = D.get(64 * n), *t2 = D.get(128 * n);
  u32* d_bad = (u32*)D.get(4);
  if (D.oom) return ZKWG_RC_OOM;
  const int rc = miller(d_g1, d_g2, (u32)n, t1, t2, d_bad, d_f, d_inside, st);
  if (rc != ZKWG_RC_OK) return rc;
  return hipStreamSynchronize(st) == hipSuccess ? ZKWG_RC_OK : ZKWG_RC_HIP_ERROR;
}

int zkwg_fq12_product_device(int device, const void* d_f, const uint8_t* d_use, uint64_t n, uint8_t* out, void* hip_stream) {
  if (n > ZK_PAIR_MAX || !out || (n && !d_f) || ((uintptr_t)d_f & 15)) return ZKWG_RC_BAD_ARG;
  if (device < 0) return ZKWG_RC_NO_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  Fq12 root = fq12_one();
  if (n) {
    DevBufs D;
    void *a = D.get(level_bytes(n)), *b = D.get(level_bytes(level_bytes(n) / 384));
    if (D.oom) return ZKWG_RC_OOM;
    const int rc = product(d_f, d_use, (u32)n, a, b, root, (hipStream_t)hip_stream);
    if (rc != ZKWG_RC_OK) return rc;
  }
  memcpy(out, (const void*)&root, 384);
  return ZKWG_RC_OK;
}

int zkwg_groth16_verify_batch(int device, const zkwg_verification_key* vk, uint64_t n, const uint8_t* proofs, const uint8_t* publics, const uint8_t* rand16, uint8_t* ok) {
  if (!vk || !vk->ic || (n && (!proofs || !ok || (vk->n_public && !publics))) || n > ZK_PAIR_MAX) return ZKWG_RC_BAD_ARG;
  try {
    memset(&g_stats, 0, sizeof g_stats);
    ZkG16Key K;
    memcpy((void*)&K.alpha, vk->alpha1, 64); memcpy((void*)&K.beta, vk->beta2, 128); memcpy((void*)&K.gamma, vk->gamma2, 128); memcpy((void*)&K.delta, vk->delta2, 128);
    K.ic.resize((u64)vk->n_public + 1);
    memcpy((void*)K.ic.data(), vk->ic, 64 * K.ic.size());
    std::vector<u8> drawn;
    if (!rand16 && n) {                                           // from the operating system; a zero entry (2^-128) is drawn again
      drawn.resize(16 * n);
      FILE* f = fopen("/dev/urandom", "rb");
      bool got = f != nullptr;
      for (u64 i = 0; i < n && got; ++i) {
        bool zero = true;
        while (zero && got) {
          got = fread(drawn.data() + 16 * i, 1, 16, f) == 16;
          for (int b = 0; b < 16; ++b) zero = zero && drawn[16 * i + b] == 0;
        }
      }
      if (f) fclose(f);
      if (!got) { zk_set_last_error("groth16 verify: the operating system gave no random bytes"); return ZKWG_RC_HIP_ERROR; }
      rand16 = drawn.data();
    }
    std::string err;
    DevBufs bufs;                                                 // (freed when the call returns, after the bisection's download)
    const int rc = zk_g16_verify_batch(K, n, proofs, publics, rand16, ok, [&](const std::vector<G1Affine>& A, const std::vector<G2Affine>& B, const std::vector<G1Affine>& C,
                                       const u8* r16, ZkG16Leaves& L) {
      if (device < 0) return zk_g16_leaves_host(A, B, C, r16, L, g_stats);
      return leaves_device(device, A, B, C, r16, L, bufs);
    }, g_stats, err);
    if (rc == ZKWG_RC_BAD_CONFIG && !err.empty()) return fail(err);
    return rc;
  } catch (const std::bad_alloc&) {
    return ZKWG_RC_OOM;
  }
}

void zkwg_groth16_verify_stats(double seconds[6], uint64_t counts[4]) {
  if (seconds) for (int i = 0; i < 6; ++i) seconds[i] = g_stats.seconds[i];
  if (counts) for (int i = 0; i < 4; ++i) counts[i] = g_stats.counts[i];
}

}
#endif
