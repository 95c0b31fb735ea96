// C-ABI of the transform stage (include/zkwg.h "prover stage 2"): plans (twiddle / coset tables built on the host once per
// domain size), stand-alone transforms, and the H-evaluation pipeline of groth16_prove.js over a batch of emails.
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include "../../include/zkwg.h"
#include "zkwg_ntt_core.h"

extern "C" int zk_ntt_launch(int dit, const Fr* src, u64 src_es, u64 src_ps, u64 valid, int src_lazy, void* work, Fr* out, const Fr* tw, const Fr* scale,
                             const Fr* uni_host, u32 L, u32 n_polys, u32 inv, hipStream_t st);
extern "C" int zk_ntt_join_launch(const void* work, Fr* out, u64 n, u64 out_es, u32 n_emails, hipStream_t st);
extern "C" int zk_ntt_bitrev_launch(Fr* data, u32 L, u32 n_polys, hipStream_t st);

struct zkwg_ntt {
  int device;
  u32 L;
  u64 n;
  // The tables are in 2^261-Montgomery form (canonical words): the kernels keep values in 9 x 29-bit limb form (zkwg_fr29.h), whose
  // product divides by 2^261; the DATA stay in the callers' 2^256 form (one operand in 2^261 form is what a product needs).
  Fr* d_tw;       // w^k, k < n; w = Fr.w[L] of ffjavascript (nqr = 5)
  Fr* d_scale;    // position p (bit-reversed coefficient index): inc^bitrev(p) / n
  Fr ninv_m;      // 1 / n
};

extern "C" {

int zkwg_ntt_create(int device, uint32_t log2_n, zkwg_ntt_t** out) {
  if (!out || log2_n < 2 || log2_n > 26) return ZKWG_RC_BAD_ARG;
  try {
    zkwg_ntt* p = new zkwg_ntt();
    p->device = device; p->L = log2_n; p->n = 1ull << log2_n; p->d_tw = p->d_scale = nullptr;
    std::vector<Fr> tw, sc;
    if (!zk_ntt_tables(log2_n, tw, sc, p->ninv_m)) { delete p; return ZKWG_RC_BAD_CONFIG; }   // (zkwg_ntt_core.h: shared with the host mirror)
    if (device >= 0) {
      if (hipSetDevice(device) != hipSuccess) { delete p; return ZKWG_RC_NO_DEVICE; }
      if (hipMalloc((void**)&p->d_tw, p->n * sizeof(Fr)) != hipSuccess || hipMalloc((void**)&p->d_scale, p->n * sizeof(Fr)) != hipSuccess ||
          hipMemcpy(p->d_tw, tw.data(), p->n * sizeof(Fr), hipMemcpyHostToDevice) != hipSuccess ||
          hipMemcpy(p->d_scale, sc.data(), p->n * sizeof(Fr), hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(p->d_tw); hipFree(p->d_scale); delete p;
        return ZKWG_RC_OOM;
      }
    }
    *out = p;
    return ZKWG_RC_OK;
  } catch (const std::bad_alloc&) {
    return ZKWG_RC_OOM;
  }
}
void zkwg_ntt_destroy(zkwg_ntt_t* p) {
  if (!p) return;
  if (p->device >= 0) { hipSetDevice(p->device); hipFree(p->d_tw); hipFree(p->d_scale); }
  delete p;
}
uint64_t zkwg_ntt_domain(const zkwg_ntt_t* p) { return p ? p->n : 0; }
// three polynomials per email in planar limb form: 16 + 16 + 4 bytes per element
uint64_t zkwg_ntt_work_bytes(const zkwg_ntt_t* p, uint64_t n_emails) { return p ? 3ull * p->n * 36ull * n_emails : 0; }

int zkwg_ntt_transform_device(zkwg_ntt_t* p, void* d_data, uint64_t n_polys, int inverse, void* hip_stream) {
  if (!p || !d_data) return ZKWG_RC_BAD_ARG;
  if (p->device < 0) return ZKWG_RC_NO_DEVICE;
  if (n_polys == 0) return ZKWG_RC_OK;
  if (n_polys > 65535) return ZKWG_RC_BAD_ARG;
  if (hipSetDevice(p->device) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  hipStream_t st = (hipStream_t)hip_stream;
  Fr* d = (Fr*)d_data;
  // the passes run through a temporary limb-form buffer (this entry point is not the pipeline's: it allocates and synchronises)
  void* work = nullptr;
  if (hipMalloc(&work, 36ull * p->n * n_polys) != hipSuccess) { (void)hipGetLastError(); return ZKWG_RC_OOM; }
  int rc;
  if (inverse) {
    // natural -> (DIF, inverse roots, x 1 / n) -> bit-reversed -> permuted back to natural order
    rc = zk_ntt_launch(0, d, 3 * p->n, p->n, p->n, 0, work, d, p->d_tw, nullptr, &p->ninv_m, p->L, (u32)n_polys, 1u, st);
    if (rc == 0) rc = zk_ntt_bitrev_launch(d, p->L, (u32)n_polys, st);
  } else {
    rc = zk_ntt_bitrev_launch(d, p->L, (u32)n_polys, st);
    if (rc == 0) rc = zk_ntt_launch(1, d, 3 * p->n, p->n, p->n, 0, work, d, p->d_tw, nullptr, nullptr, p->L, (u32)n_polys, 0u, st);
  }
  if (hipStreamSynchronize(st) != hipSuccess) rc = -1;
  hipFree(work);
  return rc == 0 ? ZKWG_RC_OK : ZKWG_RC_HIP_ERROR;
}

int zkwg_h_evaluations_device(zkwg_ntt_t* p, const void* d_abc, uint64_t abc_stride, uint64_t n_constraints, uint64_t n_emails,
                              void* d_work, void* d_out, uint64_t out_stride, void* hip_stream) {
  if (!p || !d_abc || !d_work || !d_out) return ZKWG_RC_BAD_ARG;
  if (p->device < 0) return ZKWG_RC_NO_DEVICE;
  if (n_emails == 0) return ZKWG_RC_OK;
  if (n_constraints > p->n || abc_stride < 96 * n_constraints || (abc_stride & 31) || out_stride < 32 * p->n || (out_stride & 31) || 3 * n_emails > 65535)
    return ZKWG_RC_BAD_ARG;
  if (hipSetDevice(p->device) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  hipStream_t st = (hipStream_t)hip_stream;
  void* work = d_work;
  const u32 np = (u32)(3 * n_emails);
  // 3 inverse transforms per email straight from A.w | B.w | C.w (zero-padded to the domain), leaving the coset-shifted
  // coefficients inc^i a_i in bit-reversed order; 3 forward transforms from that order; a b - c
  int rc = zk_ntt_launch(0, (const Fr*)d_abc, abc_stride / 32, n_constraints, n_constraints, 0, work, nullptr, p->d_tw, p->d_scale, nullptr, p->L, np, 1u, st);
  if (rc == 0) rc = zk_ntt_launch(1, nullptr, 0, 0, p->n, 1, work, nullptr, p->d_tw, nullptr, nullptr, p->L, np, 0u, st);
  if (rc == 0) rc = zk_ntt_join_launch(work, (Fr*)d_out, p->n, out_stride / 32, (u32)n_emails, st);
  return rc == 0 ? ZKWG_RC_OK : ZKWG_RC_HIP_ERROR;
}

}  // extern "C"
