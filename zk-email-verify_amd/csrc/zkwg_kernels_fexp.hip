// Kernels of per-proof groth16 verification (bodies: zkwg_fexp_core.h, shared with the host path and the host build of the CPU tests).
//   zk_fexp_fold    value i = the product of the k adjacent values k i .. k i + k - 1 (k = 3: the three Miller values of a proof)
//   zk_fexp_step    one product step of the program: out[i] = post(pre_a(x[i]) pre_b(y[i]))
//   zk_fexp_ninv    the inversion step: out[i] = N[i] / (n[i] N[i])_0
//   zk_fexp_pow_u   g -> g^u (62 cyclotomic squarings, 23 products); launched three times
//   zk_g16_vkx      proof i: -(IC_0 + the n_public points x_ij IC_j), affine, into slot 3 i + 1 of the G1 side of the Miller launch
// The first three: a lane pair per value (item = thread / 2, half = thread & 1), 32 values per workgroup, as zk_pair_miller; every lane pair
// runs the same instructions whatever its value is.  A value crosses from launch to launch as 384 bytes of canonical Montgomery words.
// No scratch memory and no LDS: the live state of zk_fexp_pow_u is the base, the accumulator and one product (the footprint of the
// Miller loop), of zk_fexp_step two operands and a product; the chain's seven values are NOT held at once, which is why it is cut into steps.
// tests/test_kernel_resources_fexp.py holds the property for every kernel of this file.
#include <hip/hip_runtime.h>
#include "zkwg_fexp_core.h"

__global__ __launch_bounds__(64) void zk_fexp_fold(const Fq* f, u32 n, u32 k, Fq* out) {
  const u32 i = blockIdx.x * 32u + threadIdx.x / 2u, h = threadIdx.x & 1u;
  if (i >= n) return;                         // (both lanes of a pair leave together)
  zk_fexp_fold_value(f + 12ull * k * i, k, out + 12ull * i, h);
}

__global__ __launch_bounds__(64) void zk_fexp_ninv(const Fq* x, const Fq* y, u32 n, Fq* out) {
  const u32 i = blockIdx.x * 32u + threadIdx.x / 2u, h = threadIdx.x & 1u;
  if (i >= n) return;
  zk_fexp_ninv_value(x + 12ull * i, y + 12ull * i, out + 12ull * i, h);
}

__global__ __launch_bounds__(64) void zk_fexp_pow_u(const Fq* g, u32 n, Fq* out) {
  const u32 i = blockIdx.x * 32u + threadIdx.x / 2u, h = threadIdx.x & 1u;
  if (i >= n) return;
  zk_fexp_pow_u_value(g + 12ull * i, out + 12ull * i, h);
}

__global__ __launch_bounds__(64) void zk_fexp_step(const Fq* x, const Fq* y, u32 n, u32 pre_a, u32 pre_b, u32 post, Fq* out) {
  const u32 i = blockIdx.x * 32u + threadIdx.x / 2u, h = threadIdx.x & 1u;
  if (i >= n) return;
  zk_fexp_step_value(x + 12ull * i, y + 12ull * i, pre_a, pre_b, post, out + 12ull * i, h);
}

__global__ __launch_bounds__(64) void zk_g16_vkx(const G1Affine* ic0, const G1Affine* terms, u32 n_terms, u32 n, G1Affine* g1) {
  const u32 i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  zk_g16_vkx_point(ic0, terms + (u64)n_terms * i, n_terms, g1 + 3ull * i + 1);
}

// n <= ZK_FEXP_MAX values; f: n x k x 384 bytes, out: n x 384 bytes
void zk_fexp_fold_launch(const void* f, u32 n, u32 k, void* out, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(zk_fexp_fold, dim3((n + 31) / 32), dim3(64), 0, st, (const Fq*)f, n, k, (Fq*)out);
}
// out may be x or y
void zk_fexp_ninv_launch(const void* x, const void* y, u32 n, void* out, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(zk_fexp_ninv, dim3((n + 31) / 32), dim3(64), 0, st, (const Fq*)x, (const Fq*)y, n, (Fq*)out);
}
void zk_fexp_pow_u_launch(const void* g, u32 n, void* out, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(zk_fexp_pow_u, dim3((n + 31) / 32), dim3(64), 0, st, (const Fq*)g, n, (Fq*)out);
}
// out may be x or y
void zk_fexp_step_launch(const void* x, const void* y, u32 n, u32 pre_a, u32 pre_b, u32 post, void* out, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(zk_fexp_step, dim3((n + 31) / 32), dim3(64), 0, st, (const Fq*)x, (const Fq*)y, n, pre_a, pre_b, post, (Fq*)out);
}
// terms: n x n_terms points in the zkey's form; g1: 3 n points, of which 3 i + 1 is written
void zk_g16_vkx_launch(const void* ic0, const void* terms, u32 n_terms, u32 n, void* g1, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(zk_g16_vkx, dim3((n + 63) / 64), dim3(64), 0, st, (const G1Affine*)ic0, (const G1Affine*)terms, n_terms, n, (G1Affine*)g1);
}
