// Kernels of `powersoftau verify` (bodies: zkwg_verify_core.h, shared with the host build of the CPU tests).
//   zk_verify_g2_subgroup   is table-form G2 point i in the subgroup of order r?  A lane pair per point (zkwg_ec29.h: item = thread / 2,
//                           half = thread & 1); every pair walks the SAME 63 digits of u, then three additions, a doubling, nine constant
//                           products and a cross-multiplied comparison.  Counts the points outside and keeps the lowest such index.
//   zk_verify_widen         16-byte scalars -> the 32-byte scalars the multi-exponentiation plans read
// The curve check in front of the first is the set-up's kernel (zk_setup_prepare_launch).  No scratch memory, no LDS; 2 wavefronts per
// SIMD for the subgroup test, the floor of the other G2 walks (tests/test_kernel_resources_verify.py).
#include <hip/hip_runtime.h>
#include "zkwg_verify_core.h"

// res[0]: points outside the subgroup, res[1]: the lowest index of one (the caller sets it to 0xffffffff)
__global__ __launch_bounds__(64) void zk_verify_g2_subgroup(const G2Affine* pts, u32 n, ZkPhase2Digits Du, u32* res) {
  const u32 i = blockIdx.x * 32u + threadIdx.x / 2u, h = threadIdx.x & 1u;
  if (i >= n) return;                         // (both lanes of a pair leave together)
  const bool inside = zk_verify_g2_in_subgroup(pts + i, h, Du);
  if (!inside && h == 0) {
    atomicAdd(res, 1u);
    atomicMin(res + 1, i);
  }
}

__global__ __launch_bounds__(256) void zk_verify_widen(const uint4* in, uint4* out, u64 n) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  out[2 * i] = in[i];
  out[2 * i + 1] = make_uint4(0, 0, 0, 0);
}

// n <= ZK_VERIFY_PIECE table-form points
void zk_verify_g2_subgroup_launch(const void* pts, u32 n, const ZkPhase2Digits& Du, u32* res, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(zk_verify_g2_subgroup, dim3((n + 31) / 32), dim3(64), 0, st, (const G2Affine*)pts, n, Du, res);
}
void zk_verify_widen_launch(const void* in, void* out, u64 n, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(zk_verify_widen, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, (const uint4*)in, (uint4*)out, n);
}
