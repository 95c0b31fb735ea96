// Kernels of batched groth16 verification (bodies: zkwg_pair_core.h, shared with the host build of the CPU tests).
//   zk_pair_miller    pair i of table-form points -> its Miller value (384 bytes, the host's Fq12) and whether the G2 point is in the
//                     subgroup of order r.  A lane pair per pair (item = thread / 2, half = thread & 1), 32 pairs per workgroup; every lane
//                     pair runs the same 64 doubling and 36 + 2 addition steps, whatever its points are.
//   zk_pair_product   one level of the product tree: lane pair j multiplies the ZK_PAIR_FOLD values 4 j .. 4 j + 3 that are in range and in
//                     use (the others count as 1) and stores the product.  Fq12 products are exact and the store is canonical, so the root
//                     does not depend on how the levels are cut.
// No scratch memory and no LDS: an Fq12 is 54 registers per lane, and f^2 keeps its operand and its result (108) beside the running point
// (36), the base point (18 + 18) and the temporaries of one Fq2 product -- inside the 256 registers of 2 wavefronts per SIMD, so the Fq12
// temporaries were NOT moved to LDS.  The products are written per output coefficient for that reason (no array of 11 partial sums).
// tests/test_kernel_resources_pair.py holds both properties.
#include <hip/hip_runtime.h>
#include "zkwg_pair_core.h"

__global__ __launch_bounds__(64) void zk_pair_miller(const G1Affine* p, const G2Affine* q, u32 n, ZkPhase2Digits Du, Fq* f, u8* inside) {
  const u32 i = blockIdx.x * 32u + threadIdx.x / 2u, h = threadIdx.x & 1u;
  if (i >= n) return;                         // (both lanes of a pair leave together)
  const bool in = zk_pair_miller_point(p + i, q + i, h, Du, f + 12ull * i);
  if (h == 0) inside[i] = in ? 1 : 0;
}

__global__ __launch_bounds__(64) void zk_pair_product(const Fq* f, const u8* use, u32 n, Fq* out) {
  const u32 j = blockIdx.x * 32u + threadIdx.x / 2u, h = threadIdx.x & 1u;
  if (j >= (n + ZK_PAIR_FOLD - 1) / ZK_PAIR_FOLD) return;
  ZkF12 acc = zk_f12_one();
#pragma unroll 1
  for (u32 k = 0; k < ZK_PAIR_FOLD; ++k) {
    const u32 i = j * ZK_PAIR_FOLD + k;
    const bool on = i < n && (!use || use[i] != 0);             // (the same for both lanes of the pair)
    const ZkF12 x = zk_f12_load(f + 12ull * (on ? i : 0u), h);  // (index 0 exists: n >= 1 here)
    acc = zk_f12_mul(acc, zk_f12_select(on, x, zk_f12_one()));
    ZKF12_CLAIM(acc, 5, 2, ZK_F12_MUL_V5);                        // (the host build of this loop checks it: tests/native/pairtest.cpp pt_pair_product)
  }
  zk_f12_store(out + 12ull * j, acc, h);
}

// n <= ZK_PAIR_MAX table-form pairs; f: n x 384 bytes
void zk_pair_miller_launch(const void* g1, const void* g2, u32 n, const ZkPhase2Digits& Du, void* f, u8* inside, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(zk_pair_miller, dim3((n + 31) / 32), dim3(64), 0, st, (const G1Affine*)g1, (const G2Affine*)g2, n, Du, (Fq*)f, inside);
}
// out: ceil(n / ZK_PAIR_FOLD) x 384 bytes, not f; use may be null (every value counts)
void zk_pair_product_launch(const void* f, const u8* use, u32 n, void* out, hipStream_t st) {
  if (!n) return;
  const u32 m = (n + ZK_PAIR_FOLD - 1) / ZK_PAIR_FOLD;
  hipLaunchKernelGGL(zk_pair_product, dim3((m + 31) / 32), dim3(64), 0, st, (const Fq*)f, use, n, (Fq*)out);
}
