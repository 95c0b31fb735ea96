// Kernels of "each point times its own scalar" (bodies: zkwg_ptau_key_core.h, shared with the host mirror of the CPU tests).  One lane
// per G1 point, a lane pair per G2 point (zkwg_ec29.h): item = thread / 2, half = thread & 1.
//   zk_ptau_key_table   rows 1 - 7 of every point's table (3 P .. 15 P) as accumulators, row-major: acc[row - 1][point]
//   zk_ptau_key_walk    the regular walk over the affine table T[row][point]: 63 windows of 4 doublings and one mixed addition of the row
//                       the lane's digit selects, then the even scalar's fix-up.  SCALARS = true: the lane reads its scalar (32 bytes,
//                       standard form); false: it computes c t^(first + i) from the table of t^(2^i) (zk_key_power_scalar).
// The curve check in front and the conversions to affine points (of the table's rows and of the results) are the set-up's kernels
// (zk_setup_prepare_launch / zk_setup_to_affine_launch).  No scratch memory, no LDS; 3 wavefronts per SIMD for G1 and 2 for G2
// (tests/test_kernel_resources_ptau_key.py).
#include <hip/hip_runtime.h>
#include "zkwg_ptau_key_core.h"

template <class C> __global__ __launch_bounds__(64) void zk_ptau_key_table(const typename C::Affine* tab, Xyzz29<typename C::F>* acc, u32 n) {
  constexpr u32 per = 64u / C::LANES;
  const u32 i = blockIdx.x * per + threadIdx.x / C::LANES, h = threadIdx.x % C::LANES;
  if (i >= n) return;                         // (both lanes of a pair leave together)
  zk_key_table_point<C>(tab + i, h, acc + (u64)i * C::LANES + h, (u64)n * C::LANES);
}

template <class C, bool SCALARS> __global__ __launch_bounds__(64) void zk_ptau_key_walk(const typename C::Affine* tab, Xyzz29<typename C::F>* acc, u32 n, const uint4* scalars,
                                                                                         const ZkKeyPowers* powers, u64 first, u32 n_bits) {
  constexpr u32 per = 64u / C::LANES;
  const u32 i = blockIdx.x * per + threadIdx.x / C::LANES, h = threadIdx.x % C::LANES;
  if (i >= n) return;
  Fr k;
  if (SCALARS) {
    const uint4 a = scalars[2 * (u64)i], b = scalars[2 * (u64)i + 1];
    k = zk_key_reduce(Fr{{(u64)a.x | ((u64)a.y << 32), (u64)a.z | ((u64)a.w << 32), (u64)b.x | ((u64)b.y << 32), (u64)b.z | ((u64)b.w << 32)}});
  } else {
    k = zk_key_power_scalar(powers, first + i, n_bits);
  }
  acc[(u64)i * C::LANES + h] = zk_key_mul<C>(tab + i, n, h, zk_key_recode(k));
}

// table-form points at tab[0 .. n) -> accumulators of rows 1 - 7 at acc[0 .. 7 n)
void zk_ptau_key_table_launch(int group, const void* tab, void* acc, u32 n, hipStream_t st) {
  if (!n) return;
  if (group == 1) hipLaunchKernelGGL(zk_ptau_key_table<ZkEcG1>, dim3((n + 63) / 64), dim3(64), 0, st, (const G1Affine*)tab, (Xyzz29<ZkF1>*)acc, n);
  else hipLaunchKernelGGL(zk_ptau_key_table<ZkEcG2>, dim3((n + 31) / 32), dim3(64), 0, st, (const G2Affine*)tab, (Xyzz29<ZkF2>*)acc, n);
}
// the table T[row][point] (8 n table-form points) -> accumulators at acc[0 .. n); scalars: n x 32 bytes, or null: c t^(first + i) from `powers`
void zk_ptau_key_walk_launch(int group, const void* tab, void* acc, u32 n, const void* scalars, const ZkKeyPowers* powers, u64 first, hipStream_t st) {
  if (!n) return;
  const u32 n_bits = zk_key_bits(first + n - 1);
  const dim3 grid(group == 1 ? (n + 63) / 64 : (n + 31) / 32), block(64);
  if (group == 1 && scalars) hipLaunchKernelGGL((zk_ptau_key_walk<ZkEcG1, true>), grid, block, 0, st, (const G1Affine*)tab, (Xyzz29<ZkF1>*)acc, n, (const uint4*)scalars, powers, first, n_bits);
  else if (group == 1) hipLaunchKernelGGL((zk_ptau_key_walk<ZkEcG1, false>), grid, block, 0, st, (const G1Affine*)tab, (Xyzz29<ZkF1>*)acc, n, (const uint4*)scalars, powers, first, n_bits);
  else if (scalars) hipLaunchKernelGGL((zk_ptau_key_walk<ZkEcG2, true>), grid, block, 0, st, (const G2Affine*)tab, (Xyzz29<ZkF2>*)acc, n, (const uint4*)scalars, powers, first, n_bits);
  else hipLaunchKernelGGL((zk_ptau_key_walk<ZkEcG2, false>), grid, block, 0, st, (const G2Affine*)tab, (Xyzz29<ZkF2>*)acc, n, (const uint4*)scalars, powers, first, n_bits);
}
