// Kernel of a phase-2 contribution (body: zkwg_phase2_core.h, shared with the host mirror of the CPU tests): acc[i] = s P[i] for n
// table-form points and ONE scalar, whose non-adjacent form arrives as a kernel argument -- every lane of every wavefront takes the same
// path through the digit string.  One lane per G1 point, a lane pair per G2 point (zkwg_ec29.h): item = thread / 2, half = thread & 1.
// The curve check in front of it and the conversion to canonical affine points behind it are the set-up's kernels
// (zk_setup_prepare_launch / zk_setup_to_affine_launch, zkwg_kernels_setup.hip).  No scratch memory (tests/test_kernel_resources_phase2.py).
#include <hip/hip_runtime.h>
#include "zkwg_phase2_core.h"

template <class C> __global__ __launch_bounds__(64) void zk_phase2_scale(const typename C::Affine* pts, Xyzz29<typename C::F>* acc, u32 n, ZkPhase2Digits D) {
  constexpr u32 per = 64u / C::LANES;
  const u32 i = blockIdx.x * per + threadIdx.x / C::LANES, h = threadIdx.x % C::LANES;
  if (i >= n) return;                         // (both lanes of a pair leave together)
  acc[(u64)i * C::LANES + h] = zk_phase2_scale_point<C>(pts + i, h, D);
}

// n <= ZK_PHASE2_PIECE table-form points at pts -> accumulators at acc (144 / 288 bytes each)
void zk_phase2_scale_launch(int group, const void* pts, void* acc, u32 n, const ZkPhase2Digits& D, hipStream_t st) {
  if (!n) return;
  if (group == 1) hipLaunchKernelGGL(zk_phase2_scale<ZkEcG1>, dim3((n + 63) / 64), dim3(64), 0, st, (const G1Affine*)pts, (Xyzz29<ZkF1>*)acc, n, D);
  else hipLaunchKernelGGL(zk_phase2_scale<ZkEcG2>, dim3((n + 31) / 32), dim3(64), 0, st, (const G2Affine*)pts, (Xyzz29<ZkF2>*)acc, n, D);
}
