// Kernels of the transform over points (bodies: zkwg_ptau_core.h, shared with the host mirror of the CPU tests).  One butterfly per
// G1 lane, per G2 lane pair (zkwg_ec29.h): item = thread / 2, half = thread & 1.  zk_ptau_stage<C, true> serves the stages whose
// wavefronts hold one twiddle (its digit words go through readfirstlane: scalar branches, the lockstep walk of zk_phase2_scale),
// zk_ptau_stage<C, false> the stages where lanes differ (the addition predicated on the lane's digit).  The curve check in front, the
// 2^-L scaling and the conversion behind every stage are the kernels of the set-up and of phase 2 (zk_setup_prepare_launch,
// zk_phase2_scale_launch, zk_setup_to_affine_launch).  No scratch memory (tests/test_kernel_resources_ptau.py).
#include <hip/hip_runtime.h>
#include "zkwg_ptau_core.h"

// stage s of a 2^L-point transform: table-form points at pts -> accumulators at acc (same indices); tw: the table of a 2^(s + 1 + tw_shift)-point transform
template <class C, bool UNIFORM> __global__ __launch_bounds__(64) void zk_ptau_stage(const typename C::Affine* pts, Xyzz29<typename C::F>* acc, const ZkPtauTw* tw, u32 L, u32 s, u32 tw_shift) {
  constexpr u32 per = 64u / C::LANES;
  const u32 t = blockIdx.x * per + threadIdx.x / C::LANES, h = threadIdx.x % C::LANES;
  if (t >= (1u << (L - 1u))) return;          // (both lanes of a pair leave together)
  const ZkPtauAt at = zk_ptau_at(t, L, s);
  Xyzz29<typename C::F> sum, dif;
  zk_ptau_butterfly<C, UNIFORM>(pts + at.i0, pts + at.i1, h, at.j ? tw + ((u64)at.j << tw_shift) : nullptr, sum, dif);
  acc[at.i0 * C::LANES + h] = sum;
  acc[at.i1 * C::LANES + h] = dif;
}
// the permutation to bit-reversed order, in place: one lane per 16 bytes of the pair (i, reversed i), i below its reverse
__global__ __launch_bounds__(256) void zk_ptau_permute(uint4* pts, u32 L, u32 lg_chunks) {
  const u64 k = (u64)blockIdx.x * 256u + threadIdx.x;
  const u32 i = (u32)(k >> lg_chunks), c = (u32)k & ((1u << lg_chunks) - 1u);
  if (i >= (1u << L)) return;
  const u32 r = zk_ptau_bitrev(i, L);
  if (i >= r) return;
  uint4* a = pts + ((u64)i << lg_chunks) + c;
  uint4* b = pts + ((u64)r << lg_chunks) + c;
  const uint4 va = *a, vb = *b;
  *a = vb; *b = va;
}

template <class C>
static void zk_ptau_stage_t(const void* pts, void* acc, const ZkPtauTw* tw, u32 L, u32 s, u32 tw_shift, hipStream_t st) {
  constexpr u32 per = 64u / C::DEV_LANES;
  const u32 n_bf = 1u << (L - 1u), groups = 1u << (L - 1u - s);
  typedef Xyzz29<typename C::F> X;
  if (groups >= per) hipLaunchKernelGGL((zk_ptau_stage<C, true>), dim3((n_bf + per - 1) / per), dim3(64), 0, st, (const typename C::Affine*)pts, (X*)acc, tw, L, s, tw_shift);
  else hipLaunchKernelGGL((zk_ptau_stage<C, false>), dim3((n_bf + per - 1) / per), dim3(64), 0, st, (const typename C::Affine*)pts, (X*)acc, tw, L, s, tw_shift);
}
// stage s < L of a 2^L-point transform (L >= 1) under the table of a 2^table_L-point transform, table_L >= L
void zk_ptau_stage_launch(int group, const void* pts, void* acc, const ZkPtauTw* tw, u32 L, u32 s, u32 table_L, hipStream_t st) {
  const u32 tw_shift = table_L - 1u - s;
  if (group == 1) zk_ptau_stage_t<ZkEcG1>(pts, acc, tw, L, s, tw_shift, st);
  else zk_ptau_stage_t<ZkEcG2>(pts, acc, tw, L, s, tw_shift, st);
}
void zk_ptau_permute_launch(int group, void* pts, u32 L, hipStream_t st) {
  const u32 lg = group == 2 ? 3u : 2u;        // 16-byte pieces of a point: 8 / 4
  const u64 n = (1ull << L) << lg;
  hipLaunchKernelGGL(zk_ptau_permute, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, (uint4*)pts, L, lg);
}
