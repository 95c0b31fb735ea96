// Kernels of the groth16 set-up (bodies: zkwg_setup_core.h, shared with the host mirror of the CPU tests): the segmented linear
// combinations of points  out[wire] = sum_t coef_t table[row_t]  behind sections 3 and 5 - 8 of a new .zkey, their conversion to
// canonical affine points, the curve check of the uploaded powers of tau and the strided copy behind section 9.
// G2 runs on lane pairs (zkwg_ec29.h): item = thread / 2, half = thread & 1.  No kernel here may use scratch memory
// (tests/test_kernel_resources_setup.py).
#include <hip/hip_runtime.h>
#include "zkwg_setup_core.h"

template <class C> struct ZkSetupArgs {
  typedef Xyzz29<typename C::F> X;
  ZkSetupDev T;
  ZkSetupTab<C> tab;
  const ZkSetupJob* jobs;
  u32 n_jobs;
  X* out;             // the accumulators (short, join) or the partial sums (chunk) the jobs write
  const X* part;      // join: the partial sums
};

// the sum of a wavefront's accumulators, in item 0 (red: one entry per lane)
template <class C>
__device__ __forceinline__ Xyzz29<typename C::F> zk_setup_wave_reduce(Xyzz29<typename C::F> acc, Xyzz29<typename C::F>* red, u32 item, u32 h) {
  constexpr u32 per = 64u / C::LANES;
  for (u32 s = per / 2; s >= 1; s >>= 1) {
    red[threadIdx.x] = acc;
    __syncthreads();
    if (item < s) acc = ec29_add<typename C::F>(acc, red[(item + s) * C::LANES + h]);
    __syncthreads();
  }
  return acc;
}
// one lane (pair) per wire of at most ZK_SETUP_LONG terms; the jobs are sorted by cost
template <class C> __global__ __launch_bounds__(64) void zk_setup_short(ZkSetupArgs<C> A) {
  constexpr u32 per = 64u / C::LANES;
  const u32 j = blockIdx.x * per + threadIdx.x / C::LANES, h = threadIdx.x % C::LANES;
  if (j >= A.n_jobs) return;
  const ZkSetupJob job = A.jobs[j];
  A.out[(u64)job.out * C::LANES + h] = zk_setup_sum<C>(A.T, A.tab, job.t0, job.n, 0u, 1u, h);
}
// one wavefront per chunk of a long wire
template <class C> __global__ __launch_bounds__(64) void zk_setup_chunk(ZkSetupArgs<C> A) {
  __shared__ Xyzz29<typename C::F> red[64];
  constexpr u32 per = 64u / C::LANES;
  const u32 item = threadIdx.x / C::LANES, h = threadIdx.x % C::LANES;
  const ZkSetupJob job = A.jobs[blockIdx.x];
  const Xyzz29<typename C::F> acc = zk_setup_wave_reduce<C>(zk_setup_sum<C>(A.T, A.tab, job.t0, job.n, item, per, h), red, item, h);
  if (item == 0) A.out[(u64)job.out * C::LANES + h] = acc;
}
// one wavefront per long wire: the sum of its chunks
template <class C> __global__ __launch_bounds__(64) void zk_setup_join_wave(ZkSetupArgs<C> A) {
  __shared__ Xyzz29<typename C::F> red[64];
  constexpr u32 per = 64u / C::LANES;
  const u32 item = threadIdx.x / C::LANES, h = threadIdx.x % C::LANES;
  const ZkSetupJob job = A.jobs[blockIdx.x];
  const Xyzz29<typename C::F> acc = zk_setup_wave_reduce<C>(zk_setup_join<C>(A.part, job.t0, job.n, item, per, h), red, item, h);
  if (item == 0) A.out[(u64)job.out * C::LANES + h] = acc;
}
template <class C> __global__ __launch_bounds__(64) void zk_setup_den_k(const Xyzz29<typename C::F>* acc, Fq29* den, u32 n) {
  constexpr u32 per = 64u / C::LANES;
  const u32 i = blockIdx.x * per + threadIdx.x / C::LANES, h = threadIdx.x % C::LANES;
  if (i >= n) return;
  const Fq29 d = zk_setup_den_of<C>(acc[(u64)i * C::LANES + h]);
  if (h == 0) den[i] = d;
}
__global__ __launch_bounds__(64) void zk_setup_inv_k(Fq29* den, Fq29* pref, u32 n, u32 n_lanes) {
  const u32 lane = blockIdx.x * 64u + threadIdx.x;
  if (lane < n_lanes) zk_setup_batch_inv(den, pref, n, lane, n_lanes);
}
template <class C> __global__ __launch_bounds__(64) void zk_setup_affine_k(const Xyzz29<typename C::F>* acc, const Fq29* den, const u32* seg_wire, typename C::Affine* out, u32 n) {
  constexpr u32 per = 64u / C::LANES;
  const u32 i = blockIdx.x * per + threadIdx.x / C::LANES, h = threadIdx.x % C::LANES;
  if (i >= n) return;
  zk_setup_affine<C>(acc[(u64)i * C::LANES + h], den[i], out + (seg_wire ? seg_wire[i] : i), h);      // (no map: point i -> out[i])
}
// the curve check (and the tables' form) of n uploaded points; *bad is raised when a point fails
template <class C> __global__ __launch_bounds__(64) void zk_setup_prepare(const typename C::Affine* in, typename C::Affine* out, u64 n, u32* bad) {
  constexpr u32 per = 64u / C::LANES;
  const u64 i = (u64)blockIdx.x * per + threadIdx.x / C::LANES;
  if (i >= n) return;
  if (!zk_setup_prepare_half<C>(in, out, i, threadIdx.x % C::LANES)) atomicOr(bad, 1u);
}
// section 9: out[j] = in[2 j + 1], 64-byte points, four lanes per point
__global__ __launch_bounds__(256) void zk_setup_odd_copy(const uint4* in, uint4* out, u64 n) {
  const u64 t = (u64)blockIdx.x * 256u + threadIdx.x;
  if (t < 4 * n) out[t] = in[4 * (2 * (t >> 2) + 1) + (t & 3u)];
}

// n accumulators -> canonical affine points in the zkey's form: out[seg_wire[i]] (out[i] without a map); den, pref: n values of room each
template <class C>
static void zk_setup_to_affine_t(const void* acc, Fq29* den, Fq29* pref, const u32* seg_wire, void* out, u32 n, hipStream_t st) {
  typedef Xyzz29<typename C::F> X;
  constexpr u32 per = 64u / C::DEV_LANES;
  if (!n) return;
  const u32 n_lanes = (n + ZK_SETUP_INV_BATCH - 1) / ZK_SETUP_INV_BATCH;
  hipLaunchKernelGGL(zk_setup_den_k<C>, dim3((n + per - 1) / per), dim3(64), 0, st, (const X*)acc, den, n);
  hipLaunchKernelGGL(zk_setup_inv_k, dim3((n_lanes + 63) / 64), dim3(64), 0, st, den, pref, n, n_lanes);
  hipLaunchKernelGGL(zk_setup_affine_k<C>, dim3((n + per - 1) / per), dim3(64), 0, st, (const X*)acc, (const Fq29*)den, seg_wire, (typename C::Affine*)out, n);
}
template <class C>
static void zk_setup_run_t(const ZkSetupRun& r, hipStream_t st) {
  typedef Xyzz29<typename C::F> X;
  constexpr u32 per = 64u / C::DEV_LANES;
  const ZkSetupTab<C> tab{(const typename C::Affine*)r.t0, (const typename C::Affine*)r.t1, (const typename C::Affine*)r.t2};
  if (r.n_short) hipLaunchKernelGGL(zk_setup_short<C>, dim3((r.n_short + per - 1) / per), dim3(64), 0, st, ZkSetupArgs<C>{r.T, tab, r.shorts, r.n_short, (X*)r.acc, nullptr});
  if (r.n_chunk) hipLaunchKernelGGL(zk_setup_chunk<C>, dim3(r.n_chunk), dim3(64), 0, st, ZkSetupArgs<C>{r.T, tab, r.chunks, r.n_chunk, (X*)r.part, nullptr});
  if (r.n_join) hipLaunchKernelGGL(zk_setup_join_wave<C>, dim3(r.n_join), dim3(64), 0, st, ZkSetupArgs<C>{r.T, tab, r.joins, r.n_join, (X*)r.acc, (const X*)r.part});
  zk_setup_to_affine_t<C>(r.acc, r.den, r.pref, r.seg_wire, r.out, r.n_seg, st);
}
void zk_setup_run_launch(int group, const ZkSetupRun& r, hipStream_t st) {
  if (group == 1) zk_setup_run_t<ZkEcG1>(r, st);
  else zk_setup_run_t<ZkEcG2>(r, st);
}
void zk_setup_to_affine_launch(int group, const void* acc, Fq29* den, Fq29* pref, const u32* seg_wire, void* out, u32 n, hipStream_t st) {
  if (group == 1) zk_setup_to_affine_t<ZkEcG1>(acc, den, pref, seg_wire, out, n, st);
  else zk_setup_to_affine_t<ZkEcG2>(acc, den, pref, seg_wire, out, n, st);
}
void zk_setup_prepare_launch(int group, const void* in, void* out, u64 n, u32* bad, hipStream_t st) {
  if (group == 1) hipLaunchKernelGGL(zk_setup_prepare<ZkEcG1>, dim3((u32)((n + 63) / 64)), dim3(64), 0, st, (const G1Affine*)in, (G1Affine*)out, n, bad);
  else hipLaunchKernelGGL(zk_setup_prepare<ZkEcG2>, dim3((u32)((n + 31) / 32)), dim3(64), 0, st, (const G2Affine*)in, (G2Affine*)out, n, bad);
}
void zk_setup_odd_copy_launch(const void* in, void* out, u64 n, hipStream_t st) {
  hipLaunchKernelGGL(zk_setup_odd_copy, dim3((u32)((4 * n + 255) / 256)), dim3(256), 0, st, (const uint4*)in, (uint4*)out, n);
}
