// zk_zkey_abc -- the first stage of `groth16.prove(zkey, wtns)` from witness VALUES (snarkjs' buildABC1; reference call site
// packages/helpers/src/chunked-zkey.ts:80-84): per witness A.w | B.w | C.w with C.w = A.w o B.w, Montgomery form, in the layout
// zkwg_h_evaluations_device reads.  The rows come from section 4 of the key (zkwg_zkey_core.h: table, forms and bounds); the witnesses
// are 32-byte standard-form values, E of them per launch.
//
//   zk_zkey_abc_short  one lane per constraint of at most ZK_ZKEY_LONG terms, the constraints sorted by length so that the lanes of a
//                      wavefront run the same number of steps (98 % of EmailVerifier's constraints have fewer than 8 terms)
//   zk_zkey_abc_long   one wavefront per longer constraint: lane l takes the terms l, l + 64, ..., the 64 shares are added across the
//                      wavefront (no LDS, no scratch)
// Both take G witnesses per lane (grid.y = groups of witnesses; G = 2, or 4 with ZKWG_ZKEY_G=4: DESIGN.md section 23): a row's +-1 terms are
// read once for the group and the G gathers of a term are independent loads in flight together.
//   zk_zkey_range      a witness value >= r anywhere among the nVars values flags its witness (status ZKWG_ERR_WITNESS_NOT_REDUCED);
//   zk_zkey_scrub      ... and a flagged witness is zeroed in the context's copy, so that no non-canonical scalar reaches the sums.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include "zkwg_zkey_core.h"


struct ZkZkeyArgs {
  ZkZkeyDev T;
  const u8* wit;
  u64 stride;
  u8* abc;
  u64 abc_stride;
  u32 count;
};

template <int G>
__device__ __forceinline__ void zk_zkey_witnesses(const ZkZkeyArgs& A, u32 e0, const u8* (&w)[G]) {
#pragma unroll
  for (int g = 0; g < G; ++g) w[g] = A.wit + (u64)min(e0 + g, A.count - 1) * A.stride;      // (a short last group repeats its last witness)
}
__device__ __forceinline__ void zk_zkey_store(const ZkZkeyArgs& A, u32 e, u32 j, const Fr& a, const Fr& b) {
  Fr* out = (Fr*)(A.abc + (u64)e * A.abc_stride);
  out[j] = a; out[A.T.n_rows + j] = b; out[2 * A.T.n_rows + j] = fr_mont_mul(a, b);
}

template <int G>
__global__ __launch_bounds__(256) void zk_zkey_abc_short(ZkZkeyArgs A) {
  const u64 o = A.T.n_long + (u64)blockIdx.x * 256 + threadIdx.x;
  if (o >= A.T.n_rows) return;
  const u32 j = A.T.order[o], e0 = blockIdx.y * G;
  const u8* w[G];
  zk_zkey_witnesses<G>(A, e0, w);
  Fr a[G], b[G];
  zk_zkey_row<G>(A.T, A.T.rows[2ull * j], 0, 1, w, a);
  zk_zkey_row<G>(A.T, A.T.rows[2ull * j + 1], 0, 1, w, b);
#pragma unroll
  for (int g = 0; g < G; ++g) if (e0 + g < A.count) zk_zkey_store(A, e0 + g, j, a[g], b[g]);
}

__device__ __forceinline__ Fr zk_zkey_wave_sum(Fr v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    Fr o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o.l[i] = __shfl_xor((unsigned long long)v.l[i], off, 64);
    v = fr_add(v, o);
  }
  return v;
}
template <int G>
__global__ __launch_bounds__(256) void zk_zkey_abc_long(ZkZkeyArgs A) {
  const u32 o = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (o >= A.T.n_long) return;                        // (a whole wavefront leaves)
  const u32 j = A.T.order[o], e0 = blockIdx.y * G;
  const u8* w[G];
  zk_zkey_witnesses<G>(A, e0, w);
  Fr a[G], b[G];
  zk_zkey_row<G>(A.T, A.T.rows[2ull * j], lane, 64, w, a);
  zk_zkey_row<G>(A.T, A.T.rows[2ull * j + 1], lane, 64, w, b);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const Fr sa = zk_zkey_wave_sum(a[g]), sb = zk_zkey_wave_sum(b[g]);
    if (lane == 0 && e0 + g < A.count) zk_zkey_store(A, e0 + g, j, sa, sb);
  }
}

__global__ __launch_bounds__(256) void zk_zkey_range(const u8* __restrict__ wit, u64 stride, u64 n_vars, int* __restrict__ flags) {
  const u8* w = wit + (u64)blockIdx.y * stride;
  bool bad = false;
  for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n_vars; i += (u64)gridDim.x * 256) {
    u32 x[8];
    zk_zkey_load(w + 32 * i, x);
    // r's top word is 0x30644e72: almost every value is decided by it
    if (x[7] >= 0x30644e72u && fr_geq(zk_zkey_words_fr(x), fr_p())) bad = true;
  }
  if (bad) flags[blockIdx.y] = 1;
}
__global__ __launch_bounds__(256) void zk_zkey_scrub(u8* __restrict__ wit, u64 stride, u64 n_vars, const int* __restrict__ flags) {
  if (!flags[blockIdx.y]) return;
  uint4* w = (uint4*)(wit + (u64)blockIdx.y * stride);
  for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < 2 * n_vars; i += (u64)gridDim.x * 256) w[i] = uint4{0, 0, 0, 0};
}

// count witnesses `stride` bytes apart (16-byte aligned) -> count records A.w | B.w | C.w `abc_stride` bytes apart
int zk_zkey_abc_launch(const ZkZkeyDev& T, const void* d_wit, u64 stride, u32 count, void* d_abc, u64 abc_stride, hipStream_t st) {
  if (!count || !T.n_rows) return 0;
  ZkZkeyArgs A{T, (const u8*)d_wit, stride, (u8*)d_abc, abc_stride, count};
  static const u32 G = getenv("ZKWG_ZKEY_G") && atoi(getenv("ZKWG_ZKEY_G")) == 4 ? 4u : 2u;      // (tuning knob; 2 measured 11 % faster than 4: DESIGN.md section 23)
  const u32 groups = (count + G - 1) / G;
  const u64 n_short = T.n_rows - T.n_long;
  // (the long constraints first: they are the longest-running wavefronts)
  const dim3 gl((T.n_long + 3) / 4, groups), gs((u32)((n_short + 255) / 256), groups);
  if (T.n_long) { if (G == 2) hipLaunchKernelGGL(zk_zkey_abc_long<2>, gl, dim3(256), 0, st, A); else hipLaunchKernelGGL(zk_zkey_abc_long<4>, gl, dim3(256), 0, st, A); }
  if (n_short) { if (G == 2) hipLaunchKernelGGL(zk_zkey_abc_short<2>, gs, dim3(256), 0, st, A); else hipLaunchKernelGGL(zk_zkey_abc_short<4>, gs, dim3(256), 0, st, A); }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
// flags[e] = 1 for every witness with a value >= r, and such a witness zeroed in place (d_wit is the caller's own copy)
int zk_zkey_range_launch(void* d_wit, u64 stride, u64 n_vars, u32 count, int* d_flags, hipStream_t st) {
  if (!count) return 0;
  if (hipMemsetAsync(d_flags, 0, 4ull * count, st) != hipSuccess) return -1;
  const u64 g = (n_vars + 255) / 256;
  const dim3 grid((u32)(g > 1024 ? 1024 : g), count);
  hipLaunchKernelGGL(zk_zkey_range, grid, dim3(256), 0, st, (const u8*)d_wit, stride, n_vars, d_flags);
  hipLaunchKernelGGL(zk_zkey_scrub, grid, dim3(256), 0, st, (u8*)d_wit, stride, n_vars, (const int*)d_flags);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
