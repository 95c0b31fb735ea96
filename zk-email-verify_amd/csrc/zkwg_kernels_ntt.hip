// Batched BN254-Fr number-theoretic transforms for the step that follows A.w | B.w | C.w in `snarkjs.groth16.prove`
// (reference call site: packages/helpers/src/chunked-zkey.ts:80-84; SURVEY.md 8f4 "hand-off into the prover"): per proof
// three inverse transforms, the coset shift, three forward transforms and a(x) b(x) - c(x) on a domain of 2^20 .. 2^22
// points -- 6 x 2^L x L / 2 butterflies of one Montgomery product each.  ARITHMETIC-bound: ~150 M products per
// EmailVerifier(1024,1536) proof against ~2 GB of HBM traffic; the bound is the issue rate of v_mad_u64_u32.  No MFMA:
// the products are 254-bit modular integers.
//
// Structure:
//   * decimation in frequency (natural order in, bit-reversed out) for the inverse transforms, decimation in time
//     (bit-reversed in, natural out) for the forward ones: no permutation pass between them, and the coset scaling
//     inc^i / n is a table indexed by bit-reversed position, fused into the last inverse pass;
//   * each transform is ceil(L / 7) passes over HBM ("four-step" recursion): COLUMN passes run 2^g-point sub-transforms (g <= 7)
//     on 1024 / 2^g neighbouring columns of a block at a time in LDS, followed (DIF) or preceded (DIT) by the block twiddle
//     w_N^(column * frequency); the last / first pass transforms contiguous 2^g-element rows, 1,024 elements per workgroup;
//   * round 6: VALUES STAY IN 9 x 29-BIT LIMB FORM across the butterfly stages of a pass (zkwg_fr29.h): a product is the 250-instruction
//     product-scanning form without split / pack / conditional subtraction (315 behind the 4 x 64-bit interface), an addition is 9
//     adds, a subtraction adds a multiple of r that dominates the subtrahend (round 5: carry chain + compare + select each).  Data
//     keep the callers' 2^256 form, the twiddle / scale tables are in 2^261 form (one operand in that form is what the 2^-261 of the
//     product needs).  Bounds: a DIF stage pair grows a value 4 x at most (radix-4 group: y0 = x0 + x1 + x2 + x3), so with pass
//     inputs < 5 r the three pairs + one single stage of a 7-stage pass stay below 640 r (the top limb holds what exceeds 2^232:
//     < 2^32 up to 1,352 r), and the pass's closing product with a canonical twiddle returns < (640 / 169 + 1) r < 5 r; a DIT stage adds
//     at most 3 r.  Limbs 0 .. 7 are carry-normalised where a sum feeds a sum (two of a group's four values per stage pair).
//   * the work buffer between passes holds limb form too, planar (16 + 16 + 4 bytes per element in three arrays per polynomial):
//     nothing is reduced or packed until a b - c leaves as canonical words;
//   * one workgroup = 1,024 elements = 36 KiB of LDS + its twiddles: 3 workgroups per CU.
//   * the per-phase bodies, the butterflies, the pass schedule and the plan's tables live in zkwg_ntt_core.h, shared with the host mirror
//     of the CPU tests; the kernels below are those phases with a barrier between them.
#include "zkwg_kernels.h"
#include "zkwg_ntt_core.h"

// the butterfly stages of a pass (zkwg_ntt_core.h zk_ntt_stage_pair / zk_ntt_stage_single), a barrier after each
template <bool DIT>
__device__ __forceinline__ void zk_ntt_stages(const ZkLds29& y, const ZkLds29& twl, u32 G, u32 g, u32 nel, u32 C) {
  u32 st = 0;
  for (; st + 1u < g; st += 2u) {
    zk_ntt_stage_pair<DIT>(y, twl, G, st, nel, C, threadIdx.x, 256u);
    __syncthreads();
  }
  if (st < g) {
    zk_ntt_stage_single<DIT>(y, twl, G, st, nel, C, threadIdx.x, 256u);
    __syncthreads();
  }
}

// One column pass (zkwg_ntt_core.h zk_ntt_col_wg).  Polynomial q = blockIdx.y.
template <bool DIT>
__global__ __launch_bounds__(256) void zk_ntt_col(ZkNttBuf src, ZkNttBuf dst,   /* launched in place: src may alias dst */
                                                   const Fr* __restrict__ tw, u32 L, u32 lb, u32 g, u32 inv) {
  extern __shared__ uint4 lds4[];
  const ZkNttColWg w = zk_ntt_col_wg(lds4, L, lb, g, inv, blockIdx.x, blockIdx.y);
  zk_ntt_col_load<DIT>(w, src, tw, threadIdx.x, 256u);
  __syncthreads();
  zk_ntt_stages<DIT>(w.y, w.twl, w.G, g, w.G, w.C);
  zk_ntt_col_store<DIT>(w, dst, tw, threadIdx.x, 256u);
}

// The row pass (zkwg_ntt_core.h zk_ntt_row_wg).  DIF (inverse direction of the pipeline): optional multiplication by scale[position]
// on the way out (coset shift and 1 / n).
template <bool DIT>
__global__ __launch_bounds__(256) void zk_ntt_row(ZkNttBuf src, ZkNttBuf dst,   /* launched in place: src may alias dst */
                                                   const Fr* __restrict__ tw, const Fr* __restrict__ scale, Fr uni, u32 use_uni, u32 L, u32 g, u32 inv) {
  extern __shared__ uint4 lds4[];
  const ZkNttRowWg w = zk_ntt_row_wg(lds4, L, g, inv, blockIdx.x, blockIdx.y);
  zk_ntt_row_load(w, src, tw, threadIdx.x, 256u);
  __syncthreads();
  zk_ntt_stages<DIT>(w.y, w.twl, w.G, g, w.TILE, 1u);
  zk_ntt_row_store(w, dst, scale, uni, use_uni, threadIdx.x, 256u);
}

// out[k] = a[k] b[k] - c[k] (zkwg_ntt_core.h zk_ntt_join_value), email e = blockIdx.y
__global__ __launch_bounds__(256) void zk_ntt_join(ZkNttBuf work, Fr* __restrict__ out, u64 n, u64 out_es) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  zk_ntt_join_thread(work, out, n, out_es, blockIdx.y, i);
}
// in-place bit-reversal permutation of n_polys arrays of 2^L elements (stand-alone transforms only: the pipeline needs none)
__global__ __launch_bounds__(256) void zk_ntt_bitrev(Fr* __restrict__ data, u32 L) {
  const u64 n = 1ull << L;
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  zk_ntt_bitrev_thread(data, L, blockIdx.y, i);
}

// ---- launch helpers (called from zkwg_ntt_api.hip) ---------------------------------------------------------------
// passes of one transform: column passes (block size 2^lb, 2^g-point sub-transforms), then the row pass (DIF), or the
// reverse (DIT).  src: canonical words (src_lazy = 0: polynomial q at src + (q / 3) src_es + (q % 3) src_ps, `valid` elements) or the
// work buffer itself; `work`: n_polys x 36 n bytes; the LAST pass writes to `out` when it is given (canonical words, polynomial q at
// out + q n: the stand-alone transforms), to the work buffer otherwise.
extern "C" int zk_ntt_launch(int dit, const Fr* src, u64 src_es, u64 src_ps, u64 valid, int src_lazy, void* work, Fr* out, const Fr* tw, const Fr* scale,
                             const Fr* uni_host, u32 L, u32 n_polys, u32 inv, hipStream_t st) {
  const Fr uni = uni_host ? *uni_host : fr_zero();
  const u32 use_uni = uni_host ? 1u : 0u;
  const u64 n = 1ull << L;
  const ZkNttSched sc = zk_ntt_sched(L);      // (zkwg_ntt_core.h: the host mirror runs the same schedule)
  const u32 tile = sc.tile;
  const size_t row_lds = zk_ntt_lds_bytes(tile, sc.g_row);
  const dim3 rgrid((u32)(n / tile), n_polys);
  const ZkNttBuf W{work, 0, 0, n, 1u};
  ZkNttBuf S = src_lazy ? W : ZkNttBuf{src, src_es, src_ps, valid, 0u};
  // canonical destination addressing is (q / 3) es + (q % 3) ps: consecutive polynomials n apart = es 3 n, ps n
  const ZkNttBuf OUT{out, 3u * n, n, n, 0u};
  if (!dit) {
    for (u32 i = 0; i < sc.ng; ++i) {
      hipLaunchKernelGGL((zk_ntt_col<false>), dim3((u32)(n / tile), n_polys), dim3(256), zk_ntt_lds_bytes(tile, sc.gs[i]), st, S, W, tw, L, sc.lb[i], sc.gs[i], inv);
      S = W;
    }
    hipLaunchKernelGGL((zk_ntt_row<false>), rgrid, dim3(256), row_lds, st, S, out ? OUT : W, tw, scale, uni, use_uni, L, sc.g_row, inv);
  } else {
    hipLaunchKernelGGL((zk_ntt_row<true>), rgrid, dim3(256), row_lds, st, S, (sc.ng == 0 && out) ? OUT : W, tw, (const Fr*)nullptr, uni, 0u, L, sc.g_row, inv);
    for (u32 i = sc.ng; i-- > 0;)
      hipLaunchKernelGGL((zk_ntt_col<true>), dim3((u32)(n / tile), n_polys), dim3(256), zk_ntt_lds_bytes(tile, sc.gs[i]), st, W, (i == 0 && out) ? OUT : W, tw, L, sc.lb[i], sc.gs[i], inv);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int zk_ntt_join_launch(const void* work, Fr* out, u64 n, u64 out_es, u32 n_emails, hipStream_t st) {
  const ZkNttBuf W{work, 0, 0, n, 1u};
  hipLaunchKernelGGL(zk_ntt_join, dim3((u32)((n + 255u) / 256u), n_emails), dim3(256), 0, st, W, out, n, out_es);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int zk_ntt_bitrev_launch(Fr* data, u32 L, u32 n_polys, hipStream_t st) {
  hipLaunchKernelGGL(zk_ntt_bitrev, dim3((u32)(((1ull << L) + 255u) / 256u), n_polys), dim3(256), 0, st, data, L);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
