// Kernel declarations (definitions in zkwg_kernels_*.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "zkwg_sched.h"
#include "zkwg_o0.h"

__global__ void zk_sha_chain(ZkSched s, ZkBufs B);   // zkwg_kernels_sha.hip
template <bool REC, bool TRACE> __global__ void zk_sha_trace(ZkSched s, ZkBufs B);   // zkwg_kernels_sha.hip: <records, trace> = <0,1>, <1,0>, <1,1>
__global__ void zk_rsa(ZkSched s, ZkBufs B);         // zkwg_kernels_rsa.hip
__global__ void zk_fpmul_small(ZkSched s, ZkBufs B);
__global__ void zk_substr(ZkSched s, ZkBufs B);      // zkwg_kernels_substr.hip
__global__ void zk_app_tail(ZkSched s, ZkBufs B);    // zkwg_kernels_app.hip
__global__ void zk_cea_chunks(ZkSched s, ZkBufs B);  // zkwg_kernels_cea.hip (evaluator: zkwg_poseidon29.h, V = 6)
__global__ void zk_cea_tail(ZkSched s, ZkBufs B);
__global__ void zk_poseidon9(ZkSched s, ZkBufs B);   // zkwg_kernels_rsa.hip
__global__ void zk_poseidon9_wave(ZkSched s, ZkBufs B);
__global__ void zk_poseidon9_g16(ZkSched s, ZkBufs B);
__global__ void zk_misc_ev(ZkSched s, ZkBufs B);     // zkwg_kernels_misc.hip
__global__ void zk_net_eval(ZkSched s, ZkBufs B);    // zkwg_kernels_net.hip
__global__ void zk_net_scan(ZkSched s, ZkBufs B);
__global__ void zk_rslb_chunks(ZkSched s, ZkBufs B); // zkwg_kernels_rslb.hip (evaluator: zkwg_poseidon29.h, V = 6)
#include "zkwg_rslb_wave.h"   // ZK_RS_MERGE_LANES
__global__ void zk_rslb_merge(ZkSched s, ZkBufs B);
__global__ void zk_rslb_merge1(ZkSched s, ZkBufs B);     // the same chain, one lane per email in limb form
__global__ void zk_rslb_classify(ZkSched s, ZkBufs B);   // constant chunks: the units to hash | the all-zero ones
__global__ void zk_rslb_fill_const(ZkSched s, ZkBufs B);
__global__ void zk_rslb_scan(ZkSched s, ZkBufs B);
__global__ void zk_r1cs_check(const u64* row_ptr, const u32* wire, const Fr* coef, const u8* kind, u32 m,
                              const u8* wit, u64 stride, unsigned long long* first_bad);  // zkwg_kernels_r1cs.hip
__global__ void zk_r1cs_eval(const u64* row_ptr, const u32* wire, const Fr* coef, const u8* kind, u32 m, const u8* wit, u64 stride,
                             u8* out, u64 out_stride, int mont);  // zkwg_kernels_r1cs.hip
// zkwg_kernels_expand3.hip: one piece of 256 K slots per workgroup, standard / Montgomery form; K slots per lane: ZK_X3_SLOTS,
// ZK_X3_SLOTS_O0 (zkwg_sched.h)
__global__ void zk_expand3(ZkX3 A); __global__ void zk_expand3_mont(ZkX3 A);
__global__ void zk_expand3_o0(ZkX3 A, ZkO0Dev O); __global__ void zk_expand3_o0_mont(ZkX3 A, ZkO0Dev O);
__global__ void zk_image_to_mont(ZkX3 A);
__global__ void zk_expand3_subm(ZkX3 A);             // zkwg_kernels_substr.hip: zk_expand3 with the ZSEG_SUBM decoder (substring mains)
__global__ void zk_expand3_cea(ZkX3 A);              // zkwg_kernels_cea.hip: zk_expand3 with the ZSEG_CEA decoder (CleanEmailAddress)
__global__ void zk_o0_rows_small(ZkX3 A, ZkO0Dev O);
__global__ void zk_o0_chains_small(ZkX3 A, ZkO0Dev O);
__global__ void zk_o0_generic(ZkX3 A, ZkO0Dev O);
__global__ void zk_o0_rows_small_long(ZkX3 A, ZkO0Dev O);
#define ZK_ROW_EMAILS 8   // emails per thread of zk_o0_rows_small
__global__ void zk_o0_rows_fr(ZkX3 A, ZkO0Dev O);
__global__ void zk_mont_convert(Fr* v, u64 n, int to_mont);  // zkwg_kernels_handoff.hip
__global__ void zk_gen_inputs(ZkSched s, ZkDkimBatch D, u8* recs, int* gen_status, u32 n);  // zkwg_kernels_inputs.hip
__global__ void zk_gen_reveal_inputs(ZkSched s, ZkDkimBatch D, ZkNeedles Q, u8* recs, int* gen_status, u32 n);
