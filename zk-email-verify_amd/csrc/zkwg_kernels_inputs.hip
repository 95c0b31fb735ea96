// zk_gen_inputs -- batched input generation on the device: restates
// generateEmailVerifierInputsFromDKIMResult (packages/helpers/src/input-generators.ts:190-252),
// sha256Pad / generatePartialSHA / findIndexInUint8Array (sha-utils.ts:9-111, incl. the SHA-256 midstate of
// lib/fast-sha256.ts:240-251 cacheState) and toCircomBigIntBytes (binary-format.ts:71-83).
// One wavefront per email: raw canonical header / body bytes + 2048-bit big-endian key and signature
// in, one packed input record out.  The per-email error codes mirror the reference's thrown errors.
#include "zkwg_gen_inputs_body.h"
#include "zkwg_kernels.h"

__global__ __launch_bounds__(64) void zk_gen_inputs(ZkSched s, ZkDkimBatch D, u8* __restrict__ recs,
                                                   int* __restrict__ gen_status, u32 n) {
  __shared__ alignas(16) u8 lds[ZK_GEN_LDS];
  zk_gen_inputs_body<false>(s, D, ZkNeedles{nullptr, nullptr}, recs, gen_status, n, lds);
}

// EmailReveal's records from one needle per email (zkwg_generate_reveal_inputs_device): the same walk, the cut and the two
// indices from the search of csrc/zkwg_locate_core.h
__global__ __launch_bounds__(64) void zk_gen_reveal_inputs(ZkSched s, ZkDkimBatch D, ZkNeedles Q, u8* __restrict__ recs,
                                                          int* __restrict__ gen_status, u32 n) {
  __shared__ alignas(16) u8 lds[ZK_GEN_LDS + ZK_LOC_LDS];
  zk_gen_inputs_body<true>(s, D, Q, recs, gen_status, n, lds);
}
