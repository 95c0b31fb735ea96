// DKIM verification of raw emails on gfx950 (the cores are csrc/zkwg_dkim_core.h):
//
//   zk_dkim_body     one wavefront per email: the canonical body (relaxed or simple) of its raw body into [n][body_stride] and its
//                    length -- the two arrays of zkwg_dkim_batch.  16 raw bytes per lane and step, one wave-exclusive scan, the emitted
//                    bytes staged in LDS and stored to contiguous addresses.
//   zk_dkim_hash     one lane per stream: SHA-256 of the n canonical bodies and of the n canonical headers, with the compression
//                    function of the witness path (zk_sha256_compress, csrc/zkwg_dev.h); the padded last block of a stream is built
//                    in the lane's 64 bytes of LDS.
//   zk_dkim_verify   one wavefront per email: bh= against the body digest, then sig^65537 mod n against EMSA-PKCS1-v1_5 of the header
//                    digest for each candidate key in turn (csrc/zkwg_rsa_wave.h: zkw_barrett_mu, zkw_mulmod); the first key that
//                    verifies wins.  Precedence as lib/mailauth/dkim-verifier.ts:245-335: body hash, then key, then signature.
#include "zkwg_dev.h"
#include "zkwg_dkim_core.h"

__global__ __launch_bounds__(64) void zk_dkim_body(const ZkDkimRec* __restrict__ recs, const u8* __restrict__ raw, u8* __restrict__ bodies,
                                                  u32* __restrict__ body_len, u32* __restrict__ fits, u32 stride, u32 n) {
  const u32 e = blockIdx.x;
  if (e >= n) return;
  __shared__ __attribute__((aligned(16))) u8 stage[ZK_DKIM_STAGE];
  const ZkDkimRec& r = recs[e];
  u32 f = 1, len = 0;
  if (r.pre_status == 0) len = zkw_dkim_body(raw + r.raw_off, r.raw_len, r.body_mode, r.has_l != 0, r.l, bodies + (u64)e * stride, stride, stage, &f);
  if (threadIdx.x == 0) { body_len[e] = len; fits[e] = f; }
}

__global__ __launch_bounds__(64) void zk_dkim_hash(const ZkDkimRec* __restrict__ recs, const u8* __restrict__ bodies, const u32* __restrict__ body_len,
                                                  const u32* __restrict__ fits, u32 body_stride, const u8* __restrict__ headers,
                                                  const u32* __restrict__ header_len, u32 header_stride, u8* __restrict__ body_digest,
                                                  u8* __restrict__ header_digest, u32 n) {
  __shared__ __attribute__((aligned(16))) u8 tails[64][64];
  const u32 g = blockIdx.x * 64u + threadIdx.x;
  if (g >= 2u * n) return;
  const bool is_header = g >= n;
  const u32 e = is_header ? g - n : g;
  u8* out = (is_header ? header_digest : body_digest) + 32ull * e;
  u32 st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (recs[e].pre_status == 0 && (is_header || fits[e])) {
    const u8* data = is_header ? headers + (u64)e * header_stride : bodies + (u64)e * body_stride;
    const u32 len = is_header ? header_len[e] : body_len[e];
    if (len <= (is_header ? header_stride : body_stride))
      zk_dkim_sha256(data, len, tails[threadIdx.x], st, [](u32* s, const u8* blk) { zk_sha256_compress(s, blk); });
  }
#pragma unroll
  for (u32 j = 0; j < 8; ++j) *(u32*)(out + 4 * j) = __builtin_bswap32(st[j]);
}

__global__ __launch_bounds__(64) void zk_dkim_verify(const ZkDkimRec* __restrict__ recs, const ZkDkimKey* __restrict__ keys, const u32* __restrict__ fits,
                                                    const u8* __restrict__ body_digest, const u8* __restrict__ header_digest,
                                                    const u8* __restrict__ signature_be, u32 flags, int* __restrict__ status,
                                                    int* __restrict__ key_index, u8* __restrict__ pubkey_be, u32 n) {
  const u32 e = blockIdx.x;
  if (e >= n) return;
  __shared__ ZkRsaLds S;
  const u32 lane = threadIdx.x;
  const ZkDkimRec& r = recs[e];
  int st = r.pre_status, idx = -1;
  if (!st && !fits[e]) st = ZK_DKIM_ST_DOES_NOT_FIT;
  if (!st && !(flags & 1u)) {
    const bool differs = lane < 32 && body_digest[32ull * e + lane] != r.bh[lane];
    if (__ballot(differs) != 0) st = ZK_DKIM_ST_BODY_HASH;
  }
  if (!st && r.key_count == 0) st = ZK_DKIM_ST_NO_KEY;
  if (!st) {
    u32 usable = 0;
    for (u32 k = 0; k < r.key_count && idx < 0; ++k) {
      const ZkDkimKey& key = keys[r.key_first + k];
      if (!zk_dkim_key_usable(key.bits, key.exponent)) continue;
      ++usable;
      if (zkw_dkim_rsa(S, key.modulus_be, signature_be + 256ull * e, header_digest + 32ull * e)) idx = (int)k;
    }
    if (idx < 0) st = usable ? ZK_DKIM_ST_BAD_SIGNATURE : ZK_DKIM_ST_UNSUPPORTED;
  }
  const u32 pick = idx >= 0 ? (u32)idx : 0u;
  for (u32 i = lane; i < 256; i += 64) pubkey_be[256ull * e + i] = r.key_count ? keys[r.key_first + pick].modulus_be[i] : 0;
  if (lane == 0) { status[e] = st; key_index[e] = idx; }
}

// ------------------------------------------------------------------ launches (csrc/zkwg_dkim_api.hip)
void zk_dkim_body_launch(const void* recs, const void* raw, void* bodies, void* body_len, void* fits, u32 stride, u32 n, hipStream_t st) {
  if (n) hipLaunchKernelGGL(zk_dkim_body, dim3(n), dim3(64), 0, st, (const ZkDkimRec*)recs, (const u8*)raw, (u8*)bodies, (u32*)body_len, (u32*)fits, stride, n);
}
void zk_dkim_hash_launch(const void* recs, const void* bodies, const void* body_len, const void* fits, u32 body_stride, const void* headers,
                         const void* header_len, u32 header_stride, void* body_digest, void* header_digest, u32 n, hipStream_t st) {
  if (n) hipLaunchKernelGGL(zk_dkim_hash, dim3((2 * n + 63) / 64), dim3(64), 0, st, (const ZkDkimRec*)recs, (const u8*)bodies, (const u32*)body_len, (const u32*)fits,
                            body_stride, (const u8*)headers, (const u32*)header_len, header_stride, (u8*)body_digest, (u8*)header_digest, n);
}
void zk_dkim_verify_launch(const void* recs, const void* keys, const void* fits, const void* body_digest, const void* header_digest, const void* signature_be,
                           u32 flags, void* status, void* key_index, void* pubkey_be, u32 n, hipStream_t st) {
  if (n) hipLaunchKernelGGL(zk_dkim_verify, dim3(n), dim3(64), 0, st, (const ZkDkimRec*)recs, (const ZkDkimKey*)keys, (const u32*)fits, (const u8*)body_digest,
                            (const u8*)header_digest, (const u8*)signature_be, flags, (int*)status, (int*)key_index, (u8*)pubkey_be, n);
}
