// EmailReveal's own outputs (circuits/email-reveal.circom): what the main adds to EmailVerifier and RevealSubstring.
//
//   revealed[c]    = PackBytes(S)(rs.substring)[c] (utils/bytes.circom:28-60): the little-endian integer of the up to 31
//                    revealed bytes 31 c .. 31 c + 30, as a field element
//   emailNullifier = Poseidon(1)(PoseidonLarge(121, 17)(signature)) (helpers/email-nullifier.circom:15-23,
//                    utils/hash.circom:15-39) with the 420 + 216 S-box signals of the two permutations
//
// Everything is formed from the input record alone -- the revealed bytes are selected again with the gate and the shift of
// SelectSubArray (zkwg_substr_core.h) instead of being read from zk_substr's words -- so zk_app_tail and zk_substr run side by
// side.  One email per lane; the permutation state (and the dense mixes' temporaries) are addressed with a stride, LDS
// columns on the device.  Plain functions: compiled for the host by tests/native/apptest.cpp.
#pragma once
#include "zkwg_sched.h"
#include "zkwg_poseidon_sparse.h"

// byte i of rs.substring: in[(i + startIndex) mod L] while i < length, else 0 (utils/array.circom:90-100, :128-142)
ZK_HD u32 zk_app_revealed_byte(const u8* src, u32 L, u32 S, u32 start, u32 len, u32 i) {
  u32 b0 = 0, lg = 0;
  for (u64 n = (u64)L - 1; n > 0; n >>= 1) ++b0;            // log2Ceil(L), log2Ceil(S) (utils/functions.circom:7-17)
  for (u64 n = (u64)S - 1; n > 0; n >>= 1) ++lg;
  const u64 w = ((u64)i + (1ull << lg) - (u64)len) & ((2ull << lg) - 1ull);   // gts[i] = LessThan(lg)(i, length): 1 - bit lg
  if ((w >> lg) & 1ull) return 0u;
  const u32 sh = start & ((1u << b0) - 1u);
  return src[(i + sh) % L];
}

// revealed[c], standard form: 31 bytes fill 248 bits of the four limbs
ZK_HD Fr zk_app_pack_chunk(const u8* src, u32 L, u32 S, u32 start, u32 len, u32 c) {
  u64 l0 = 0, l1 = 0, l2 = 0, l3 = 0;
  for (u32 j = 0; j < ZK_APP_PACK; ++j) {
    const u32 i = ZK_APP_PACK * c + j;
    if (i >= S) break;
    const u64 v = zk_app_revealed_byte(src, L, S, start, len, i);
    const u32 sh = 8u * (j & 7u);
    // (selects, not an indexed array: a runtime limb index would put the element in scratch memory)
    if (j < 8u) l0 |= v << sh; else if (j < 16u) l1 |= v << sh; else if (j < 24u) l2 |= v << sh; else l3 |= v << sh;
  }
  return Fr{{l0, l1, l2, l3}};
}

// poseidonInput[i] = in[2i] + 2^121 in[2i+1] (i < 8), in[16] (i = 8) of PoseidonLarge(121, 17) over 17 16-byte limbs
ZK_HD Fr zk_app_large_input(const u8* limbs, u32 i) {
  const u64 top_mask = (1ull << 57) - 1;
  const u64* lo = (const u64*)(limbs + 16 * (2 * i));
  Fr v{{lo[0], lo[1] & top_mask, 0, 0}};
  if (i < 8) {
    const u64* hp = (const u64*)(limbs + 16 * (2 * i + 1));
    const u64 h0 = hp[0], h1 = hp[1] & top_mask;
    v.l[1] |= h0 << 57;
    v.l[2] = (h0 >> 7) | (h1 << 57);
    v.l[3] = h1 >> 7;
  }
  return v;
}

// One email.  `pos9` / `pos1`: sparse-round tables of t = 10 (R_P = 60) and t = 2 (R_P = 56) (zk_build_poseidon_sparse);
// `st`, `tmp`: 10 field elements each with stride `ss` (this email's own).  Writes frv[A.f_out ..] and frv[A.f_pos ..].
ZK_HD void zk_app_core(const ZkAppLayout& A, const u8* rec, Fr* frv, const Fr* pos9, const Fr* pos1, Fr* st, Fr* tmp, const u32 ss) {
  const u32 start = *(const u32*)(rec + A.in_start), len = *(const u32*)(rec + A.in_len);
  for (u32 c = 0; c < A.chunks; ++c)
    frv[A.f_out + A.nullifier + c] = zk_app_pack_chunk(rec + A.in_src, A.src_len, A.S, start, len, c);
  if (!A.nullifier) return;
  st[0] = fr_zero();
  for (u32 i = 0; i < 9; ++i) st[(1 + i) * ss] = zk_app_large_input(rec + A.in_sig, i);
  const Fr h9 = zk_poseidon_sparse<10>(st, ss, pos9, 60, frv + A.f_pos, tmp, ss);     // signatureHash (linear: not kept)
  st[0] = fr_zero();
  st[ss] = h9;
  frv[A.f_out] = zk_poseidon_sparse<2>(st, ss, pos1, 56, frv + A.f_pos + ZK_P9_KEPT, tmp, ss);
}
