// SHA-256 round states: the compact form of one Sha256compression instance in the image, its writer and its slot decoders.
//
// The 30,952 kept signals of a compression (zkwg_sched.h) are the bits of 952 groups of 32..35 bits -- the TRACE, one u64 word per
// group (7,616 bytes per block).  Every group is a short function of the round's working variables and the message schedule, so
// the image of an EmailVerifier handle holds one RECORD of ZK_SHAR_WORDS = 200 u32 per block instead (800 bytes, in `small`,
// 16-byte aligned), and zk_expand's decoders recompute the group a slot belongs to:
//   W[0..63]    at ZK_SHAR_W + t   the message schedule
//   A[-4..63]   at ZK_SHAR_A + t   A[-1..-4] = hin[0..3], A[t] = the new `a` after round t = (u32)suma_t
//   E[-4..63]   at ZK_SHAR_E + t   E[-1..-4] = hin[4..7], E[t] = (u32)sume_t
// At the start of round t the working variables are (a,b,c,d) = A[t-1..t-4] and (e,f,g,h) = E[t-1..t-4].
// The trace itself is still written for the readers that address its words one by one: the descriptor tables of numbered
// (`--O0` / `--O1`) circuits and attached constraint systems (zkwg_o0.h), and the Sha256Bytes main, whose image keeps the
// documented word-by-word form (include/zkwg.h "compact image") and has no record.
// Plain C++ so that the CPU tests compile the writer and the decoders as they are (tests/native/shacompacttest.cpp).
#pragma once
#include "zkwg_sched.h"

#define ZK_SHAR_WORDS 200u
#define ZK_SHAR_W 0u
#define ZK_SHAR_A 68u    // word of A[0]: A[-4] is word 64
#define ZK_SHAR_E 136u   // word of E[0]: E[-4] is word 132

ZK_HD u32 zk_shar_rotr(u32 x, u32 r) { return (x >> r) | (x << (32u - r)); }
ZK_HD u32 zk_sha_k(u32 t) {
  static constexpr u32 K[64] = {
      0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
      0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
      0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
      0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
      0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
      0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
      0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
      0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
  return K[t];
}
// four consecutive words: a 16-byte access where the address allows it (the writer's are aligned, a decoder's start at any word)
struct ZkW4 { u32 x, y, z, w; };
ZK_HD ZkW4 zk_ld4(const u32* p) { ZkW4 v; __builtin_memcpy(&v, p, 16); return v; }
ZK_HD void zk_st4_aligned(u32* p, u32 x, u32 y, u32 z, u32 w) { const ZkW4 v{x, y, z, w}; __builtin_memcpy(__builtin_assume_aligned(p, 16), &v, 16); }

// ---------------------------------------------------------------- writer
// The 64 rounds of one block: w[0..15] = the block's message words (w[16..63] are filled in), hin = the chaining state before the
// block.  REC: the record at `rec` (16-byte aligned).  TRACE: the 952 groups at `tr`, one u64 per kept bit-group, bit k of a group =
// the signal with index k (circomlib bit vectors are LSB-first), group order = layout order inside the block (zkwg_sched.h).
template <bool REC, bool TRACE>
ZK_HD void zk_sha_rounds(u32 (&w)[64], const u32* hin, u32* rec, u64* tr) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int t = 16; t < 64; ++t) {  // sigmaPlus[t-16]
    const u32 x2 = w[t - 2], x15 = w[t - 15];
    const u32 a1 = zk_shar_rotr(x2, 17), b1 = zk_shar_rotr(x2, 19), c1 = x2 >> 10;
    const u32 a0 = zk_shar_rotr(x15, 7), b0 = zk_shar_rotr(x15, 18), c0 = x15 >> 3;
    const u32 s1 = a1 ^ b1 ^ c1, s0 = a0 ^ b0 ^ c0;
    const u64 sum = (u64)s1 + w[t - 7] + s0 + w[t - 16];
    if constexpr (TRACE) {
      u64* g = tr + ZK_G_SP + (t - 16) * 5;
      g[0] = s1; g[1] = b1 & c1; g[2] = s0; g[3] = b0 & c0; g[4] = sum;
    }
    w[t] = (u32)sum;
  }
  const u32 h0 = hin[0], h1 = hin[1], h2 = hin[2], h3 = hin[3], h4 = hin[4], h5 = hin[5], h6 = hin[6], h7 = hin[7];
  if constexpr (REC) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int t = 0; t < 64; t += 4) zk_st4_aligned(rec + ZK_SHAR_W + t, w[t], w[t + 1], w[t + 2], w[t + 3]);
    zk_st4_aligned(rec + ZK_SHAR_A - 4, h3, h2, h1, h0);
    zk_st4_aligned(rec + ZK_SHAR_E - 4, h7, h6, h5, h4);
  }
  u32 a = h0, b = h1, c = h2, d = h3, e_ = h4, f_ = h5, g_ = h6, h = h7;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int t = 0; t < 64; ++t) {
    const u32 eb = zk_shar_rotr(e_, 11), ec = zk_shar_rotr(e_, 25);
    const u32 bs1 = zk_shar_rotr(e_, 6) ^ eb ^ ec;
    const u32 ch = (e_ & f_) ^ (~e_ & g_);
    const u64 t1 = (u64)h + bs1 + ch + zk_sha_k(t) + w[t];
    const u32 ab = zk_shar_rotr(a, 13), ac = zk_shar_rotr(a, 22);
    const u32 bs0 = zk_shar_rotr(a, 2) ^ ab ^ ac;
    const u32 mmid = b & c;
    const u32 maj = (a & (b ^ c)) | mmid;
    const u64 t2 = (u64)bs0 + maj;
    const u64 sume = (u64)d + (u32)t1;
    const u64 suma = (u64)(u32)t1 + (u32)t2;
    if constexpr (TRACE) {
      u64* g1 = tr + ZK_G_T1 + t * 4;
      g1[0] = ch; g1[1] = bs1; g1[2] = eb & ec; g1[3] = t1;
      u64* g2 = tr + ZK_G_T2 + t * 5;
      g2[0] = bs0; g2[1] = ab & ac; g2[2] = maj; g2[3] = mmid; g2[4] = t2;
      tr[ZK_G_SUMA + t] = suma;
      tr[ZK_G_SUME + t] = sume;
    }
    h = g_; g_ = f_; f_ = e_; e_ = (u32)sume; d = c; c = b; b = a; a = (u32)suma;
    if (REC && (t & 3) == 3) {   // (a,b,c,d) = A[t..t-3], (e,f,g,h) = E[t..t-3]
      zk_st4_aligned(rec + ZK_SHAR_A + t - 3, d, c, b, a);
      zk_st4_aligned(rec + ZK_SHAR_E + t - 3, h, g_, f_, e_);
    }
  }
  if constexpr (TRACE) {
    tr[ZK_G_FSUM + 0] = (u64)h0 + a; tr[ZK_G_FSUM + 1] = (u64)h1 + b;
    tr[ZK_G_FSUM + 2] = (u64)h2 + c; tr[ZK_G_FSUM + 3] = (u64)h3 + d;
    tr[ZK_G_FSUM + 4] = (u64)h4 + e_; tr[ZK_G_FSUM + 5] = (u64)h5 + f_;
    tr[ZK_G_FSUM + 6] = (u64)h6 + g_; tr[ZK_G_FSUM + 7] = (u64)h7 + h;
  }
}

// ---------------------------------------------------------------- slot decoders
// Slot r of the block's sigmaPlus / t1 / t2 / (suma | sume | fsum) signals from its record: the loads do not depend on which
// group of the period the slot is in, so they are issued first; then only that group is computed.  Same values as the trace.
ZK_HD u32 zk_shar_bit(u64 v, u32 bit) { return (u32)(v >> bit) & 1u; }
// sigmaPlus[i], i = r / 162: sigma1.xor3.out32, .mid32, sigma0.xor3.out32, .mid32, sum.out34 over W[t-2], W[t-15], W[t-7], W[t-16], t = i + 16
ZK_HD u32 zk_shar_sp(const u32* rec, u32 r) {
  const u32 i = r / ZK_SP_SLOTS, q = r - i * ZK_SP_SLOTS;
  const u32 sub = (q >> 5) < 4u ? (q >> 5) : 4u, bit = q - sub * 32u;
  const u32* w = rec + ZK_SHAR_W + i;   // W[t-16]
  const u32 x16 = w[0], x15 = w[1], x7 = w[9], x2 = w[14];
  const u32 b1 = zk_shar_rotr(x2, 19), c1 = x2 >> 10, s1 = zk_shar_rotr(x2, 17) ^ b1 ^ c1;
  const u32 b0 = zk_shar_rotr(x15, 18), c0 = x15 >> 3, s0 = zk_shar_rotr(x15, 7) ^ b0 ^ c0;
  const u64 v = sub == 0u ? s1 : sub == 1u ? (b1 & c1) : sub == 2u ? s0 : sub == 3u ? (b0 & c0) : (u64)s1 + x7 + s0 + x16;
  return zk_shar_bit(v, bit);
}
// t1[t], t = r / 131: ch.out32, bigsigma1.xor3.out32, .mid32, sum.out35
ZK_HD u32 zk_shar_t1(const u32* rec, u32 r) {
  const u32 t = r / ZK_T1_SLOTS, q = r - t * ZK_T1_SLOTS;
  const u32 sub = (q >> 5) < 3u ? (q >> 5) : 3u, bit = q - sub * 32u;
  const ZkW4 s = zk_ld4(rec + ZK_SHAR_E + t - 4);   // h, g, f, e
  const u32 wt = rec[ZK_SHAR_W + t], k = zk_sha_k(t);
  const u32 e = s.w, eb = zk_shar_rotr(e, 11), ec = zk_shar_rotr(e, 25);
  const u32 bs1 = zk_shar_rotr(e, 6) ^ eb ^ ec, ch = (e & s.z) ^ (~e & s.y);
  const u64 v = sub == 0u ? ch : sub == 1u ? bs1 : sub == 2u ? (eb & ec) : (u64)s.x + bs1 + ch + k + wt;
  return zk_shar_bit(v, bit);
}
// t2[t], t = r / 161: bigsigma0.xor3.out32, .mid32, maj.out32, .mid32, sum.out33
ZK_HD u32 zk_shar_t2(const u32* rec, u32 r) {
  const u32 t = r / ZK_T2_SLOTS, q = r - t * ZK_T2_SLOTS;
  const u32 sub = (q >> 5) < 4u ? (q >> 5) : 4u, bit = q - sub * 32u;
  const ZkW4 s = zk_ld4(rec + ZK_SHAR_A + t - 4);   // d, c, b, a
  const u32 a = s.w, ab = zk_shar_rotr(a, 13), ac = zk_shar_rotr(a, 22);
  const u32 bs0 = zk_shar_rotr(a, 2) ^ ab ^ ac, mmid = s.z & s.y, maj = (a & (s.z ^ s.y)) | mmid;
  const u64 v = sub == 0u ? bs0 : sub == 1u ? (ab & ac) : sub == 2u ? maj : sub == 3u ? mmid : (u64)bs0 + maj;
  return zk_shar_bit(v, bit);
}
// suma[64], sume[64], fsum[8], 33 bits each.  With x = E[t] - A[t-4] (mod 2^32, = (u32)t1): sume = A[t-4] + x and
// suma = x + (u32)(A[t] - x); fsum[j] = hin[j] + {A[63..60], E[63..60]}[j]
ZK_HD u32 zk_shar_sum(const u32* rec, u32 r) {
  const u32 g = r / 33u, bit = r - g * 33u;
  u32 i0, i1, i2;
  if (g < 128u) {
    const u32 t = g & 63u;
    i0 = ZK_SHAR_E + t; i1 = ZK_SHAR_A + t - 4u; i2 = ZK_SHAR_A + t;
  } else {
    const u32 j = g - 128u, base = j < 4u ? ZK_SHAR_A : ZK_SHAR_E + 4u;   // hin[j] = A[-1-j] / E[-1-(j-4)]
    i0 = base - 1u - j; i1 = base + 63u - j; i2 = i0;
  }
  const u32 l0 = rec[i0], l1 = rec[i1], l2 = rec[i2];
  const u32 x = l0 - l1;
  const u64 v = g < 64u ? (u64)x + (u32)(l2 - x) : g < 128u ? (u64)l1 + x : (u64)l0 + l1;
  return zk_shar_bit(v, bit);
}
