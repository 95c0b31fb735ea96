// RevealSubstring(L, S, uniq) and CountSubstringOccurrences(L, S) -- helpers/reveal-substring.circom:13-50 with
// utils/array.circom:78-101 (SelectSubArray), :112-143 (VarShiftLeft), :196-217 (CheckSubstringMatch), :226-254
// (CountSubstringOccurrences) -- the mains of tests/test-circuits/reveal-substring-test.circom and
// count-substring-occurrences-test.circom.
//
// One wavefront evaluates one email.  in[] and the substring are staged as bytes (LDS on the device); what lands in the
// image is small: the range-check words, the revealed bytes, a word copy of in[] for VarShiftLeft.tmp, and per start position
// the number of leading positions whose difference is zero -- the 4 S + 2 kept signals of every CheckSubstringMatch
// component derive from that in zk_expand (zkwg_expand_dec.h ZkDecSubm).
//
// Written as ZK_PAR_FOR / ZK_SEQ phases like zkwg_rsa_core.h: compiled for the host the phases run in sequence
// (tests/native/substrtest.cpp).
#pragma once
#include "zkwg_sched.h"

#if defined(__HIPCC__)
#define ZK_SUB_LANE() (threadIdx.x & 63u)
#define ZK_SUB_PAR_FOR(i, n) for (u32 i = ZK_SUB_LANE(); i < (u32)(n); i += 64u)
#define ZK_SUB_SEQ if (ZK_SUB_LANE() == 0u)
#define ZK_SUB_SYNC() __syncthreads()
#define ZK_SUB_DEV __device__
#else
#define ZK_SUB_LANE() 0u
#define ZK_SUB_PAR_FOR(i, n) for (u32 i = 0; i < (u32)(n); ++i)
#define ZK_SUB_SEQ
#define ZK_SUB_SYNC()
#define ZK_SUB_DEV
#endif

ZK_HD u32 zk_sub_log2ceil(u64 a) { u64 n = a - 1; u32 r = 0; while (n > 0) { ++r; n >>= 1; } return r; }   // utils/functions.circom:7-17

// One email.  `ws`: zk_sub_lds_bytes(L, S) bytes of working set shared by the wavefront.  Returns the status to lane 0
// (0, or 4 = ZKWG_ERR_ASSERT_FAILED on exactly what the templates assert; other lanes' return value is unspecified).
ZK_SUB_DEV inline int zk_substr_core(const ZkSubLayout& U, u32 m_one, u32 range_flags_off, const u8* rec, u64* bits, u32* small, u8* ws) {
  const u32 L = U.L, S = U.S;
  u8* xin = ws;
  u8* xs = ws + ((L + 15u) & ~15u);
  u32* part = (u32*)(xs + ((S + 15u) & ~15u));   // [64] partial counts, [64] = failure flag
  const bool reveal = U.present == 1u;
  // stage in[] (and the count main's substring)
  ZK_SUB_PAR_FOR(i, L) {
    const u8 v = rec[U.in_in + i];
    xin[i] = v;
    if (reveal) small[U.m_in + i] = v;
  }
  if (!reveal) ZK_SUB_PAR_FOR(j, S) { const u8 v = rec[U.in_sub + j]; xs[j] = v; small[U.m_sub + j] = v; }
  ZK_SUB_PAR_FOR(l, 64u) part[l] = 0u;
  u32 start = 0, len = 0;
  if (reveal) {
    start = *(const u32*)(rec + U.in_start);
    len = *(const u32*)(rec + U.in_len);
  }
  ZK_SUB_SEQ {
    u32 bad = *(const u32*)(rec + range_flags_off) != 0u;
    small[m_one] = 1u;
    if (reveal) {
      // isSubstringStartIndexValid / isSubstringLengthValid / isSumValid (reveal-substring.circom:23-33): LessThan(b)(x, y) has
      // n2b.in = x + 2^b - y
      const u32 b0 = zk_sub_log2ceil(L), b1 = zk_sub_log2ceil((u64)S + 1u), b2 = zk_sub_log2ceil((u64)L + 1u);
      const u64 sum = (u64)start + len;
      bits[U.b_lt] = (u64)start + (1ull << b0) - L;
      bits[U.b_lt + 1] = (u64)len + (1ull << b1) - (S + 1u);
      bits[U.b_lt + 2] = sum + (1ull << b2) - (L + 1u);
      if (start >= L || len > S || sum > L) bad = 1u;
      bits[U.b_shift] = start;                    // VarShiftLeft.n2b = Num2Bits(log2Ceil(L))(shift)
      small[U.m_start] = start; small[U.m_start + 1] = len;
    }
    part[64] = bad;
  }
  ZK_SUB_SYNC();
  if (reveal) {
    // gts[i] = GreaterThan(lg)(length, i) = LessThan(lg)(i, length): n2b.in = i + 2^lg - length, out = 1 - bit lg;
    // out[i] = gts[i].out * shifter.out[i], shifter.out[i] = in[(i + shift) mod L] (array.circom:90-100, :128-142)
    const u32 lg = zk_sub_log2ceil(S), b0 = zk_sub_log2ceil(L);
    const u32 sh = start & ((1u << b0) - 1u);
    ZK_SUB_PAR_FOR(i, S) {
      const u64 w = ((u64)i + (1ull << lg) - (u64)len) & ((2ull << lg) - 1ull);   // (a length above S fails its range check)
      bits[U.b_gts + i] = w;
      const u32 g = 1u - (u32)((w >> lg) & 1ull);
      const u8 v = g ? xin[(i + sh) % L] : (u8)0;
      xs[i] = v;
      small[U.m_sub + i] = v;
    }
    ZK_SUB_SYNC();
  }
  if (U.uniq) {
    // matches[i] = CheckSubstringMatch(S)(in[i ..] zero-filled, substring): difference[j] = (in[i + j] - substring[j]) substring[j];
    // matchAccumulator[j + 1] = 1 while every difference so far is zero (array.circom:207-216, :236-245)
    u32 cnt = 0;
    ZK_SUB_PAR_FOR(i, L) {
      u32 m = 0;
      while (m < S) {
        const int s = xs[m], x = i + m < L ? (int)xin[i + m] : 0;
        if ((x - s) * s != 0) break;
        ++m;
      }
      small[U.m_sub + S + i] = m;
      cnt += (u32)(m == S);
    }
    part[ZK_SUB_LANE()] += cnt;
    ZK_SUB_SYNC();
    ZK_SUB_SEQ {
      u32 count = 0;
      for (u32 l = 0; l < 64u; ++l) count += part[l];
      if (xs[0] == 0) part[64] = 1u;                        // firstElementNonZero === 0 (array.circom:203-205)
      if (reveal) { if (count != 1u) part[64] = 1u; }       // countSubstringOccurrences.count === 1 (reveal-substring.circom:46)
      else small[U.m_count] = count;
    }
  }
  ZK_SUB_SYNC();
  return part[64] ? 4 : 0;
}
