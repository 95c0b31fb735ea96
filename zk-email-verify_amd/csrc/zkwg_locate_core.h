// Substring search over a byte stream, one wavefront per stream: the first occurrence of a needle in src[0, len), or the
// number of its occurrences there (overlapping ones count, as CountSubstringOccurrences of utils/array.circom counts them).  An
// occurrence lies wholly inside [0, len): one that starts inside and ends beyond is none.  It is what zk_gen_reveal_inputs
// (csrc/zkwg_gen_inputs_body.h) finds the revealed string with, in canonical bodies of any length, and counts it with in the record.
//
// Two builds: the gfx950 kernel, and the CPU tests on the simulated wavefront (tests/native/locatetest.cpp with ZKWG_WAVESIM).
//
// The walk.  A tile is ZK_LOC_TILE = 1,024 start positions, 16 consecutive ones per lane.  The wavefront stages the tile's bytes and the
// bytes behind it that a match starting in the tile can reach in LDS, beside the needle: one 16-byte load per lane where the address
// allows it, single bytes otherwise (any base, any stride).  A lane keeps a 16-bit candidate mask: a position is a candidate when the
// needle still fits there and its first byte -- taken from the lane's own 16 loaded bytes, in registers -- equals the needle's; the
// candidates are compared in full out of LDS.  A needle longer than ZK_LOC_CHUNK is compared in chunks of that many bytes: the window
// and the needle chunk are staged again at the chunk's offset and only the surviving candidates look at it; a tile without survivors
// leaves the chunk loop at once.  All branches around the staging and the ballots are wavefront-uniform.
// Between tiles the function carries the tile's offset and (count) a per-lane sum; nothing else.  FIRST leaves at the first tile with
// a hit: __ballot finds the lane, __ffsll the position in its mask.  COUNT adds __popcll of the masks and reduces once at the end.
#pragma once
#include "zkwg_rsa_core.h"

#define ZK_LOC_LANE_BYTES 16u
#define ZK_LOC_TILE (64u * ZK_LOC_LANE_BYTES)
#define ZK_LOC_CHUNK 256u                                   // needle bytes compared per staging
#define ZK_LOC_WIN (ZK_LOC_TILE + ZK_LOC_CHUNK)             // staged source bytes (the last one is never read)
#define ZK_LOC_LDS (ZK_LOC_WIN + ZK_LOC_CHUNK)              // LDS the caller provides, 16-byte aligned
#define ZK_LOC_NONE 0xffffffffu
#define ZK_LOC_FIRST 0u
#define ZK_LOC_COUNT 1u

// the same search, serially: the statement the wavefront function is checked against on the device = -1 side of the tests
inline u32 zk_locate_serial(const u8* src, u32 len, const u8* nd, u32 L, u32 what) {
  u32 count = 0;
  for (u32 p = 0; L && (u64)p + L <= len; ++p) {
    u32 k = 0;
    while (k < L && src[p + k] == nd[k]) ++k;
    if (k < L) continue;
    if (what == ZK_LOC_FIRST) return p;
    ++count;
  }
  return what == ZK_LOC_FIRST ? ZK_LOC_NONE : count;
}

#if defined(__HIPCC__) || defined(ZKWG_WAVESIM)
#if defined(ZKWG_WAVESIM)
inline int zk_loc_ffs64(u64 v) { return __builtin_ffsll((long long)v); }
inline u32 zk_loc_pop32(u32 v) { return (u32)__builtin_popcount(v); }
#else
__device__ __forceinline__ int zk_loc_ffs64(u64 v) { return __ffsll((unsigned long long)v); }
__device__ __forceinline__ u32 zk_loc_pop32(u32 v) { return (u32)__popcll((unsigned long long)v); }
#endif

struct alignas(16) ZkLoc16 { u32 w[4]; };

// win[0, ZK_LOC_TILE + extra) <- src[base, base + ZK_LOC_TILE + extra), zero where the stream has ended; extra < ZK_LOC_CHUNK.
// Returns the lane's own 16 bytes.  The caller synchronises.
ZK_DEV inline ZkLoc16 zkw_loc_stage(const u8* src, u32 len, u32 base, u32 extra, u8* win) {
  const u32 lane = ZK_LANE();
  const u32 i0 = base + ZK_LOC_LANE_BYTES * lane;            // base < len <= 2^32 - 1 - ZK_LOC_TILE is the caller's (zkw_locate)
  const u32 nvalid = i0 >= len ? 0u : zk_minu(ZK_LOC_LANE_BYTES, len - i0);
  ZkLoc16 v = {{0, 0, 0, 0}};
  if (nvalid == ZK_LOC_LANE_BYTES && (((uintptr_t)(src + i0)) & 15u) == 0) {
    __builtin_memcpy(&v, __builtin_assume_aligned(src + i0, 16), 16);
  } else {
#pragma unroll
    for (u32 k = 0; k < ZK_LOC_LANE_BYTES; ++k)
      if (k < nvalid) v.w[k >> 2] |= (u32)src[i0 + k] << (8 * (k & 3));
  }
  __builtin_memcpy(__builtin_assume_aligned(win + ZK_LOC_LANE_BYTES * lane, 16), &v, 16);
  for (u32 k = lane; k < extra; k += 64) {
    const u64 at = (u64)base + ZK_LOC_TILE + k;
    win[ZK_LOC_TILE + k] = at < len ? src[at] : (u8)0;
  }
  return v;
}

// what = ZK_LOC_FIRST: the first p with src[p, p + L) = nd[0, L) and p + L <= len, or ZK_LOC_NONE.
// what = ZK_LOC_COUNT: the number of such p.
// lds: ZK_LOC_LDS bytes, 16-byte aligned.  L = 0 or L > len: NONE / 0.  len < 2^32 - 2 * ZK_LOC_TILE.  Uniform result; the function
// begins and ends with a barrier, so the caller may use `lds` right before and right after.
ZK_DEV inline u32 zkw_locate(const u8* src, u32 len, const u8* nd, u32 L, u32 what, u8* lds) {
  const u32 lane = ZK_LANE();
  u8* win = lds;
  u8* pat = lds + ZK_LOC_WIN;
  u32 count = 0, found = ZK_LOC_NONE;
  ZK_SYNC();
  if (L != 0 && L <= len) {
    const u32 last = len - L;                                // the last start position at which the needle fits
    const u32 nchunk = (L + ZK_LOC_CHUNK - 1) / ZK_LOC_CHUNK;
    for (u32 t0 = 0; t0 <= last; t0 += ZK_LOC_TILE) {
      u32 cand = 0;
      for (u32 c = 0; c < nchunk; ++c) {
        const u32 off = c * ZK_LOC_CHUNK;
        const u32 cl = zk_minu(ZK_LOC_CHUNK, L - off);
        if (c) ZK_SYNC();                                    // the lanes are done with the chunk before
        const ZkLoc16 own = zkw_loc_stage(src, len, t0 + off, cl - 1, win);
        for (u32 k = lane; k < cl; k += 64) pat[k] = nd[off + k];
        ZK_SYNC();
        if (c == 0) {
          const u32 b0 = pat[0];
#pragma unroll
          for (u32 k = 0; k < ZK_LOC_LANE_BYTES; ++k) {
            const u32 p = t0 + ZK_LOC_LANE_BYTES * lane + k;
            if (p <= last && ((own.w[k >> 2] >> (8 * (k & 3))) & 0xffu) == b0) cand |= 1u << k;
          }
        }
        for (u32 m = cand; m; m &= m - 1) {                  // the surviving candidates, in full out of LDS
          const u32 k = (u32)zk_loc_ffs64(m) - 1u;
          const u8* w = win + ZK_LOC_LANE_BYTES * lane + k;
          u32 j = 0;
          while (j < cl && w[j] == pat[j]) ++j;
          if (j < cl) cand &= ~(1u << k);
        }
        if (c + 1 < nchunk && __ballot(cand != 0) == 0) break;
      }
      if (what == ZK_LOC_FIRST) {
        const u64 hit = __ballot(cand != 0);
        if (hit) {
          const int l = zk_loc_ffs64(hit) - 1;
          const u32 m = (u32)__shfl((int)cand, l);
          found = t0 + ZK_LOC_LANE_BYTES * (u32)l + (u32)zk_loc_ffs64(m) - 1u;
          break;
        }
      } else {
        count += zk_loc_pop32(cand);
      }
      ZK_SYNC();                                             // before the next tile overwrites the window
    }
  }
  if (what == ZK_LOC_COUNT) {
    for (u32 d = 1; d < 64; d <<= 1) count += (u32)__shfl((int)count, (int)(lane ^ d));
    found = count;
  }
  ZK_SYNC();
  return found;
}
#endif  // __HIPCC__ || ZKWG_WAVESIM
