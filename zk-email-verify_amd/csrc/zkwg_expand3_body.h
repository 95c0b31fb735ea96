// The body of zk_expand (zkwg_kernels_expand3.hip: what the kernel does and why it has this shape), in a header so that the
// substring mains and CleanEmailAddress can instantiate it with their own decoder beside the common ones (SUBM = true: zk_expand3_subm,
// zkwg_kernels_substr.hip) without adding a case to the headline kernel's switch.
#pragma once
#include "zkwg_expand_dec.h"
#include "zkwg_kernels.h"

__device__ __forceinline__ uint4 zk_fr_half4(const Fr& m, u32 hf) {
  const u64 x = hf ? m.l[2] : m.l[0], y = hf ? m.l[3] : m.l[1];   // (selects: a runtime index would put the element in scratch memory)
  return make_uint4((u32)x, (u32)(x >> 32), (u32)y, (u32)(y >> 32));
}
// Montgomery form of the rare values no table holds.  Out of line, with the reference sources passed BY VALUE: a reference
// to the ZkRefSrc of the caller would force that struct into scratch memory -- 32 bytes per lane stored on every email
// iteration whether or not the call happens (PMC: 1.39 x the algorithmic bytes written by the Montgomery kernels, r03_pmc_abc)
__device__ __noinline__ uint4 zk_mont_slow(u32 code, u32 hf, const uint4* frv, const uint4* invtab, const u8* rec, const u32* small) {
  if (!(code >> 31)) return zk_fr_half4(fr_to_mont(Fr{{(u64)code, 0, 0, 0}}), hf);   // an immediate >= 2^16
  // RAW / NEG / I64: standard-form value first (zk_ref_half), then one product
  ZkRefSrc R;
  R.frv = frv; R.invtab = invtab; R.rec = rec; R.small = small;
  const uint4 a = zk_ref_half(code, 0u, R), b = zk_ref_half(code, 1u, R);
  const Fr x{{(u64)a.x | ((u64)a.y << 32), (u64)a.z | ((u64)a.w << 32), (u64)b.x | ((u64)b.y << 32), (u64)b.z | ((u64)b.w << 32)}};
  return zk_fr_half4(fr_to_mont(x), hf);
}
// the 16-byte half `hf` of the slot whose code is `code`
template <bool MONT>
__device__ __forceinline__ uint4 zk_slot_half(u32 code, u32 hf, const ZkX3& A, const ZkRefSrc& R) {
  if constexpr (!MONT) {
    return (code >> 31) ? zk_ref_half(code, hf, R) : zk_small(hf ? 0u : code);
  } else {
    if (!(code >> 31)) {
      if (code <= 1u) return code ? zk_fr_half4(fr_R(), hf) : zk_zero4();   // R = 2^256 mod r
      if (code < 65536u) return ((const uint4*)A.rtab)[2u * code + hf];
      return zk_mont_slow(code, hf, R.frv, R.invtab, R.rec, R.small);
    }
    const u32 t = ZK_REF_TYPE(code), p = ZK_REF_PAYLOAD(code);
    if (t == 0u) return R.frv[2u * p + hf];                                       // Montgomery copy of the image's fr
    if (t == 1u) return R.invtab[2u * p + hf];                                    // Montgomery inverse table
    if (t == 2u) return R.frv[2u * (A.img_fr + ((p - A.limb_off) >> 4)) + hf];    // converted limb
    // integers of the image (RAW / NEG / I64: results of integer rows, negative small values): |v| < 2^16 -> the table,
    // r - table[|v|] for a negative one (the A.w / B.w / C.w of bit constraints are full of -1 and -2)
    {
      long long v;
      if (t == 6u) v = -(long long)p;
      else {
        const u32 w = R.small[p];
        if (t == 3u) v = (long long)w; else if (t == 4u) v = (long long)((int)(w << 1) >> 1); else v = (long long)((u64)w | ((u64)R.small[p + 1] << 32));
      }
      const u64 m = v < 0 ? (u64)(-v) : (u64)v;
      if (m < 65536u) {
        const uint4* tb = (const uint4*)A.rtab + 2u * (u32)m;
        if (v >= 0) return tb[hf];
        // r - x, x = m R mod r, 0 < x < r: low half with its borrow, high half minus that borrow
        const uint4 xl = tb[0];
        const u64 x0 = (u64)xl.x | ((u64)xl.y << 32), x1 = (u64)xl.z | ((u64)xl.w << 32);
        const u64 r0 = ZK_P0, r1 = ZK_P1, r2 = ZK_P2, r3 = ZK_P3;
        const u64 d0 = r0 - x0, b0 = r0 < x0 ? 1ull : 0ull;
        const u64 d1 = r1 - x1 - b0, b1 = (r1 < x1 || (r1 == x1 && b0)) ? 1ull : 0ull;
        if (!hf) return make_uint4((u32)d0, (u32)(d0 >> 32), (u32)d1, (u32)(d1 >> 32));
        const uint4 xh = tb[1];
        const u64 x2 = (u64)xh.x | ((u64)xh.y << 32), x3 = (u64)xh.z | ((u64)xh.w << 32);
        const u64 d2 = r2 - x2 - b1, b2 = (r2 < x2 || (r2 == x2 && b1)) ? 1ull : 0ull;
        const u64 d3 = r3 - x3 - b2;
        return make_uint4((u32)d2, (u32)(d2 >> 32), (u32)d3, (u32)(d3 >> 32));
      }
    }
    return zk_mont_slow(code, hf, R.frv, R.invtab, R.rec, R.small);
  }
}

__device__ __forceinline__ u32 zk_x3_unit(u32 xcd_remap) {
  // workgroups are dealt to the 8 XCDs round-robin (blockIdx % 8).  1: each XCD streams through one contiguous eighth of the
  // whole launch; G > 1: through a contiguous run of G pieces inside each group of 8 G pieces (the eight streams then stay
  // within 8 G pieces of each other); 0: plain order
  u32 blk = blockIdx.x;
  if (xcd_remap == 1u) {
    const u32 per = gridDim.x >> 3;
    if (blk < per * 8u) blk = (blk & 7u) * per + (blk >> 3);
  } else if (xcd_remap > 1u) {
    const u32 G = xcd_remap, grp = blk / (8u * G), r = blk - grp * 8u * G;
    if ((grp + 1u) * 8u * G <= gridDim.x) blk = grp * 8u * G + (r & 7u) * G + (r >> 3);
  }
  return blk;
}
__device__ __forceinline__ ZkCtx zk_x3_ctx(const ZkX3& A, u32 e) {
  ZkCtx cx;
  cx.rec = A.in + (u64)e * A.in_stride;
  cx.bits = A.bits + (u64)e * A.img_bits;
  cx.small = A.small + (u64)e * A.img_small;
  cx.half = (int)A.inv_half;
  cx.m_dfa_cm = A.m_dfa_cm; cx.m_dfa_pm = A.m_dfa_pm; cx.m_dfa_st = A.m_dfa_st;
  cx.nd = A.netd;
  return cx;
}
// store side: wavefront w owns the 64 K consecutive slots [64 K w, 64 K (w + 1)) of the piece (K = slots per lane);
// lane l holds the codes of slots 64 k + l (k < K).  Chunk 64 j + l (j < 2 K) of the wavefront's 2 K KiB belongs to
// slot 32 j + (l >> 1): register j / 2, fetched from lane 32 (j & 1) + (l >> 1) with one wavefront shuffle.
template <bool MONT, int K>
__device__ __forceinline__ void zk_x3_store(const ZkX3& A, const ZkCtx& cx, u32 e, u32 el, u64 slot0, u32 nsl, const u32 (&code)[K]) {
  const u32 lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, hf = lane & 1u;
  ZkRefSrc R;
  R.frv = MONT ? (const uint4*)(A.frm + (u64)e * (A.img_fr + ZK_MONT_LIMBS)) : (const uint4*)(A.frv + (u64)e * A.img_fr);
  R.invtab = (const uint4*)(MONT ? A.invtab_m : A.invtab);
  R.rec = cx.rec; R.small = cx.small;
  const u32 w0 = 64u * K * wv;                                        // first slot of this wavefront inside the piece
  uint4* __restrict__ dst = A.wit + (u64)el * A.wit_stride16 + (slot0 + w0) * 2u;
  const u32 left = nsl > w0 ? (nsl - w0) * 2u : 0u;                   // chunks of this wavefront inside the witness
  uint4 v[2 * K];
#pragma unroll
  for (int j = 0; j < 2 * K; ++j) {
    const u32 c = __shfl(code[j >> 1], 32u * (j & 1) + (lane >> 1));
    v[j] = zk_slot_half<MONT>(c, hf, A, R);
  }
#pragma unroll
  for (int j = 0; j < 2 * K; ++j)
    if (64u * j + lane < left) dst[64u * j + lane] = v[j];
}

template <bool MONT, int K, bool SUBM = false, bool CEA = false>
__device__ __forceinline__ void zk_expand3_body(const ZkX3& A) {
  constexpr u32 SLOTS = 256u * K;
  const u32 unit = zk_x3_unit(A.xcd_remap);
  const u32 p = unit % A.nportions, el = unit / A.nportions;   // piece p of email el (launch-local)
  const u32 e = el + A.e_first;
  const u64 slot0 = (u64)p * SLOTS;
  const u32 nsl = (u32)min((u64)SLOTS, A.W - slot0);
  const u32 lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const ZkCtx cx = zk_x3_ctx(A, e);
  const ZkPortionEntry en = A.ent[p];
  u32 code[K];
  if (en.type < ZSEG_NTYPES) {
    // the whole piece lies inside one segment: its parameters came with the entry
    ZkSeg sg;
    sg.slot = 0; sg.nslots = 0; sg.type = en.type; sg.src = en.src; sg.a = en.a; sg.b = en.b; sg.c = en.c; sg.r0 = 0; sg.pad = en.magic;
    zk_decode_k<K, SUBM, CEA>(sg, en.r_start, 64u * K * wv + lane, nsl, cx, code);
  } else {
    // the piece straddles segments: find each slot's
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const u32 i = 64u * K * wv + 64u * k + lane;
      code[k] = 0u;
      if (i < nsl) {
        const u64 slot = slot0 + i;
        for (u32 si = en.first_seg; si < A.nsegs; ++si) {
          const ZkSeg sg = A.segs[si];
          if (sg.slot > slot) break;
          if (slot < sg.slot + sg.nslots) { code[k] = zk_decode_any<SUBM, CEA>(sg, (u32)(slot - sg.slot) + sg.r0, cx); break; }
        }
      }
    }
  }
  zk_x3_store<MONT, K>(A, cx, e, el, slot0, nsl, code);
}
