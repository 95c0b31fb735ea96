// The transforms of zkwg_kernels_ntt.hip: butterflies, the per-phase bodies of the column, row and join kernels, the pass schedule and
// the plan's tables, shared with the host mirror of the CPU tests (tests/native/hosttest.cpp runs exactly these functions, thread by
// thread, phase by phase, in the launch order of zk_ntt_launch).  A phase is what one thread does between two barriers: the kernels
// call it with (threadIdx.x, 256) and __syncthreads() between phases.  The value bounds of the lazy limb form (notation of
// zkwg_fr29.h: [U, V] = limbs 0 .. 7 < U 2^29, value < V r) are the ones the checked host build (ZKWG_FR29_CHECK) confirms.
#pragma once
#include "zkwg_fr29.h"

#define ZK_NTT_TILE 1024u   // elements per workgroup: a column pass takes 1024 / 2^g neighbouring columns (>= 128 contiguous bytes per row access)
#define ZK_NTT_GMAX 7u      // butterfly stages per pass (the value bounds below)

// four words of LDS: HIP's uint4 on the device, a plain struct in the host build
#if defined(__HIPCC__)
typedef uint4 ZkU4;
ZK_HD ZkU4 zk_u4(u32 a, u32 b, u32 c, u32 d) { return make_uint4(a, b, c, d); }
#else
struct ZkU4 { u32 x, y, z, w; };
inline ZkU4 zk_u4(u32 a, u32 b, u32 c, u32 d) { return ZkU4{a, b, c, d}; }
#endif

ZK_HD u32 zk_bitrev(u32 x, u32 bits) {
#if defined(__HIP_DEVICE_COMPILE__)
  return bits ? (__brev(x) >> (32u - bits)) : 0u;
#else
  u32 r = 0;
  for (u32 i = 0; i < bits; ++i) r |= ((x >> i) & 1u) << (bits - 1u - i);
  return r;
#endif
}
// w^e for the transform's direction: tw[k] = w^k (2^261 form), k < n; the inverse direction reads w^(n - e)
ZK_HD Fr29 zk_ntt_tw(const Fr* __restrict__ tw, u64 n, u64 e, bool inv) {
  e &= n - 1u;
  return fr29_from_fr(tw[inv ? ((n - e) & (n - 1u)) : e]);
}
ZK_HD Fr29 zk_l29(ZkU4 a, ZkU4 b, u32 t) { return Fr29{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, t}}; }

// LDS layout: limbs 0-3, limbs 4-7 and the top limb of an element live in separate arrays (lo[i], hi[i], top[i]): a wavefront's
// ds_read_b128 of consecutive elements covers each bank once
struct ZkLds29 {
  ZkU4* lo; ZkU4* hi; u32* top;
  ZK_HD Fr29 get(u32 i) const { return zk_l29(lo[i], hi[i], top[i]); }
  ZK_HD void put(u32 i, const Fr29& v) const {
    lo[i] = zk_u4(v.l[0], v.l[1], v.l[2], v.l[3]); hi[i] = zk_u4(v.l[4], v.l[5], v.l[6], v.l[7]); top[i] = v.l[8];
  }
};
ZK_HD ZkLds29 zk_lds29(ZkU4* base, u32 count) { return ZkLds29{base, base + count, (u32*)(base + 2u * count)}; }
// bytes of LDS for `count` elements (16-byte granules)
ZK_HD size_t zk_lds29_bytes(u32 count) { return ((size_t)count * 36 + 15) & ~(size_t)15; }

// a polynomial in HBM: canonical words (the callers' arrays: A.w | B.w | C.w, stand-alone transforms) or the planar limb form of the work buffer
struct ZkNttBuf {
  const void* base;
  u64 es, ps, valid;      // canonical: polynomial q at base + (q / 3) es + (q % 3) ps (Fr units), `valid` elements (zero beyond)
  u32 lazy;               // 1: planar limb form, polynomial q at base + q * 36 n bytes
};
ZK_HD Fr29 zk_ntt_load(const ZkNttBuf& b, u64 n, u64 q, u64 idx) {
  if (b.lazy) {
    const u8* p = (const u8*)b.base + q * 36u * n;
    return zk_l29(((const ZkU4*)p)[idx], ((const ZkU4*)(p + 16u * n))[idx], ((const u32*)(p + 32u * n))[idx]);
  }
  const Fr* s = (const Fr*)b.base + (q / 3u) * b.es + (q % 3u) * b.ps;
  return idx < b.valid ? fr29_from_fr(s[idx]) : fr29_zero();
}
// V: bound of the value in units of r when the destination is canonical
template <int V>
ZK_HD void zk_ntt_store(const ZkNttBuf& b, u64 n, u64 q, u64 idx, const Fr29& v) {
  if (b.lazy) {
    u8* p = (u8*)b.base + q * 36u * n;
    ((ZkU4*)p)[idx] = zk_u4(v.l[0], v.l[1], v.l[2], v.l[3]);
    ((ZkU4*)(p + 16u * n))[idx] = zk_u4(v.l[4], v.l[5], v.l[6], v.l[7]);
    ((u32*)(p + 32u * n))[idx] = v.l[8];
  } else {
    ((Fr*)b.base + (q / 3u) * b.es + (q % 3u) * b.ps)[idx] = fr29_to_fr_v<V>(v);
  }
}

// ---- butterflies in limb form.  I: the inputs' value bound in units of r; every input has limbs 0 .. 7 < 2^29 (DIF) -------------------
// DIF radix-4 group (two stages): 4 products, 2 carry normalisations; outputs < 4 I r with normalised limbs
template <int I>
ZK_HD void zk_dif4(const Fr29& x0, const Fr29& x1, const Fr29& x2, const Fr29& x3, const Fr29& wa, const Fr29& wb, const Fr29& w2,
                   Fr29& y0, Fr29& y1, Fr29& y2, Fr29& y3) {
  const Fr29 a0 = fr29_add(x0, x2), a1 = fr29_add(x1, x3);                                  // [2, 2 I]
  const Fr29 a2 = fr29_mul(fr29_sub<I + 1, 1>(x0, x2), wa);                                 // operand [3, 2 I + 1] -> [1, (2 I + 1) / 169 + 1 <= 5]
  const Fr29 a3 = fr29_mul(fr29_sub<I + 1, 1>(x1, x3), wb);
  y0 = fr29_norm(fr29_add(a0, a1));                                                         // [1, 4 I]
  y1 = fr29_mul(fr29_sub<2 * I + 1, 2>(a0, a1), w2);                                        // operand [5, 4 I + 1] -> [1, (4 I + 1) / 169 + 1]
  y2 = fr29_norm(fr29_add(a2, a3));                                                         // [1, 10]
  y3 = fr29_mul(fr29_sub<6, 1>(a2, a3), w2);                                                // [1, 2]
}
template <int I>
ZK_HD void zk_dif2(const Fr29& a, const Fr29& b, const Fr29& w, Fr29& y0, Fr29& y1) {
  y0 = fr29_norm(fr29_add(a, b));                                                           // [1, 2 I]
  y1 = fr29_mul(fr29_sub<I + 1, 1>(a, b), w);                                               // [1, (2 I + 1) / 169 + 1]
}
// DIT radix-4 group: x0, x2 normalised by the caller, x1, x3 limbs < 6 2^29; every product is below 2 r, an output gains at most 6 r
ZK_HD void zk_dit4(const Fr29& x0, const Fr29& x1, const Fr29& x2, const Fr29& x3, const Fr29& w1, const Fr29& wp, const Fr29& wq,
                   Fr29& y0, Fr29& y1, Fr29& y2, Fr29& y3) {
  const Fr29 t1 = fr29_mul(x1, w1), t3 = fr29_mul(x3, w1);                                  // [1, 2]
  const Fr29 a0 = fr29_add(x0, t1), a1 = fr29_sub<3, 1>(x0, t1);                            // [2, V + 2], [3, V + 3]
  const Fr29 u2 = fr29_mul(fr29_add(x2, t3), wp), u3 = fr29_mul(fr29_sub<3, 1>(x2, t3), wq);    // operands [2], [3] -> [1, 2]
  y0 = fr29_add(a0, u2); y2 = fr29_sub<3, 1>(a0, u2);                                       // [3, V + 4], [4, V + 5]
  y1 = fr29_add(a1, u3); y3 = fr29_sub<3, 1>(a1, u3);                                       // [4, V + 5], [5, V + 6]
}

// The butterfly stages of 2^g-point sub-transforms over `nel` elements per column, C columns interleaved (element i of
// column cc at i * C + cc), two stages per pass through LDS where possible: zk_ntt_stage_pair for st = 0, 2, .. while st + 1 < g,
// then zk_ntt_stage_single at st = g - 1 when g is odd, a barrier after each.
template <bool DIT>
ZK_HD void zk_ntt_stage_pair(const ZkLds29& y, const ZkLds29& twl, u32 G, u32 st, u32 nel, u32 C, u32 thread, u32 threads) {
  const u32 h = DIT ? (1u << st) : (G >> (st + 2u));
  for (u32 b = thread; b < (nel / 4u) * C; b += threads) {
    const u32 cc = b % C, q = b / C;
    const u32 p = q % h, i0 = (q / h) * 4u * h + p;
    const u32 e0 = i0 * C + cc, e1 = (i0 + h) * C + cc, e2 = (i0 + 2u * h) * C + cc, e3 = (i0 + 3u * h) * C + cc;
    Fr29 y0, y1, y2, y3;
    if (DIT) {
      zk_dit4(fr29_norm(y.get(e0)), y.get(e1), fr29_norm(y.get(e2)), y.get(e3), twl.get(p * (G / (2u * h))), twl.get(p * (G / (4u * h))),
              twl.get((p + h) * (G / (4u * h))), y0, y1, y2, y3);
      y.put(e0, y0); y.put(e2, y2); y.put(e1, y1); y.put(e3, y3);
    } else {
      const Fr29 x0 = y.get(e0), x1 = y.get(e1), x2 = y.get(e2), x3 = y.get(e3);
      const Fr29 wa = twl.get(p << st), wb = twl.get((p + h) << st), w2 = twl.get(p << (st + 1u));
      // (the inputs' bound: 5 r at the first stage pair of a pass, 4 x more at each following one)
      if (st == 0) zk_dif4<5>(x0, x1, x2, x3, wa, wb, w2, y0, y1, y2, y3);
      else if (st == 2) zk_dif4<20>(x0, x1, x2, x3, wa, wb, w2, y0, y1, y2, y3);
      else zk_dif4<80>(x0, x1, x2, x3, wa, wb, w2, y0, y1, y2, y3);
      y.put(e0, y0); y.put(e1, y1); y.put(e2, y2); y.put(e3, y3);
    }
  }
}
template <bool DIT>
ZK_HD void zk_ntt_stage_single(const ZkLds29& y, const ZkLds29& twl, u32 G, u32 st, u32 nel, u32 C, u32 thread, u32 threads) {
  const u32 half = DIT ? (1u << st) : (G >> (st + 1u));
  for (u32 b = thread; b < (nel / 2u) * C; b += threads) {
    const u32 cc = b % C, pi = b / C;
    const u32 i = (pi / half) * 2u * half + (pi % half), j = i + half;
    const u32 k = DIT ? (pi % half) * (G / (2u * half)) : ((pi % half) << st);
    if (DIT) {
      const Fr29 a = fr29_norm(y.get(i * C + cc)), tt = fr29_mul(y.get(j * C + cc), twl.get(k));
      y.put(i * C + cc, fr29_add(a, tt));
      y.put(j * C + cc, fr29_sub<3, 1>(a, tt));
    } else {
      const Fr29 a = y.get(i * C + cc), bb = y.get(j * C + cc), w = twl.get(k);
      Fr29 y0, y1;
      if (st == 0) zk_dif2<5>(a, bb, w, y0, y1);
      else if (st == 2) zk_dif2<20>(a, bb, w, y0, y1);
      else if (st == 4) zk_dif2<80>(a, bb, w, y0, y1);
      else zk_dif2<320>(a, bb, w, y0, y1);
      y.put(i * C + cc, y0);
      y.put(j * C + cc, y1);
    }
  }
}

// One column pass, one workgroup.  Block size N = 2^lb (the sub-problem of this recursion level), sub-transform size G = 2^g over the
// rows r of a column: element index = block * N + r * (N >> g) + c.  DIF: sub-transform, then y *= w_N^(c * bitrev_g(r)).
// DIT: y *= w_N^(c * bitrev_g(r)) first, then the sub-transform.  Polynomial q = blockIdx.y.  Phases: load | stages | store.
struct ZkNttColWg {
  ZkLds29 y, twl;         // [G][C] elements; w_G^k, k < G / 2 (direction applied)
  u64 n, base, q;
  u32 L, lb, g, G, C, c0;
  bool inv;
};
ZK_HD ZkNttColWg zk_ntt_col_wg(ZkU4* lds4, u32 L, u32 lb, u32 g, u32 inv, u32 bx, u32 by) {
  ZkNttColWg w;
  w.n = 1ull << L;
  const u32 TILE = w.n < ZK_NTT_TILE ? (u32)w.n : ZK_NTT_TILE;      // (domains below 1,024 points: one workgroup, fewer columns)
  w.G = 1u << g; w.C = TILE >> g;
  w.y = zk_lds29(lds4, w.G * w.C);
  w.twl = zk_lds29(lds4 + zk_lds29_bytes(w.G * w.C) / 16u, w.G / 2u);
  const u32 cols_per_block = 1u << (lb - g);
  const u64 cid0 = (u64)bx * w.C;
  const u64 block = cid0 >> (lb - g);
  w.c0 = (u32)(cid0 & (cols_per_block - 1u));
  w.q = by;
  w.base = block << lb;
  w.L = L; w.lb = lb; w.g = g; w.inv = inv != 0;
  return w;
}
template <bool DIT>
ZK_HD void zk_ntt_col_load(const ZkNttColWg& w, const ZkNttBuf& src, const Fr* __restrict__ tw, u32 thread, u32 threads) {
  for (u32 k = thread; k < w.G / 2u; k += threads) w.twl.put(k, zk_ntt_tw(tw, w.n, (u64)k << (w.L - w.g), w.inv));
  for (u32 t = thread; t < w.G * w.C; t += threads) {
    const u32 r = t / w.C, cc = t % w.C;
    const u64 idx = w.base + ((u64)r << (w.lb - w.g)) + w.c0 + cc;
    Fr29 v = zk_ntt_load(src, w.n, w.q, idx);
    if (DIT) v = fr29_mul(v, zk_ntt_tw(tw, w.n, ((u64)(w.c0 + cc) * zk_bitrev(r, w.g)) << (w.L - w.lb), w.inv));     // limbs < 6 2^29, value < 30 r -> [1, 2]
    w.y.put(t, v);
  }
}
template <bool DIT>
ZK_HD void zk_ntt_col_store(const ZkNttColWg& w, const ZkNttBuf& dst, const Fr* __restrict__ tw, u32 thread, u32 threads) {
  for (u32 t = thread; t < w.G * w.C; t += threads) {
    const u32 r = t / w.C, cc = t % w.C;
    const u64 idx = w.base + ((u64)r << (w.lb - w.g)) + w.c0 + cc;
    Fr29 v = w.y.get(t);
    if (!DIT) v = fr29_mul(v, zk_ntt_tw(tw, w.n, ((u64)(w.c0 + cc) * zk_bitrev(r, w.g)) << (w.L - w.lb), w.inv));    // < 640 r -> [1, 5]
    zk_ntt_store<32>(dst, w.n, w.q, idx, v);                                                                          // (DIT: [1, 2] + 21 r)
  }
}

// The row pass, one workgroup: contiguous blocks of G = 2^g elements, 1,024 elements per workgroup.  DIF (inverse direction of the
// pipeline): optional multiplication by scale[position] on the way out (coset shift and 1 / n).  Phases: load | stages | store.
struct ZkNttRowWg {
  ZkLds29 y, twl;         // [TILE] elements; w_G^k, k < G / 2
  u64 n, base, q;
  u32 L, g, G, TILE;
  bool inv;
};
ZK_HD ZkNttRowWg zk_ntt_row_wg(ZkU4* lds4, u32 L, u32 g, u32 inv, u32 bx, u32 by) {
  ZkNttRowWg w;
  w.n = 1ull << L;
  w.G = 1u << g;
  w.TILE = w.n < 1024u ? (u32)w.n : 1024u;
  w.y = zk_lds29(lds4, w.TILE);
  w.twl = zk_lds29(lds4 + zk_lds29_bytes(w.TILE) / 16u, w.G / 2u);
  w.q = by;
  w.base = (u64)bx * w.TILE;
  w.L = L; w.g = g; w.inv = inv != 0;
  return w;
}
ZK_HD void zk_ntt_row_load(const ZkNttRowWg& w, const ZkNttBuf& src, const Fr* __restrict__ tw, u32 thread, u32 threads) {
  for (u32 k = thread; k < w.G / 2u; k += threads) w.twl.put(k, zk_ntt_tw(tw, w.n, (u64)k << (w.L - w.g), w.inv));
  for (u32 t = thread; t < w.TILE; t += threads) w.y.put(t, zk_ntt_load(src, w.n, w.q, w.base + t));
}
ZK_HD void zk_ntt_row_store(const ZkNttRowWg& w, const ZkNttBuf& dst, const Fr* __restrict__ scale, const Fr& uni, u32 use_uni, u32 thread, u32 threads) {
  for (u32 t = thread; t < w.TILE; t += threads) {
    Fr29 v = w.y.get(t);
    if (scale) v = fr29_mul(v, fr29_from_fr(scale[w.base + t]));
    else if (use_uni) v = fr29_mul(v, fr29_from_fr(uni));     // (stand-alone inverse transform: 1 / n)
    zk_ntt_store<32>(dst, w.n, w.q, w.base + t, v);           // (DIT without a product: < 5 + 21 r)
  }
}

// out[k] = a[k] b[k] - c[k]  (joinABC of groth16_prove.js) for limb-form a, b, c of 2^256-form values below 30 r; canonical words,
// 2^256 form.  mul(a, b) carries 2^256 2^256 / 2^261: the constant 2^266 restores it.  ab is below 1.04 r, NOT below r: ab - c + 31 r
// reaches [32 r, 33 r) when ab >= r and c < ab - r (c = 0 is inside the contract), so the conversion takes values below 33 r.
ZK_HD Fr zk_ntt_join_value(const Fr29& a_in, const Fr29& b_in, const Fr29& c_in) {
  const Fr29 a = fr29_norm(a_in), b = fr29_norm(b_in), c = fr29_norm(c_in);
  const Fr29 k266 = Fr29{{0x0fffead7u, 0x1d5444f4u, 0x04438aa5u, 0x03b4d096u, 0x134c84dau, 0x0e92d304u, 0x14cb95b3u, 0x041b9d3du, 0x00058003u}};     // 2^266 mod r
  const Fr29 ab = fr29_mul(fr29_mul(a, b), k266);             // [1, 30 30 / 169 + 1 = 7] -> [1, 7 / 169 + 1 < 1.05]
  return fr29_to_fr_v<33>(fr29_sub<31, 1>(ab, c));
}
// polynomials of email e at work + (3 e + {0, 1, 2}) * 36 n bytes (limb form)
ZK_HD void zk_ntt_join_thread(const ZkNttBuf& work, Fr* __restrict__ out, u64 n, u64 out_es, u64 e, u64 i) {
  out[e * out_es + i] = zk_ntt_join_value(zk_ntt_load(work, n, 3u * e, i), zk_ntt_load(work, n, 3u * e + 1u, i), zk_ntt_load(work, n, 3u * e + 2u, i));
}
// in-place bit-reversal permutation of element i of polynomial q (stand-alone transforms only: the pipeline needs none)
ZK_HD void zk_ntt_bitrev_thread(Fr* __restrict__ data, u32 L, u64 q, u64 i) {
  const u64 n = 1ull << L;
  const u64 j = (u64)zk_bitrev((u32)i, L);
  if (i < j) {
    Fr* p = data + q * n;
    const Fr a = p[i], b = p[j];
    p[i] = b; p[j] = a;
  }
}

// ---- the pass schedule of one transform: L stages in ceil(L / GMAX) passes of nearly equal size; the row pass takes the last share
// (and at most log2 of its tile).  Column pass i (i < ng) runs gs[i] stages on blocks of 2^lb[i] elements: DIF runs the column passes
// in order, then the row pass; DIT the row pass, then the column passes in reverse order.
struct ZkNttSched {
  u32 np, ng, g_row, tile;
  u32 gs[8], lb[8];
};
ZK_HD ZkNttSched zk_ntt_sched(u32 L) {
  ZkNttSched s;
  const u64 n = 1ull << L;
  s.np = (L + ZK_NTT_GMAX - 1u) / ZK_NTT_GMAX;
  u32 lb = L;
  for (u32 i = 0; i < s.np; ++i) { s.gs[i] = L / s.np + (i < L % s.np ? 1u : 0u); s.lb[i] = lb; lb -= s.gs[i]; }
  s.g_row = s.gs[s.np - 1u];
  s.ng = s.np - 1u;
  s.tile = n < 1024u ? (u32)n : 1024u;
  return s;
}
// bytes of LDS of a pass of g stages
ZK_HD size_t zk_ntt_lds_bytes(u32 tile, u32 g) { return zk_lds29_bytes(tile) + zk_lds29_bytes((1u << g) / 2u); }

#include <vector>
// ---- the plan's tables (host).  ffjavascript F1Field: s = 28, t = (r - 1) >> 28, w[28] = 5^t, w[i] = w[i+1]^2, shift = 5^2.  The
// tables are in 2^261-Montgomery form (canonical words): tw[k] = w^k, k < n; sc[p] = inc^bitrev(p) / n; ninv = 1 / n.  False when
// w is not a primitive n-th root.
static inline Fr zk_ntt_pow_m(Fr base_m, const u64 e[4]) {   // Montgomery in / out
  Fr acc = fr_R();
  for (int i = 255; i >= 0; --i) {
    acc = fr_mont_mul(acc, acc);
    if ((e[i >> 6] >> (i & 63)) & 1) acc = fr_mont_mul(acc, base_m);
  }
  return acc;
}
static inline bool zk_ntt_tables(u32 L, std::vector<Fr>& tw, std::vector<Fr>& sc, Fr& ninv_m) {
  const u64 n = 1ull << L;
  const u64 r1[4] = {ZK_P0 - 1, ZK_P1, ZK_P2, ZK_P3};
  u64 t[4];
  for (int i = 0; i < 4; ++i) t[i] = (r1[i] >> 28) | (i < 3 ? r1[i + 1] << 36 : 0);
  const Fr five_m = fr_to_mont(fr_from_u64(5));
  Fr w = zk_ntt_pow_m(five_m, t);                            // w[28]
  Fr wL1 = w;                                                // w[L + 1] (L < 28)
  for (u32 i = 28; i > L; --i) { if (i == L + 1) wL1 = w; w = fr_mont_mul(w, w); }
  const Fr inc = L == 28 ? fr_to_mont(fr_from_u64(25)) : wL1;
  tw.assign(n, Fr{}); sc.assign(n, Fr{});
  Fr acc = fr_R();
  for (u64 k = 0; k < n; ++k) { tw[k] = acc; acc = fr_mont_mul(acc, w); }
  if (!fr_eq(acc, fr_R()) || !fr_eq(tw[n / 2], fr_neg(fr_R()))) return false;   // w^n = 1, w^(n/2) = -1
  const u64 e2[4] = {ZK_P0 - 2, ZK_P1, ZK_P2, ZK_P3};
  ninv_m = zk_ntt_pow_m(fr_to_mont(fr_from_u64(n)), e2);
  acc = ninv_m;
  for (u64 i = 0; i < n; ++i) { sc[zk_bitrev((u32)i, L)] = acc; acc = fr_mont_mul(acc, inc); }
  // 2^256 form -> 2^261 form: times 32
  const Fr m32 = fr_to_mont(fr_from_u64(32));
  for (u64 k = 0; k < n; ++k) { tw[k] = fr_mont_mul(tw[k], m32); sc[k] = fr_mont_mul(sc[k], m32); }
  ninv_m = fr_mont_mul(ninv_m, m32);
  return true;
}
