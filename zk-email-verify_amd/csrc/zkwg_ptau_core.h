// Preparing a powers-of-tau file for phase 2 (snarkjs `powersoftau prepare phase2`, src/powersoftau_prepare_phase2.js [EXT]; the reference's
// workflow names the prepared file: docs/zk-email-docs/UsageGuide/README.md:145-180): the Lagrange sections 12 - 15 that zk_ptau_parse
// (zkwg_setup_core.h) reads are INVERSE DISCRETE FOURIER TRANSFORMS OVER GROUP ELEMENTS of the monomial sections 2 - 5.
// One header for the library (csrc/zkwg_ptau_api.hip, csrc/zkwg_kernels_ptau.hip) and for the host build of the CPU tests
// (tests/native/ptautest.cpp, ZKWG_FQ29_CHECK counting every violated limb-form bound).
//
//   zk_ptau_recode        a twiddle (< r) -> its non-adjacent form, two bit strings of 255 positions (a 64-byte table entry)
//   zk_ptau_table         the recoded powers w^e, e < N / 2, of the 2^L-th root of unity (or of its inverse) and the operation counts per stage
//   zk_ptau_mul           t = w v for a table-form affine v: what a lane (G2: a lane pair) of zk_ptau_stage walks
//   zk_ptau_butterfly     (u, v) -> (u + w v, u - w v)
//   zk_ptau_ntt_host      the host mirror of one transform: the launch series of zkwg_group_ntt_device over the same per-point functions
//   zk_ptau_frame / zk_ptau_prepare_apply / zk_ptau_prepare_host   the file operation
//
// THE TRANSFORM.  out[j] = sum_k w^(+-jk) in[k] over 2^L affine points, natural order in and out, w = Fr.w[L] of ffjavascript (nqr = 5:
// oracle/pyref/ntt.root, zk_ntt_tables); the inverse also multiplies by 2^-L.  Radix 2, decimation in time: the points are permuted to
// bit-reversed order, then stage s = 0 .. L - 1 (half = 2^s) takes (u, v) = (a[g 2 half + j], a[g 2 half + j + half]), j < half,
// g < 2^(L - 1 - s), to (u + w_j v, u - w_j v) with w_j = w^(j 2^(L - 1 - s)): the 2^(L - 1 - s) groups of a stage SHARE w_j.
//
// LANES.  Butterfly t of a stage is (g, j) = (t mod groups, t div groups): neighbouring lanes are neighbouring GROUPS.  While a stage
// has at least 64 groups (G2: 32 lane pairs) -- stages s <= L - 7 -- a wavefront holds one twiddle: zk_ptau_stage<C, true> fetches the
// digit words through readfirstlane, so the walk is the lockstep walk of zk_phase2_scale (scalar branches; one ec29_dbl per position,
// one ec29_add_mixed of +v or -v per non-zero digit).  The last 6 (G2: 5) stages, and every stage of a small transform, run
// zk_ptau_stage<C, false>: the same body with the digit words per lane and the addition PREDICATED on the lane's digit.  A wavefront there
// holds 64 / groups twiddles and executes the addition at the positions where ANY of them has a digit: 1 - (2/3)^k of the positions for
// k twiddles (k = 2: 0.56, 4: 0.80, 8: 0.96, >= 16: all).  Twiddle 1 (j = 0; all of stage 0) takes no walk; -1 = w^(N / 2) is never a
// stage's twiddle (j < half).
//
// WHY PREDICATED DIGITS AND NOT A WINDOW (field products per multiplication, G1: ec29_dbl 9, ec29_add_mixed 11, ec29_add 15):
//   shared twiddle, non-adjacent form      254 x 9 + 85 x 11            = 3,221
//   predicated digits, 64 twiddles a wave  254 x 9 + 254 x 11           = 5,080   (1.58 x)
//   fixed window of 4, signed, odd multiples P, 3P, 5P, 7P of the lane in LDS:  254 x 9 + 64 x 15 + (9 + 3 x 15) = 3,300   (1.02 x)
// but the window's table is 4 x 144 bytes a lane = 36 KB a wavefront (G2: 72 KB): with 160 KB of LDS a compute unit that is ONE wavefront
// per SIMD, and three per SIMD (what zk_phase2_scale<G1> runs at, and the chain of dependent products needs to hide its latency) leave
// 213 bytes a lane -- not two entries.  So the distinct-scalar share is predicated digits; it is 6 of the L - 1 multiplying stages.
// (Where EVERY multiplication has its own scalar -- a contribution to the file -- the table goes to device memory instead: zkwg_ptau_key_core.h.)
// A row/column split would leave ONE distinct pass instead of six (and fold 2^-L into it): predicted (L - 0.8) / (L + 3.5) of this
// schedule's products at large L (0.82 at L = 21).  Not built.
//
// NORMALISATION.  2^-L is applied once per level by the shared-scalar kernel of phase 2 itself (zk_phase2_scale) on
// the inputs, before the permutation: 2^L multiplications beside the ~2^(L - 1) (L - 2) of the stages.
//
// BETWEEN STAGES THE POINTS ARE AFFINE.  Counted per butterfly, G1 (G2: the same counts over Fq2):
//   XYZZ throughout      walk 254 x 9 + 85 x 15 (ec29_add: the addend has a denominator), u +- t 2 x 15                 = 3,591
//   affine each stage    walk 254 x 9 + 85 x 11, negation of t 1, u +- t 2 x 11, and per POINT the conversion: batched inversion 3 + 330 / 32,
//                        zk_setup_affine 7, back to the tables' form + curve equation 6 = 27                              = 3,298
// 8 % fewer products, the walk is zk_phase2_scale_point's over the same table-form base, and the outputs of the last stage are the
// file's canonical points with nothing more to do.  The conversion is the set-up's series zk_setup_den_k / _inv_k / _affine_k.
//
// DEGENERATE CASES.  ec29_add_mixed tests P = 0 mod q on every call and doubles or returns infinity (zkwg_phase2_core.h); an input or an
// intermediate at infinity is zeros in the affine form, passes through ec29_dbl unchanged and is the neutral element of both additions.
// tau = 1 (all inputs equal: every output but one is infinity) and tau a root of unity are cases of tests/test_ptau_prepare_cpu.py.
//
// BOUNDS ([U, V] of zkwg_fq29.h).  u, v: table-form words, x [1, 1], y [1, 1], -y [2, 2].  The walk: the invariant of zkwg_phase2_core.h,
// t = X [1, 11], Y [1, 7], ZZ, ZZZ [1, 2].  -t: Y times (2 q - 1) [2, 2] -> [1, 2] (7 x 2 <= 169).  t + u, -t + u: ec29_add_mixed takes
// X [1, 11], Y [1, 7] and gives X [1, 11], Y [1, 7], ZZ, ZZZ [1, 2], what zk_setup_den / zk_setup_affine take.
//
// DEVICE MEMORY of one transform, per point: the affine point 64 / 128 bytes, its accumulator 144 / 288, denominator and prefix product
// 36 + 36, half a table entry 32:  312 bytes (G1), 520 (G2).  The largest transform accepted: 2^29 G1 points (168 GB), 2^28 G2 points
// (140 GB) -- the padded level of a power-28 ceremony and its G2 level, on a 288 GB card; above that the call refuses.  The file
// operation adds the section in the tables' form (64 / 128 bytes a point).
#pragma once
#include "zkwg_phase2_core.h"

#define ZK_PTAU_MAX_LOG2_G1 29u
#define ZK_PTAU_MAX_LOG2_G2 28u
#define ZK_PTAU_BYTES_G1 312ull
#define ZK_PTAU_BYTES_G2 520ull
#define ZK_PTAU_TOP 254          // the highest position of a digit string: twiddles are below r < 2^254, so 3 w < 2^256

struct alignas(16) ZkPtauTw { u32 nz[8], neg[8]; };      // bit i: digit i is non-zero / is -1

// non-adjacent form of k < r (standard form): digit i = bit i + 1 of 3 k minus bit i + 1 of k
ZK_HD ZkPtauTw zk_ptau_recode(const Fr& k) {
  u64 h[4], c = 0;
  for (int i = 0; i < 4; ++i) {
    const u64 two = (k.l[i] << 1) | (i ? k.l[i - 1] >> 63 : 0);
    const u64 s = k.l[i] + two;
    const u64 c1 = s < two ? 1u : 0u;
    h[i] = s + c;
    c = c1 + (h[i] < s ? 1u : 0u);
  }
  ZkPtauTw T;
  for (int i = 0; i < 4; ++i) {
    const u64 x = h[i] ^ k.l[i], m = k.l[i] & ~h[i];
    const u64 xn = i < 3 ? h[i + 1] ^ k.l[i + 1] : 0, mn = i < 3 ? k.l[i + 1] & ~h[i + 1] : 0;
    const u64 nz = (x >> 1) | (xn << 63), ng = (m >> 1) | (mn << 63);
    T.nz[2 * i] = (u32)nz; T.nz[2 * i + 1] = (u32)(nz >> 32);
    T.neg[2 * i] = (u32)ng; T.neg[2 * i + 1] = (u32)(ng >> 32);
  }
  return T;
}
ZK_HD u32 zk_ptau_uniform(u32 v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (u32)__builtin_amdgcn_readfirstlane((int)v);
#else
  return v;
#endif
}
// w P for the table-form point P and the table entry of w.  UNIFORM: every lane of the wavefront was given the same entry.
template <class C, bool UNIFORM>
ZK_HD Xyzz29<typename C::F> zk_ptau_mul(const Aff29<typename C::F>& P, const ZkPtauTw* tw) {
  typedef typename C::F F;
  Xyzz29<F> acc = ec29_inf<F>();                                   // (stays infinity through the doublings above the top digit)
  u32 nz = 0, ng = 0;
  for (int i = ZK_PTAU_TOP; i >= 0; --i) {
    if (i == ZK_PTAU_TOP || (i & 31) == 31) {
      nz = tw->nz[i >> 5]; ng = tw->neg[i >> 5];
      if (UNIFORM) { nz = zk_ptau_uniform(nz); ng = zk_ptau_uniform(ng); }
    }
    acc = ec29_dbl<F>(acc);                                        // X [1, 8], Y [1, 7]
    if ((nz >> (i & 31)) & 1u)
      acc = ec29_add_mixed<F>(acc, Aff29<F>{P.x, zk_phase2_neg_if(P.y, ((ng >> (i & 31)) & 1u) != 0), P.inf});     // y [2, 2] -> X [1, 11], Y [1, 7]
  }
  return acc;
}
// -1 in the tables' form, unnormalised: [2, 2]
ZK_HD Fq29 zk_ptau_minus_one() { return fq29_neg<2, 1>(fq29_one()); }
// (u, v) -> (u + w v, u - w v) for table-form points at pu, pv (half h of a lane pair); tw: the entry of w, null for w = 1
template <class C, bool UNIFORM>
ZK_HD void zk_ptau_butterfly(const typename C::Affine* pu, const typename C::Affine* pv, u32 h, const ZkPtauTw* tw, Xyzz29<typename C::F>& sum, Xyzz29<typename C::F>& dif) {
  typedef typename C::F F;
  Xyzz29<F> t;
  {
    const Aff29<F> V = C::load(pv, h, false);                      // x [1, 1], y [1, 1]
    t = tw ? zk_ptau_mul<C, UNIFORM>(V, tw) : ec29_from_affine<F>(V);            // X [1, 11], Y [1, 7], ZZ, ZZZ [1, 2]
  }
  const Aff29<F> U = C::load(pu, h, false);
  sum = ec29_add_mixed<F>(t, U);                                   // X [1, 11], Y [1, 7]
  t.y = F::scale(t.y, zk_ptau_minus_one());                        // [1, 7] x [2, 2] -> [1, 2]
  dif = ec29_add_mixed<F>(t, U);
}
// butterfly t of stage s of a 2^L-point transform: its group-fastest coordinates, the indices of u and v, its twiddle's table entry
struct ZkPtauAt { u64 i0, i1; u32 j; };
ZK_HD ZkPtauAt zk_ptau_at(u32 t, u32 L, u32 s) {
  const u32 lg = L - 1u - s;
  const u32 g = t & ((1u << lg) - 1u), j = t >> lg;
  const u64 i0 = ((u64)g << (s + 1u)) + j;
  return ZkPtauAt{i0, i0 + (1ull << s), j};
}
ZK_HD u32 zk_ptau_bitrev(u32 i, u32 L) {
  u32 r = 0;
  for (u32 b = 0; b < L; ++b) r |= ((i >> b) & 1u) << (L - 1u - b);
  return r;
}

// ---- the table of recoded twiddles (host) ------------------------------------------------------------------------------------------------
static inline Fr zk_ptau_pow_m(Fr base_m, const u64 e[4]) {        // Montgomery in / out
  Fr acc = fr_R();
  for (int i = 255; i >= 0; --i) {
    acc = fr_mont_mul(acc, acc);
    if ((e[i >> 6] >> (i & 63)) & 1) acc = fr_mont_mul(acc, base_m);
  }
  return acc;
}
// the 2^L-th root of unity of ffjavascript's F1Field (s = 28, w[28] = 5^t, w[i] = w[i + 1]^2) or its inverse, Montgomery form
static inline Fr zk_ptau_root_m(u32 L, bool inverse) {
  const u64 r1[4] = {ZK_P0 - 1, ZK_P1, ZK_P2, ZK_P3};
  u64 t[4];
  for (int i = 0; i < 4; ++i) t[i] = (r1[i] >> 28) | (i < 3 ? r1[i + 1] << 36 : 0);
  Fr w = zk_ptau_pow_m(fr_to_mont(fr_from_u64(5)), t);
  for (u32 i = 28; i > L; --i) w = fr_mont_mul(w, w);
  return inverse ? fr_mont_inv(w) : w;
}
struct ZkPtauTable {
  u32 L = 0;
  bool inverse = false;
  std::vector<ZkPtauTw> tw;               // entry e: w^e, e < 2^(L - 1) (one entry, w^0, for L = 0)
  u64 adds[32], dbls[32];                 // group operations of the walks of ONE group of stage s (the sum over its 2^s twiddles)
};
static inline void zk_ptau_table(u32 L, bool inverse, ZkPtauTable& T) {
  T.L = L; T.inverse = inverse;
  const u64 half = L ? 1ull << (L - 1) : 1;
  T.tw.resize(half);
  const Fr w = zk_ptau_root_m(L, inverse);
  Fr acc = fr_R();
  std::vector<u32> add(half), dbl(half);
  for (u64 e = 0; e < half; ++e) {
    const ZkPtauTw D = T.tw[e] = zk_ptau_recode(fr_from_mont(acc));
    u32 n = 0, top = 0;
    for (u32 k = 0; k < 8; ++k) { n += (u32)__builtin_popcount(D.nz[k]); if (D.nz[k]) top = 32 * k + 31 - (u32)__builtin_clz(D.nz[k]); }
    add[e] = n ? n - 1 : 0; dbl[e] = top;
    acc = fr_mont_mul(acc, w);
  }
  for (u32 s = 0; s < 32; ++s) {
    T.adds[s] = T.dbls[s] = 0;
    if (s >= L) continue;
    for (u64 j = 1; j < (1ull << s); ++j) { T.adds[s] += add[j << (L - 1 - s)]; T.dbls[s] += dbl[j << (L - 1 - s)]; }
  }
}
// 2^-q mod r, standard form, little-endian bytes
static inline void zk_ptau_ninv(u32 q, u8 out[32]) {
  const Fr two_inv = fr_mont_inv(fr_to_mont(fr_from_u64(2)));
  Fr acc = fr_R();
  for (u32 i = 0; i < q; ++i) acc = fr_mont_mul(acc, two_inv);
  const Fr s = fr_from_mont(acc);
  memcpy(out, s.l, 32);
}
// group operations of a 2^q-point transform under a table of 2^L >= 2^q: {additions, doublings}
static inline void zk_ptau_ops(const ZkPtauTable& T, u32 q, bool inverse, u64& adds, u64& dbls) {
  for (u32 s = 0; s < q; ++s) {
    const u64 groups = 1ull << (q - 1 - s);
    adds += groups * T.adds[s] + (2ull << (q - 1)); dbls += groups * T.dbls[s];
  }
  if (inverse && q) {
    u8 k[32];
    zk_ptau_ninv(q, k);
    const ZkPhase2Digits D = zk_phase2_recode(k);
    adds += zk_phase2_adds(D) << q; dbls += zk_phase2_dbls(D) << q;
  }
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host mirror of one transform ---------------------------------------------------------------------------------------------------
// accumulators -> canonical affine points in the zkey's form: the series zk_setup_den_k -> zk_setup_inv_k -> zk_setup_affine_k
template <class C>
static inline void zk_ptau_to_affine_host(const std::vector<Xyzz29<typename C::F>>& acc, typename C::Affine* out) {
  const u64 n = acc.size(), n_lanes = (n + ZK_SETUP_INV_BATCH - 1) / ZK_SETUP_INV_BATCH;
  std::vector<Fq29> den(n), pref(n);
  for (u64 i = 0; i < n; ++i) den[i] = zk_setup_den(C(), acc[i]);
  for (u64 l = 0; l < n_lanes; ++l) zk_setup_batch_inv(den.data(), pref.data(), n, l, n_lanes);
  for (u64 i = 0; i < n; ++i) zk_setup_affine<C>(acc[i], den[i], out + i, 0);
}
// 2^q points in the TABLES' form at a (already checked) -> their transform in the zkey's form, in place; T: a table of 2^L >= 2^q
template <class C>
static inline void zk_ptau_transform_host(typename C::Affine* a, u32 q, const ZkPtauTable& T) {
  typedef typename C::F F;
  typedef typename C::Affine A;
  const u64 n = 1ull << q;
  std::vector<Xyzz29<F>> acc(n);
  std::vector<A> tmp(n);
  {                                                               // 2^-q (1 for the forward transform): zk_phase2_scale's walk
    u8 k[32] = {1};
    if (T.inverse) zk_ptau_ninv(q, k);
    const ZkPhase2Digits D = zk_phase2_recode(k);
    for (u64 i = 0; i < n; ++i) acc[i] = zk_phase2_scale_point<C>(a + i, 0, D);
    zk_ptau_to_affine_host<C>(acc, tmp.data());
  }
  if (q == 0) { a[0] = tmp[0]; return; }
  for (u64 i = 0; i < n; ++i) {                                   // back to the tables' form, and the permutation
    zk_phase2_prepare_host(C(), tmp.data(), tmp.data(), i);
    a[zk_ptau_bitrev((u32)i, q)] = tmp[i];
  }
  for (u32 s = 0; s < q; ++s) {
    for (u32 t = 0; t < n / 2; ++t) {
      const ZkPtauAt at = zk_ptau_at(t, q, s);
      zk_ptau_butterfly<C, false>(a + at.i0, a + at.i1, 0, at.j ? &T.tw[(u64)at.j << (T.L - 1 - s)] : nullptr, acc[at.i0], acc[at.i1]);
    }
    zk_ptau_to_affine_host<C>(acc, tmp.data());
    if (s + 1 == q) memcpy((void*)a, (const void*)tmp.data(), n * sizeof(A));
    else for (u64 i = 0; i < n; ++i) zk_phase2_prepare_host(C(), tmp.data(), a, i);
  }
}
// the mirror of zkwg_group_ntt_device: 2^L points in the zkey's form, in place; false: a point is not on its curve (or not reduced)
template <class C>
static inline bool zk_ptau_ntt_host(typename C::Affine* pts, u32 L, bool inverse) {
  const u64 n = 1ull << L;
  std::vector<typename C::Affine> tab(n);
  bool ok = true;
  for (u64 i = 0; i < n; ++i) ok &= zk_phase2_prepare_host(C(), pts, tab.data(), i);
  if (!ok) return false;
  ZkPtauTable T;
  zk_ptau_table(L, inverse, T);
  zk_ptau_transform_host<C>(tab.data(), L, T);
  memcpy((void*)pts, (const void*)tab.data(), n * sizeof(typename C::Affine));
  return true;
}

#endif

// ---- the file operation -----------------------------------------------------------------------------------------------------------------
// Output: sections 1 - 7 of the input cut to `power` (the header's power set, ceremonyPower kept, 2 - 6 cut to 2 n - 1 | n | n | n | 1
// points, 7 verbatim), then 12 - 15.  Level q <= power of section 12 / 13 / 14 / 15 is the inverse transform of the first 2^q points of
// section 2 / 3 / 4 / 5; level power + 1 of section 12 is that of the 2 n - 1 points of section 2 and ONE POINT AT INFINITY (tau^(2 n - 1)
// is not in a file of that power) -- also when `power` cuts a larger file, so prepare(file, P) = prepare(truncate(file, P)).
struct ZkPtauFrame {
  ZkPtauFile in;
  u32 power, n_sections;
  u64 off[16], size[16], out_bytes;       // of the output's sections
};
static inline int zk_ptau_frame(const u8* p, u64 len, u32 power, ZkPtauFrame& F, std::string& err) {
  const int rc = zk_ptau_sections(p, len, F.in, err, false);
  if (rc != ZKWG_RC_OK) return rc;
  for (const ZkPtauSection& s : ZK_PTAU_LAGRANGE)
    if (F.in.off[s.id]) return zk_ptau_fail(err, ".ptau: the file is already prepared (it has a section 12 - 15)");
  if (power > F.in.power) return zk_ptau_fail(err, ".ptau: the power asked for is above the file's");
  F.power = power ? power : F.in.power;
  const u64 n = 1ull << F.power;
  for (int i = 0; i < 16; ++i) F.off[i] = F.size[i] = 0;
  F.size[1] = 44; F.size[2] = (2 * n - 1) * 64; F.size[3] = n * 128; F.size[4] = F.size[5] = n * 64; F.size[6] = 128;
  F.size[7] = F.in.size[7];
  for (const ZkPtauSection& s : ZK_PTAU_LAGRANGE) F.size[s.id] = ((2 * n - 1) + (s.extra_level ? 2 * n : 0)) * s.point;
  u64 pos = 12;
  F.n_sections = 0;
  for (u32 id = 1; id < 16; ++id) {
    if (id >= 8 && id < 12) continue;
    if (id == 7 && !F.in.off[7]) continue;
    pos += 12;
    F.off[id] = pos;
    pos += F.size[id];
    ++F.n_sections;
  }
  F.out_bytes = pos;
  return ZKWG_RC_OK;
}
// section(group, in, count, top, out) -> rc: `in`: `count` points of the file (any byte offset; count = 2^top, or 2^top - 1: pad with one
// point at infinity); writes the inverse transforms of the first 2^q points, q = 0 .. top, back to back at `out`
template <class Section>
static inline int zk_ptau_prepare_apply(const u8* p, const ZkPtauFrame& F, u8* out, Section section) {
  memcpy(out, "ptau", 4);
  const u32 version = 1;
  memcpy(out + 4, &version, 4); memcpy(out + 8, &F.n_sections, 4);
  for (u32 id = 1; id < 16; ++id) {
    if (!F.off[id]) continue;
    memcpy(out + F.off[id] - 12, &id, 4); memcpy(out + F.off[id] - 8, &F.size[id], 8);
    if (id <= 7) memcpy(out + F.off[id], p + F.in.off[id], F.size[id]);        // (the prefix of a larger section)
  }
  memcpy(out + F.off[1] + 36, &F.power, 4);
  const u64 n = 1ull << F.power;
  int rc = section(1, p + F.in.off[2], 2 * n - 1, F.power + 1, out + F.off[12]);
  if (rc == ZKWG_RC_OK) rc = section(2, p + F.in.off[3], n, F.power, out + F.off[13]);
  if (rc == ZKWG_RC_OK) rc = section(1, p + F.in.off[4], n, F.power, out + F.off[14]);
  if (rc == ZKWG_RC_OK) rc = section(1, p + F.in.off[5], n, F.power, out + F.off[15]);
  return rc;
}
#if !defined(__HIP_DEVICE_COMPILE__)
template <class C>
static inline bool zk_ptau_section_host(const u8* in, u64 count, u32 top, u8* out, const ZkPtauTable& T) {
  typedef typename C::Affine A;
  const u64 n = 1ull << top;
  std::vector<A> src(n), tab(n), lvl(n);
  memset((void*)src.data(), 0, n * sizeof(A));
  memcpy((void*)src.data(), in, count * sizeof(A));
  bool ok = true;
  for (u64 i = 0; i < n; ++i) ok &= zk_phase2_prepare_host(C(), src.data(), tab.data(), i);
  if (!ok) return false;
  for (u32 q = 0; q <= top; ++q) {
    const u64 m = 1ull << q;
    memcpy((void*)lvl.data(), (const void*)tab.data(), m * sizeof(A));
    zk_ptau_transform_host<C>(lvl.data(), q, T);
    memcpy(out + (m - 1) * sizeof(A), (const void*)lvl.data(), m * sizeof(A));
  }
  return true;
}
static inline int zk_ptau_prepare_host(const u8* p, u64 len, u32 power, u8* out, u64 cap, u64* out_len, std::string& err) {
  ZkPtauFrame F;
  int rc = zk_ptau_frame(p, len, power, F, err);
  if (rc != ZKWG_RC_OK) return rc;
  if (cap < F.out_bytes) return ZKWG_RC_BAD_ARG;
  ZkPtauTable T;
  zk_ptau_table(F.power + 1, true, T);
  rc = zk_ptau_prepare_apply(p, F, out, [&](int group, const u8* in, u64 count, u32 top, u8* o) {
    const bool ok = group == 1 ? zk_ptau_section_host<ZkEcG1>(in, count, top, o, T) : zk_ptau_section_host<ZkEcG2>(in, count, top, o, T);
    return ok ? (int)ZKWG_RC_OK : zk_ptau_fail(err, "a point of the powers of tau is not on its curve (or not reduced)");
  });
  if (rc == ZKWG_RC_OK && out_len) *out_len = F.out_bytes;
  return rc;
}
#endif
