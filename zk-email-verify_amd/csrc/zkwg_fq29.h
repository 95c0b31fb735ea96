// BN254 base field Fq in LAZY 9 x 29-bit limb form (Montgomery constant 2^261) -- the arithmetic of the prover's multi-exponentiation
// kernels since round 6 (zkwg_ec29.h builds the G1 / G2 point formulas on it; zkwg_msm_core.h the kernels).
//
// Why (tools/mulbench.hip): on gfx950 v_mad_u64_u32 issues at nearly the plain VALU rate, so a Montgomery product is
// bound by its 162 multiply-adds only when nothing surrounds them.  With 29-bit limbs a column of the schoolbook product (<= 9 products of
// the operands + 9 of the reduction) fits a 64-bit accumulator: no carries inside a product (250 instructions, 1.7 x the 8 x 32-bit CIOS).
// Round 5 used that product behind the 4 x 64-bit interface (split / pack / conditional subtraction around every product: ~315
// instructions, and every addition / subtraction a carry chain + compare + select).  Here values STAY in limb form across a whole point
// formula: an addition is 9 independent adds, a subtraction adds a multiple of q whose limbs dominate the subtrahend's (9 adds + 9
// subs, no borrow), and only three values of a mixed addition are carry-normalised (24 dependent adds / shifts each).
//
// A value is described by two bounds, written [U, V] in the comments: every limb < U 2^29 (the top limb, l[8], is only ever bounded by the
// value), and the value < V q.  Rules:
//   fq29_mul(a, b)       needs Ua Ub <= 6 (9 Ua Ub 2^58 + 9 2^58 < 2^64) and Va Vb <= 169 (then the result is < 2 q); returns [1, Va Vb / 169 + 1]
//   fq29_dot2(a,b,c,d)   a b + c d with ONE reduction: needs Ua Ub + Uc Ud <= 6; returns [1, (Va Vb + Vc Vd) / 169 + 1]   (169 = 2^261 / q)
//   fq29_add             [Ua + Ub, Va + Vb]
//   fq29_sub<M, U>(a, b) a + negc<M, U> - b for b = [U, <= M - 1]; returns [Ua + U + 1, Va + M]
//   fq29_norm            exact carry propagation: [1, V]
// The host build can count every violated precondition (ZKWG_FQ29_CHECK: tests/native/hosttest.cpp, asserted zero by tests/test_ec29_cpu.py),
// on the actual values AND on upper bounds carried beside them: the rules above, executed (tests/test_fq29_bounds_cpu.py).
#pragma once
#include "zkwg_fq.h"

#if !defined(__HIP_DEVICE_COMPILE__) && defined(ZKWG_FQ29_CHECK)
#define ZKQ29_SHADOW 1
#endif
// Host check build only (ZKQ29_SHADOW): a value carries UPPER BOUNDS beside its limbs -- limb i < ub[i] (the U 2^29 of [U, V]), and value <= vb q in units of
// 2^-20 (rounded up wherever it is rounded).  Every fq29_* operation checks its preconditions against the operands' BOUNDS, so one
// execution of a straight-line formula proves it for every input inside the bounds its entry claims (ZKQ29_CLAIM / ZKQ29_ASSUME below).
// ub[0] = ~0 (the default) means "nothing recorded": the bounds are then the limbs themselves, which is exact for the constants.
struct Fq29 {
  u32 l[9];
#if defined(ZKQ29_SHADOW)
  mutable unsigned long long ub[9] = {~0ull, 0, 0, 0, 0, 0, 0, 0, 0};
  mutable unsigned long long vb = 0;
#endif
};
#define ZKQ29_M 0x1fffffffu
#define ZKQ29_N0 0x04866389u     // -q^-1 mod 2^29
#define ZKQ29_PINV 0x1b799c77u   // q^-1 mod 2^29

#if defined(ZKQ29_SHADOW)
// three counters: a precondition violated by the actual VALUES, one violated by the BOUNDS (the worst case over every input the claims
// admit), and a result that exceeds its own bounds (the checker would be wrong: must stay 0 everywhere)
static unsigned long long zk_fq29_violations = 0, zk_fq29_bound_violations = 0, zk_fq29_bound_unsound = 0;
#define ZKQ29_EXPECT(cond) do { if (!(cond)) ++zk_fq29_violations; } while (0)
#define ZKQ29_BOUND(cond) do { if (!(cond)) ++zk_fq29_bound_violations; } while (0)
#include <type_traits>
typedef unsigned __int128 zk_u128;
#define ZKQ29_VONE (1ull << 20)          // vb of exactly q
#define ZKQ29_CAP (1ull << 40)           // bounds saturate here (far outside every precondition)
struct ZkQ29Sh { unsigned long long ub[9], vb; };
static inline zk_u128 zk_q29_qh() { return ((zk_u128)0x30644eull << 64) | 0x72e131a029b85045ull; }          // q >> 168
static inline unsigned long long zk_q29_sat(zk_u128 x) { return x > ZKQ29_CAP ? ZKQ29_CAP : (unsigned long long)x; }
// floor(value / 2^168) of actual limbs, exactly
static inline zk_u128 zk_q29_hi(const u32 l[9]) {
  const zk_u128 lo = (zk_u128)l[0] + ((zk_u128)l[1] << 29) + ((zk_u128)l[2] << 58);
  const zk_u128 mid = (lo >> 87) + (zk_u128)l[3] + ((zk_u128)l[4] << 29) + ((zk_u128)l[5] << 58);
  return (mid >> 81) + ((zk_u128)l[6] << 6) + ((zk_u128)l[7] << 35) + ((zk_u128)l[8] << 64);
}
// value <= vb q 2^-20  =>  value >> 168 <= this, and value >> 232 (the top limb of a carried value) < zk_q29_top
static inline zk_u128 zk_q29_vmax(unsigned long long vb) { return ((zk_u128)vb * (zk_q29_qh() + 1)) >> 20; }
static inline unsigned long long zk_q29_top(unsigned long long vb) { return zk_q29_sat((zk_q29_vmax(vb) >> 64) + 1); }
static inline ZkQ29Sh zk_q29_sh(const Fq29& a) {
  ZkQ29Sh s;
  if (a.ub[0] != ~0ull) { for (int i = 0; i < 9; ++i) s.ub[i] = a.ub[i]; s.vb = a.vb; return s; }
  for (int i = 0; i < 9; ++i) s.ub[i] = (unsigned long long)a.l[i] + 1;
  s.vb = zk_q29_sat((((zk_q29_hi(a.l) + 1) << 20) + zk_q29_qh() - 1) / zk_q29_qh());      // value < (hi + 1) 2^168, q >= (q >> 168) 2^168
  u32 any = 0;
  for (int i = 0; i < 9; ++i) any |= a.l[i];
  if (!any) s.vb = 0;          // (zero is exact: 0 + M q must stay [*, M])
  return s;
}
// records the bounds of a result and checks the checker: no actual limb, nor the actual value, may exceed them
static inline void zk_q29_set(const Fq29& r, const ZkQ29Sh& s) {
  bool ok = zk_q29_hi(r.l) <= zk_q29_vmax(s.vb);
  for (int i = 0; i < 9; ++i) { r.ub[i] = s.ub[i]; ok = ok && r.l[i] < s.ub[i]; }
  r.vb = s.vb;
  if (!ok) ++zk_fq29_bound_unsound;
}
// [U, V] as bounds: limbs 0 .. 7 < U 2^29, the top limb by the value alone
static inline ZkQ29Sh zk_q29_uv(unsigned long long U, double V) {          // (V: an integer or a dyadic fraction such as 10.25 -- exact in 2^-20)
  ZkQ29Sh s;
  for (int i = 0; i < 8; ++i) s.ub[i] = U << 29;
  s.vb = (unsigned long long)(V * (double)ZKQ29_VONE);
  if ((double)s.vb < V * (double)ZKQ29_VONE) ++s.vb;
  s.ub[8] = zk_q29_top(s.vb);
  return s;
}
// ZKQ29_CLAIM(x, U, V): the bounds of x must be inside [U, V], and ARE [U, V] from here on (so that one trip through a loop body, or one
// call of a formula, is checked from the top of its contract).  ZKQ29_ASSUME only sets them: for a value whose range someone else enforces.
static inline void zk_q29_claim(const Fq29& x, unsigned long long U, double V, bool check) {
  const ZkQ29Sh c = zk_q29_uv(U, V);
  if (check) {
    const ZkQ29Sh s = zk_q29_sh(x);
    bool ok = s.vb <= c.vb;
    for (int i = 0; i < 9; ++i) ok = ok && s.ub[i] <= c.ub[i];
    ZKQ29_BOUND(ok);
  }
  zk_q29_set(x, c);
}
// a value chosen between a and b limb by limb (selects): the larger of both bounds
static inline void zk_q29_select(const Fq29& r, const Fq29& a, const Fq29& b) {
  ZkQ29Sh s = zk_q29_sh(a);
  const ZkQ29Sh t = zk_q29_sh(b);
  for (int i = 0; i < 9; ++i) s.ub[i] = s.ub[i] > t.ub[i] ? s.ub[i] : t.ub[i];
  s.vb = s.vb > t.vb ? s.vb : t.vb;
  zk_q29_set(r, s);
}
// value bound <= V q: the template argument of a conversion, a zero test or a product (its named operand)
static inline void zk_q29_need_v(const Fq29& a, unsigned long long V) { ZKQ29_BOUND(zk_q29_sh(a).vb <= V * ZKQ29_VONE); }
// a b (+ c d) with one reduction: the column sums on the limb bounds, then limbs 0 .. 7 < 2^29 and value < (Ba Bb + Bc Bd) / 2^261 + q
static inline void zk_q29_product(const Fq29& r, const Fq29& a, const Fq29& b, const Fq29* c, const Fq29* d) {
  const ZkQ29Sh sa = zk_q29_sh(a), sb = zk_q29_sh(b), sc = c ? zk_q29_sh(*c) : ZkQ29Sh{}, sd = d ? zk_q29_sh(*d) : ZkQ29Sh{};
  zk_u128 worst = 0;
  for (int k = 0; k < 17; ++k) {
    zk_u128 s = (zk_u128)9 << 58;
    for (int i = 0; i < 9; ++i) if (k - i >= 0 && k - i < 9) {
      s += (zk_u128)zk_q29_sat(sa.ub[i]) * zk_q29_sat(sb.ub[k - i]);
      if (c) s += (zk_u128)zk_q29_sat(sc.ub[i]) * zk_q29_sat(sd.ub[k - i]);
    }
    if (s > worst) worst = s;
  }
  ZKQ29_BOUND(worst < ((zk_u128)1 << 64) - ((zk_u128)1 << 36));
  const zk_u128 vv = (zk_u128)sa.vb * sb.vb + (c ? (zk_u128)sc.vb * sd.vb : 0);          // in 2^-40 q^2
  ZkQ29Sh s;
  // q / 2^261 <= ((q >> 200) + 1) / 2^61
  s.vb = vv > ((zk_u128)1 << 70) ? ZKQ29_CAP : zk_q29_sat(((vv * 0x30644e72e131a1ull + (((zk_u128)1 << 81) - 1)) >> 81) + ZKQ29_VONE);
  for (int i = 0; i < 8; ++i) s.ub[i] = 1ull << 29;
  s.ub[8] = zk_q29_top(s.vb);
  ZKQ29_BOUND(s.ub[8] <= (1ull << 32));          // the last carry fits the top limb
  zk_q29_set(r, s);
}
static inline unsigned long long zk_fq29_all_violations() { return zk_fq29_violations + zk_fq29_bound_violations + zk_fq29_bound_unsound; }
#define ZKQ29_CLAIM(x, U, V) zk_q29_claim((x), (U), (V), true)
#define ZKQ29_ASSUME(x, U, V) zk_q29_claim((x), (U), (V), false)
// ZKQ29_CLAIM_IN(x, U, V): ZKQ29_CLAIM for an INPUT of a formula -- the caller's own bounds come back when the scope ends, so what a formula
// assumes of its operand at worst does not leak into the code after the call (a declaration: not inside do { } while (0))
template <class T> struct ZkQ29In;
template <> struct ZkQ29In<Fq29> {
  const Fq29& x;
  unsigned long long ub[9], vb;
  ZkQ29In(const Fq29& x_, unsigned long long U, double V) : x(x_) { for (int i = 0; i < 9; ++i) ub[i] = x.ub[i]; vb = x.vb; zk_q29_claim(x, U, V, true); }
  ~ZkQ29In() { for (int i = 0; i < 9; ++i) x.ub[i] = ub[i]; x.vb = vb; }
};
#define ZKQ29_CAT2(a, b) a##b
#define ZKQ29_CAT(a, b) ZKQ29_CAT2(a, b)
#define ZKQ29_CLAIM_IN(x, U, V) ZkQ29In<std::decay_t<decltype(x)>> ZKQ29_CAT(zk_q29_in_, __COUNTER__)((x), (U), (V))
#define ZKQ29_NEED_V(x, V) zk_q29_need_v((x), (V))
#define ZKQ29_SELECT(r, a, b) zk_q29_select((r), (a), (b))
#else
#define ZKQ29_EXPECT(cond) do { } while (0)
#define ZKQ29_CLAIM(x, U, V) do { } while (0)
#define ZKQ29_ASSUME(x, U, V) do { } while (0)
#define ZKQ29_CLAIM_IN(x, U, V) do { } while (0)
#define ZKQ29_NEED_V(x, V) do { } while (0)
#define ZKQ29_SELECT(r, a, b) do { } while (0)
#endif

// the limbs of q, and a few constants in limb form (Python: oracle/pyref/bn254_g1.Q)
#define ZKQ29_P(i) ((i) == 0 ? 0x187cfd47u : (i) == 1 ? 0x010460b6u : (i) == 2 ? 0x1c72a34fu : (i) == 3 ? 0x02d522d0u : (i) == 4 ? 0x1585d978u : (i) == 5 ? 0x02db40c0u : (i) == 6 ? 0x00a6e141u : (i) == 7 ? 0x0e5c2634u : 0x0030644eu)
ZK_HD Fq29 fq29_zero() { return Fq29{{0, 0, 0, 0, 0, 0, 0, 0, 0}}; }
ZK_HD Fq29 fq29_one() { return Fq29{{0x157ccc21u, 0x141c2758u, 0x185230d3u, 0x014c0419u, 0x0aa36fb9u, 0x1d4240ceu, 0x11d54c07u, 0x052ac7a8u, 0x000dc836u}}; }      // 2^261 mod q
ZK_HD Fq29 fq29_r256() { return Fq29{{0x058f0d9du, 0x1aea1c6eu, 0x11c2cf74u, 0x11d651ebu, 0x1462c0a7u, 0x11b7bc3cu, 0x1cbd99bau, 0x183340fbu, 0x000e0a77u}}; }     // 2^256 mod q: x 2^261 -> x 2^256
ZK_HD Fq29 fq29_t266() { return Fq29{{0x13349ca1u, 0x1a5d84a8u, 0x0a3e5cacu, 0x100249e0u, 0x12b951e8u, 0x0e92d304u, 0x14cb95b3u, 0x041b9d3du, 0x00058003u}}; }     // 2^266 mod q: x 2^256 -> x 2^261

// 4 x 64-bit words (value < 2^256) <-> limbs
ZK_HD Fq29 fq29_split(const u64 x[4]) {
  Fq29 r;
  zk29_split<0>(x, r.l);
  r.l[8] = (u32)(x[3] >> 40);      // (zk29_split masks the top limb to 29 bits: 24 bits are there)
#if defined(ZKQ29_SHADOW)
  { ZkQ29Sh s; for (int i = 0; i < 8; ++i) s.ub[i] = 1ull << 29; s.ub[8] = 1ull << 24; s.vb = zk_q29_sat((((zk_u128)1 << 108) / zk_q29_qh()) + 1); zk_q29_set(r, s); }      // any 256-bit word: value < 2^256
#endif
  return r;
}
ZK_HD Fq29 fq29_from_fq(const Fq& a) { return fq29_split(a.l); }
// exact carry propagation: limbs 0 .. 7 < 2^29, the value unchanged (it must stay below 2^261: V <= 169)
ZK_HD Fq29 fq29_norm(const Fq29& a) {
  Fq29 r;
  u32 c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const u32 t = a.l[i] + c;          // limbs < 2^32 - 2^3: callers keep U <= 7
    ZKQ29_EXPECT(t >= c);
    r.l[i] = t & ZKQ29_M;
    c = t >> 29;
  }
  r.l[8] = a.l[8] + c;
  ZKQ29_EXPECT(r.l[8] >= c);
#if defined(ZKQ29_SHADOW)
  {
    const ZkQ29Sh sa = zk_q29_sh(a);
    ZkQ29Sh s;
    unsigned long long cb = 0;
    bool ok = zk_q29_vmax(sa.vb) < ((zk_u128)1 << 93);          // the value stays below 2^261
    for (int i = 0; i < 8; ++i) { const unsigned long long t = sa.ub[i] + cb; ok = ok && t <= (1ull << 32); s.ub[i] = t < (1ull << 29) ? t : 1ull << 29; cb = (t - 1) >> 29; }          // limb + carry < t
    ok = ok && sa.ub[8] + cb <= (1ull << 32);
    const unsigned long long top = zk_q29_top(sa.vb);
    s.ub[8] = sa.ub[8] + cb < top ? sa.ub[8] + cb : top;
    s.vb = sa.vb;
    ZKQ29_BOUND(ok);
    zk_q29_set(r, s);
  }
#endif
  return r;
}
// k q in plain limbs (k small), for the exact comparisons of the slow paths
ZK_HD Fq29 fq29_kp(u32 k) {
  Fq29 r;
  u64 c = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    c += (u64)k * ZKQ29_P(i);
    r.l[i] = i < 8 ? ((u32)c & ZKQ29_M) : (u32)c;
    c >>= 29;
  }
  return r;
}
// value == 0 mod q for a = [*, <= V]?  The filter costs three instructions: the low 29 bits of limb 0 are exact whatever the other
// limbs carry, and k q = those bits (mod 2^29) for exactly one k < 2^29 -- a value that is no multiple of q passes with probability
// (V + 1) 2^-29, and then the exact comparison decides.
template <int V>
ZK_HD bool fq29_maybe_zero(const Fq29& a) {
#if defined(ZKQ29_SHADOW)
  zk_q29_need_v(a, V);
#endif
  return ((a.l[0] * ZKQ29_PINV) & ZKQ29_M) <= (u32)V;
}
template <int V>
ZK_HD bool fq29_is_zero_mod(const Fq29& a) {
#if defined(ZKQ29_SHADOW)
  zk_q29_need_v(a, V);
#endif
  const u32 k = (a.l[0] * ZKQ29_PINV) & ZKQ29_M;
  if (k > (u32)V) return false;
  const Fq29 n = fq29_norm(a), kp = fq29_kp(k);
  u32 d = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) d |= n.l[i] ^ kp.l[i];
  return d == 0;
}
ZK_HD bool fq29_all_zero(const Fq29& a) {
  u32 d = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) d |= a.l[i];
  return d == 0;
}
// canonical: the value reduced below q, as 4 x 64-bit words (a = [*, <= V], V <= 40)
template <int V>
ZK_HD Fq fq29_to_fq(const Fq29& a) {
#if defined(ZKQ29_SHADOW)
  zk_q29_need_v(a, V);
#endif
  Fq29 n = fq29_norm(a);
  // subtract q while >= q: binary steps 32 q, 16 q, ... q
#pragma unroll
  for (int s = 5; s >= 0; --s) {
    if ((1 << s) > V) continue;
    const Fq29 kp = fq29_kp(1u << s);
    // n >= kp ?
    bool ge = true;
#pragma unroll
    for (int i = 8; i >= 0; --i) {
      if (n.l[i] != kp.l[i]) { ge = n.l[i] > kp.l[i]; break; }
    }
    if (ge) {
      u32 bw = 0;
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        const u32 t = n.l[i] - kp.l[i] - bw;
        bw = i < 8 ? (t >> 31) : 0;                // limbs < 2^29: a borrow shows in the top bit
        n.l[i] = i < 8 ? (t & ZKQ29_M) : t;
      }
    }
  }
  u64 w[4] = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const int bit = 29 * i, k = bit >> 6, s = bit & 63;
    w[k] |= (u64)n.l[i] << s;
    if (s > 64 - 29 && k + 1 < 4) w[k + 1] |= (u64)n.l[i] >> (64 - s);
  }
  return Fq{{w[0], w[1], w[2], w[3]}};
}

// ---- products ------------------------------------------------------------------------------------------------------------------------
ZK_HD Fq29 fq29_mul(const Fq29& a, const Fq29& b) {
  u32 q[9];
  Fq29 r;
  u64 acc = 0;
#if defined(ZKQ29_SHADOW)
  { unsigned __int128 worst = 0; for (int k = 0; k < 17; ++k) { unsigned __int128 s = (unsigned __int128)9 << 58; for (int i = 0; i < 9; ++i) if (k - i >= 0 && k - i < 9) s += (unsigned __int128)a.l[i] * b.l[k - i]; if (s > worst) worst = s; } ZKQ29_EXPECT(worst < ((unsigned __int128)1 << 64) - ((unsigned __int128)1 << 36)); }
#endif
#pragma unroll
  for (int k = 0; k < 9; ++k) {
#pragma unroll
    for (int i = 0; i <= k; ++i) acc += (u64)a.l[i] * b.l[k - i];
#pragma unroll
    for (int i = 0; i < k; ++i) acc += (u64)q[i] * ZKQ29_P(k - i);
    q[k] = ((u32)acc * ZKQ29_N0) & ZKQ29_M;
    acc += (u64)q[k] * ZKQ29_P(0);
    acc >>= 29;
  }
#pragma unroll
  for (int k = 9; k < 17; ++k) {
#pragma unroll
    for (int i = k - 8; i < 9; ++i) acc += (u64)a.l[i] * b.l[k - i];
#pragma unroll
    for (int i = k - 8; i < 9; ++i) acc += (u64)q[i] * ZKQ29_P(k - i);
    r.l[k - 9] = (u32)acc & ZKQ29_M;
    acc >>= 29;
  }
  ZKQ29_EXPECT(acc < (1ull << 32));
  r.l[8] = (u32)acc;
#if defined(ZKQ29_SHADOW)
  zk_q29_product(r, a, b, nullptr, nullptr);
#endif
  return r;
}
// a a: the cross products once, against the doubled limbs (45 multiply-adds for the operand part instead of 81); a = [<= 3, *]
ZK_HD Fq29 fq29_sqr(const Fq29& a) {
  u32 q[9], d[9];
  Fq29 r;
  u64 acc = 0;
#if defined(ZKQ29_SHADOW)
  { unsigned __int128 worst = 0; for (int k = 0; k < 17; ++k) { unsigned __int128 s = (unsigned __int128)9 << 58; for (int i = 0; i < 9; ++i) if (k - i >= 0 && k - i < 9) s += (unsigned __int128)a.l[i] * a.l[k - i]; if (s > worst) worst = s; } ZKQ29_EXPECT(worst < ((unsigned __int128)1 << 64) - ((unsigned __int128)1 << 36)); for (int i = 0; i < 9; ++i) ZKQ29_EXPECT(a.l[i] < (1u << 31)); }
#endif
#pragma unroll
  for (int i = 0; i < 9; ++i) d[i] = a.l[i] << 1;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
#pragma unroll
    for (int i = 0; 2 * i < k; ++i) acc += (u64)d[i] * a.l[k - i];
    if ((k & 1) == 0) acc += (u64)a.l[k / 2] * a.l[k / 2];
#pragma unroll
    for (int i = 0; i < k; ++i) acc += (u64)q[i] * ZKQ29_P(k - i);
    q[k] = ((u32)acc * ZKQ29_N0) & ZKQ29_M;
    acc += (u64)q[k] * ZKQ29_P(0);
    acc >>= 29;
  }
#pragma unroll
  for (int k = 9; k < 17; ++k) {
#pragma unroll
    for (int i = k - 8; 2 * i < k; ++i) acc += (u64)d[i] * a.l[k - i];
    if ((k & 1) == 0) acc += (u64)a.l[k / 2] * a.l[k / 2];
#pragma unroll
    for (int i = k - 8; i < 9; ++i) acc += (u64)q[i] * ZKQ29_P(k - i);
    r.l[k - 9] = (u32)acc & ZKQ29_M;
    acc >>= 29;
  }
  ZKQ29_EXPECT(acc < (1ull << 32));
  r.l[8] = (u32)acc;
#if defined(ZKQ29_SHADOW)
  { const ZkQ29Sh sa = zk_q29_sh(a); for (int i = 0; i < 9; ++i) ZKQ29_BOUND(sa.ub[i] <= (1ull << 31)); }          // the doubled limbs
  zk_q29_product(r, a, a, nullptr, nullptr);
#endif
  return r;
}
// a b + c d, one reduction
ZK_HD Fq29 fq29_dot2(const Fq29& a, const Fq29& b, const Fq29& c, const Fq29& d) {
  u32 q[9];
  Fq29 r;
  u64 acc = 0;
#if defined(ZKQ29_SHADOW)
  { unsigned __int128 worst = 0; for (int k = 0; k < 17; ++k) { unsigned __int128 s = (unsigned __int128)9 << 58; for (int i = 0; i < 9; ++i) if (k - i >= 0 && k - i < 9) s += (unsigned __int128)a.l[i] * b.l[k - i] + (unsigned __int128)c.l[i] * d.l[k - i]; if (s > worst) worst = s; } ZKQ29_EXPECT(worst < ((unsigned __int128)1 << 64) - ((unsigned __int128)1 << 36)); }
#endif
#pragma unroll
  for (int k = 0; k < 9; ++k) {
#pragma unroll
    for (int i = 0; i <= k; ++i) { acc += (u64)a.l[i] * b.l[k - i]; acc += (u64)c.l[i] * d.l[k - i]; }
#pragma unroll
    for (int i = 0; i < k; ++i) acc += (u64)q[i] * ZKQ29_P(k - i);
    q[k] = ((u32)acc * ZKQ29_N0) & ZKQ29_M;
    acc += (u64)q[k] * ZKQ29_P(0);
    acc >>= 29;
  }
#pragma unroll
  for (int k = 9; k < 17; ++k) {
#pragma unroll
    for (int i = k - 8; i < 9; ++i) { acc += (u64)a.l[i] * b.l[k - i]; acc += (u64)c.l[i] * d.l[k - i]; }
#pragma unroll
    for (int i = k - 8; i < 9; ++i) acc += (u64)q[i] * ZKQ29_P(k - i);
    r.l[k - 9] = (u32)acc & ZKQ29_M;
    acc >>= 29;
  }
  ZKQ29_EXPECT(acc < (1ull << 32));
  r.l[8] = (u32)acc;
#if defined(ZKQ29_SHADOW)
  zk_q29_product(r, a, b, &c, &d);
#endif
  return r;
}

// ---- sums and differences ---------------------------------------------------------------------------------------------------------------
ZK_HD Fq29 fq29_add(const Fq29& a, const Fq29& b) {
  Fq29 r;
#pragma unroll
  for (int i = 0; i < 9; ++i) { r.l[i] = a.l[i] + b.l[i]; ZKQ29_EXPECT(r.l[i] >= a.l[i]); }
#if defined(ZKQ29_SHADOW)
  {
    ZkQ29Sh s = zk_q29_sh(a);
    const ZkQ29Sh sb = zk_q29_sh(b);
    for (int i = 0; i < 9; ++i) { s.ub[i] = zk_q29_sat((zk_u128)s.ub[i] + sb.ub[i]); ZKQ29_BOUND(s.ub[i] <= (1ull << 32)); }
    s.vb = zk_q29_sat((zk_u128)s.vb + sb.vb);
    zk_q29_set(r, s);
  }
#endif
  return r;
}
ZK_HD Fq29 fq29_dbl(const Fq29& a) { return fq29_add(a, a); }
// M q written so that it dominates a [U, M - 1] value limb by limb: c_i = U 2^29 + e_i (i < 8), c_8 = e_8 with
// e = M q - sum_{i = 1..8} U 2^(29 i) in plain limbs.  Compile-time constants.
struct Fq29C { u32 l[9]; };
template <int M, int U>
constexpr Fq29C fq29_negc_make() {
  u64 m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, c = 0;
  for (int i = 0; i < 9; ++i) { c += (u64)M * ZKQ29_P(i); m[i] = i < 8 ? (c & ZKQ29_M) : c; c >>= 29; }
  u64 bw = 0;
  for (int i = 1; i < 9; ++i) {
    const u64 sub = (u64)U + bw;
    if (i < 8) { if (m[i] >= sub) { m[i] -= sub; bw = 0; } else { m[i] = m[i] + (1u << 29) - sub; bw = 1; } }
    else m[i] -= sub;          // (M q >> 232 is far above U + 1 for every M >= 1)
  }
  Fq29C r{};
  for (int i = 0; i < 9; ++i) r.l[i] = i < 8 ? (u32)(m[i] + ((u64)U << 29)) : (u32)m[8];
  return r;
}
template <int M, int U>
ZK_HD Fq29 fq29_negc() {
  constexpr Fq29C c = fq29_negc_make<M, U>();
  return Fq29{{c.l[0], c.l[1], c.l[2], c.l[3], c.l[4], c.l[5], c.l[6], c.l[7], c.l[8]}};
}
// a - b + M q for b = [U, <= M - 1]
template <int M, int U>
ZK_HD Fq29 fq29_sub(const Fq29& a, const Fq29& b) {
  const Fq29 c = fq29_negc<M, U>();
  Fq29 r;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    ZKQ29_EXPECT(c.l[i] >= b.l[i]);
    r.l[i] = a.l[i] + (c.l[i] - b.l[i]);
    ZKQ29_EXPECT(r.l[i] >= a.l[i]);
  }
#if defined(ZKQ29_SHADOW)
  {
    ZkQ29Sh s = zk_q29_sh(a);
    const ZkQ29Sh sb = zk_q29_sh(b);
    ZKQ29_BOUND(sb.vb <= (unsigned long long)(M - 1) * ZKQ29_VONE);
    for (int i = 0; i < 9; ++i) { ZKQ29_BOUND(sb.ub[i] <= (unsigned long long)c.l[i] + 1); s.ub[i] = zk_q29_sat((zk_u128)s.ub[i] + c.l[i]); ZKQ29_BOUND(s.ub[i] <= (1ull << 32)); }
    s.vb = zk_q29_sat((zk_u128)s.vb + (unsigned long long)M * ZKQ29_VONE);
    zk_q29_set(r, s);
  }
#endif
  return r;
}
template <int M, int U>
ZK_HD Fq29 fq29_neg(const Fq29& b) { return fq29_sub<M, U>(fq29_zero(), b); }
