// A contribution to a powers-of-tau file (snarkjs `powersoftau contribute` / `beacon`, src/powersoftau_contribute.js [EXT]; the reference's
// workflow starts from such a file: docs/zk-email-docs/UsageGuide/README.md:145-180), and the primitive underneath it: MANY POINTS, EACH
// TIMES ITS OWN SCALAR.  One header for the library (csrc/zkwg_ptau_key_api.hip, csrc/zkwg_kernels_ptau_key.hip) and for the host build
// of the CPU tests (tests/native/ptaukeytest.cpp, ZKWG_FQ29_CHECK counting every violated limb-form bound).
//
//   zk_key_recode         a scalar below r -> the bit string its regular digits are read from, and whether it was even
//   zk_key_pop            the top window of that string -> (row of the lane's table, sign)
//   zk_key_power_scalar   c t^idx mod r from the table {c, t^(2^i)}: what a lane computes when the scalars are powers
//   zk_key_table_point    P -> 3 P, 5 P, .., 15 P (accumulators), the rows of the lane's table before they are made affine
//   zk_key_mul            k P over the lane's table: what a lane (G2: a lane pair) of zk_ptau_key_walk runs
//   zk_key_mul_host       the host mirror of the launch series
//   zk_ptau_key_frame / zk_ptau_key_apply / zk_ptau_apply_key_host   the file operation
//
// THE OPERATION.  A contribution with secrets (tau, alpha, beta) multiplies point k of sections 2 and 3 by tau^k, of section 4 by
// alpha tau^k, of section 5 by beta tau^k, and the point of section 6 by beta.  Every point meets a DIFFERENT scalar, so neither the
// shared-scalar walk of phase 2 (zk_phase2_scale: the digits are kernel arguments) nor the fixed-base tables of the prover apply.
//
// REGULAR RECODING (Joye - Tunstall, signed odd digits; window ZK_KEY_W = 4).  An odd k < 2^256 is
//     k = sum_{i < 64} d_i 16^i,   d_i odd, |d_i| <= 15,
// and the digits need no recoder: with u = (k >> 1) | 2^255, window i of u is v_i = (u >> 4 i) & 15 and d_i = 2 v_i + 1 - 16
// (the signed-bit form s_j = 2 bit_(j + 1)(k) - 1, top bit + 1, grouped by four).  v_i >= 8: d_i > 0, row (d_i - 1) / 2 = v_i & 7;
// v_i < 8: d_i < 0, row (|d_i| - 1) / 2 = ~v_i & 7.  EVERY digit is non-zero, so the 64 lanes of a wavefront, each with its own scalar,
// run the same instruction stream: 4 doublings and ONE mixed addition per window, no predication, no skipped position.  The lane's digit
// only SELECTS the row of its table.  For k < r < 2^254 the top window is v_63 = 8 or 9, d_63 = + 1 or + 3: the walk starts from P or 3 P.
// AN EVEN SCALAR is walked as k + 1 (= k | 1) and P is subtracted once at the end: ONE MORE ADDITION (of the point at infinity when k
// was odd), not the negation through r - k -- that is only valid on points of order r, and G2 points are not checked for it.
//
// WHY A WINDOW OF 4 WITH AFFINE ROWS IN DEVICE MEMORY (field products per multiplication, G1; G2: the same counts over Fq2).  RECOUNTED
// from the formulas as zkwg_ec29.h has them, the two-product dot product of Y3 counted as 2: ec29_dbl 4 M + 3 S + 2 = 9, ec29_dbl_affine
// 2 M + 3 S + 2 = 7, ec29_add_mixed 6 M + 2 S + 2 = 10 (NOT the 11 of zkwg_ptau_core.h's table: madd-2008-s is 8 M + 2 S), ec29_add
// 10 M + 2 S + 2 = 14 (not 15: add-2008-s is 12 M + 2 S).  Per point made affine: batched inversion 3 + 330 / 32, zk_setup_affine 7, back
// to the tables' form with the curve equation 6 = 27 (zkwg_ptau_core.h).
//   predicated non-adjacent form, zk_ptau_mul<C, false>         254 x 9 + 254 x 10                                      = 4,826
//   window 2, digits +-1, +-3, 3 P as an accumulator in LDS     254 x 9 + 127 x 14 + (7 + 10)                           = 4,081
//   window 2, 3 P made affine                                   254 x 9 + 127 x 10 + (7 + 10) + 27                      = 3,600
//   window 3, rows P .. 7 P affine in device memory             84 x (27 + 10) + (7 + 10 + 2 x 14) + 3 x 27 + 10        = 3,244
//   window 4, rows P .. 15 P affine in device memory  (BUILT)   63 x (36 + 10) + (7 + 10 + 6 x 14) + 7 x 27 + 10        = 3,198
//   one shared scalar, non-adjacent form (zk_phase2_scale)      254 x 9 + 85 x 10                                       = 3,136
// (the last addend of each sum is the even scalar's fix-up; the curve check in front, 6, and the last conversion, 21, are common to all
// rows and left out).  Window 4 is 1.02 x the shared-scalar walk, the predicated walk 1.54 x (1.58 x with 11 for the mixed addition).
// zkwg_ptau_core.h turned the window down
// because its table does not fit in LDS at three wavefronts per SIMD; here the table is not in LDS at all.  The walk reads one row of
// 64 / 128 bytes per window, 63 x 64 bytes = 4 KB per multiplication against ~3,000 field products (~0.5 M multiply-adds): the reads of
// a 2^20-point piece are 4 GB, a millisecond or two at HBM rates beside ~100 ms of arithmetic, and three wavefronts per SIMD hide their
// latency.  The table is laid out ROW-MAJOR, T[row][point]: lanes of a wavefront that select the same row read neighbouring 64-byte
// points.  Window 5 would save 2 % more products and double the table; GLV is not built.
//
// THE LAUNCH SERIES of a piece of n points (zkwg_ptau_key_api.hip; zk_key_mul_host mirrors it):
//   zk_setup_prepare (curve check, the tables' form -> row 0)  ->  zk_ptau_key_table (rows 1 - 7 as accumulators)  ->  zk_setup_den /
//   _inv / _affine over the 7 n accumulators  ->  zk_setup_prepare over them (the tables' form again; its check can only fail through an
//   internal error)  ->  zk_ptau_key_walk  ->  zk_setup_den / _inv / _affine: canonical affine points in the zkey's form.
//
// WHICH P = +-Q CASES THE WALK MEETS.  Before the addition of window i the accumulator is 16 M P, M >= 1 the odd integer of the digits
// above i, and the addend is d_i P.  With k' = k | 1 <= r the walked scalar, k' = 16^i (16 M + d_i) + L, |L| < 16^i.
//   - P of order r, i >= 1:  0 < 16 M - 15 and 16 M + 15 <= k' / 16^i + 31 < r, so 16 M = +-d_i mod r is impossible.
//   - P of order r, i = 0:   16 M + d_0 = k'.  "Opposite" (16 M + d_0 = 0 mod r) is k' = r, i.e. k = r - 1: the last addition gives
//     INFINITY and the fix-up then adds - P, which is (r - 1) P.  "Equal" (16 M - d_0 = 0 mod r) needs k' = r - 2 |d_0| with d_0 < 0,
//     i.e. (1 - 2 |d_0|) mod 32 - 16 = - |d_0| (r = 1 mod 32): |d_0| = 17 mod 32, no digit.  It never happens.
//   - the fix-up k' P - P:  "opposite" is k' = 1, i.e. k = 0: P - P gives INFINITY, the documented result.  "Equal" needs k' = r - 1, even: never.
//   - the table, j P + 2 P for j = 1 .. 13: never for a point of order r.
//   - P at infinity: every row is infinity, the accumulator stays infinity, the result is zeros.
//   So a reduced scalar on a point of order r meets exactly two cases inside the walk: k = r - 1 (last window) and k = 0 (fix-up); both
//   end at infinity, not at a doubling.  ec29_add_mixed and ec29_add test P = 0 mod q on every call and double or return infinity, so these
//   and whatever a twist point of small order meets are COMPUTED, not excluded (tests/test_ptau_key_cpu.py multiplies by 0, r - 1, ...).
//   For a G2 point outside the subgroup of order r the walk still computes the integer multiple k P, but "c t^k mod r" is then not a
//   homomorphism of the point's group: the result of the powers call is unspecified there (no subgroup check is made, as elsewhere).
//
// BOUNDS ([U, V] of zkwg_fq29.h).  Rows: table-form words, x [1, 1], y [1, 1], a negated y [2, 2] (Aff29, what ec29_add_mixed takes).
// The walk: the invariant of zkwg_phase2_core.h -- ec29_dbl takes X [1, 11], Y [1, 7] and gives X [1, 8], Y [1, 7], ZZ, ZZZ [1, 2];
// ec29_add_mixed takes the same and gives X [1, 11], Y [1, 7], ZZ, ZZZ [1, 2].  The table: 2 P = ec29_dbl_affine(P) is X [1, 7], Y [1, 7],
// ZZ, ZZZ [1, 2]; 3 P = ec29_add_mixed(2 P, P); (j + 2) P = ec29_add(j P, 2 P).  ec29_add's PRECONDITIONS: both operands X [1, 11],
// Y [1, 7], ZZ, ZZZ [1, 2] (X and Y are only left operands of products, ZZ and ZZZ right operands with value bound 2); it gives
// X [1, 10], Y [1, 7], ZZ, ZZZ [1, 2], inside its own preconditions and inside what zk_setup_den / zk_setup_affine take.  The host build
// counts violations (ZKWG_FQ29_CHECK; the scalars' products: ZKWG_FR29_CHECK) and the CPU tests assert zero.
// Scalars: table entries are canonical (limbs < 2^29); fr29_mul returns limbs < 2^29 and a value < a b / 2^261 + r < 1.02 r, which it
// accepts again as its left operand.
//
// DEVICE MEMORY.  Per point of a piece: the table 8 x 64 (G2: 8 x 128) bytes, the accumulators of rows 1 - 7 7 x 144 (7 x 288), their
// denominators and prefix products 7 x (36 + 36):  2,024 bytes (G1), 3,544 (G2).  A piece is at most 2^20 G1 points (2.1 GB) or 2^19 G2
// points (1.9 GB) whatever the file's power.
#pragma once
#include "zkwg_ptau_core.h"
#include "zkwg_fr29.h"

#define ZK_KEY_W 4u
#define ZK_KEY_ROWS 8u                  // P, 3 P, .., 15 P
#define ZK_KEY_DIGITS 64u               // windows of a 256-bit string
#define ZK_KEY_PIECE_G1 (1u << 20)
#define ZK_KEY_PIECE_G2 (1u << 19)
#define ZK_KEY_BYTES_G1 2024ull
#define ZK_KEY_BYTES_G2 3544ull

struct ZkKeyScalar { u32 u[8]; u32 even; };      // u = ((k | 1) >> 1) | 2^255; even: k was even (P is subtracted at the end)

// k: standard form, below r
ZK_HD ZkKeyScalar zk_key_recode(const Fr& k) {
  ZkKeyScalar S;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const u64 w = (k.l[i] >> 1) | (i < 3 ? k.l[i + 1] << 63 : 1ull << 63);
    S.u[2 * i] = (u32)w; S.u[2 * i + 1] = (u32)(w >> 32);
  }
  S.even = (u32)(~k.l[0] & 1ull);
  return S;
}
struct ZkKeyDigit { u32 row; bool neg; };         // the digit is +-(2 row + 1)
// takes the TOP window off the string (which moves up by one window) and returns its digit: the walk reads the windows from the top, and
// a shift by constant amounts needs no indexed word (an indexed private array would live in scratch memory or LDS)
ZK_HD ZkKeyDigit zk_key_pop(ZkKeyScalar& S) {
  const u32 v = S.u[7] >> (32u - ZK_KEY_W);
#pragma unroll
  for (int k = 7; k > 0; --k) S.u[k] = (S.u[k] << ZK_KEY_W) | (S.u[k - 1] >> (32u - ZK_KEY_W));
  S.u[0] <<= ZK_KEY_W;
  const bool pos = (v & 8u) != 0;
  return ZkKeyDigit{(pos ? v : ~v) & 7u, !pos};
}
// any 256-bit value -> below r (2^256 < 6 r)
ZK_HD Fr zk_key_reduce(Fr k) {
  for (int i = 0; i < 6 && fr_geq(k, fr_p()); ++i) { u64 borrow; k = fr_sub_raw(k, fr_p(), borrow); }
  return k;
}

// ---- scalars that are powers: c t^idx ---------------------------------------------------------------------------------------------------
// c and t^(2^i), i < 64, in 2^261-Montgomery form (what fr29_mul keeps), canonical, as limbs
struct alignas(16) ZkKeyPowers { Fr29 c; Fr29 t2[64]; };
ZK_HD Fr zk_key_power_scalar(const ZkKeyPowers* T, u64 idx, u32 n_bits) {
  Fr29 acc = T->c;                                                // canonical
  for (u32 i = 0; i < n_bits; ++i)
    if ((idx >> i) & 1ull) acc = fr29_mul(acc, T->t2[i]);         // limbs < 2^29, value < 1.02 r
  const Fr29 one{{1, 0, 0, 0, 0, 0, 0, 0, 0}};
  return fr29_to_fr(fr29_mul(acc, one));                          // out of the Montgomery form; fr29_to_fr reduces below r
}
static inline Fr zk_key_to_r261(const Fr& std_form) { return fr_mont_mul(fr_to_mont(std_form), fr_to_mont(fr_from_u64(32))); }
// c, t: 32 bytes, little-endian, any value below 2^256; false: one of them is 0 modulo r
static inline bool zk_key_powers_table(const u8* c32, const u8* t32, ZkKeyPowers& T) {
  Fr c, t;
  memcpy(c.l, c32, 32); memcpy(t.l, t32, 32);
  c = zk_key_reduce(c); t = zk_key_reduce(t);
  if (fr_is_zero(c) || fr_is_zero(t)) return false;
  T.c = fr29_from_fr(zk_key_to_r261(c));
  Fr p = fr_to_mont(t);
  for (int i = 0; i < 64; ++i) {
    T.t2[i] = fr29_from_fr(fr_mont_mul(p, fr_to_mont(fr_from_u64(32))));
    p = fr_mont_mul(p, p);
  }
  return true;
}
static inline u32 zk_key_bits(u64 last_idx) { u32 b = 0; while (b < 64 && (last_idx >> b)) ++b; return b; }

// ---- the lane's table and its walk --------------------------------------------------------------------------------------------------------
// rows 1 .. 7 of the table of the table-form point at p (half h of a lane pair), as accumulators: rows[(j - 1) stride] = (2 j + 1) P.
// 2 P is parked in the LAST row's slot and read back for every addition (the slot is overwritten by 15 P at the end): holding it in
// registers beside the running multiple and ec29_add's temporaries costs the G1 kernel its third wavefront per SIMD.
template <class C>
ZK_HD void zk_key_table_point(const typename C::Affine* p, u32 h, Xyzz29<typename C::F>* rows, u64 stride) {
  typedef typename C::F F;
  Xyzz29<F>* const park = rows + (ZK_KEY_ROWS - 2) * stride;
  Xyzz29<F> acc;
  {
    const Aff29<F> P = C::load(p, h, false);                      // x [1, 1], y [1, 1]
    const Xyzz29<F> D = ec29_dbl_affine<F>(P);                    // 2 P: X [1, 7], Y [1, 7], ZZ, ZZZ [1, 2]; infinity for P at infinity
    *park = D;
    acc = ec29_add_mixed<F>(D, P);                                // 3 P: X [1, 11], Y [1, 7]
  }
  rows[0] = acc;
  for (u32 j = 1; j < ZK_KEY_ROWS - 1; ++j) {
    acc = ec29_add<F>(acc, *park);                                // X [1, 10], Y [1, 7], ZZ, ZZZ [1, 2]
    rows[j * stride] = acc;
  }
}
// k P: tab = row 0 of the point (the point itself), row j is `stride` points further
template <class C>
ZK_HD Xyzz29<typename C::F> zk_key_mul(const typename C::Affine* tab, u64 stride, u32 h, ZkKeyScalar S) {
  typedef typename C::F F;
  const ZkKeyDigit top = zk_key_pop(S);                           // + 1 or + 3: the walk starts from P or 3 P
  Xyzz29<F> acc = ec29_from_affine<F>(C::load(tab + top.row * stride, h, false));           // X [1, 1], Y [1, 2]
  for (u32 i = 1; i <= ZK_KEY_DIGITS; ++i) {
    // step 64 is the even scalar's fix-up, through the SAME call of the addition: no doublings, the addend - P (nothing for an odd scalar)
    const bool fix = i == ZK_KEY_DIGITS;
    const u32 n_dbl = fix ? 0u : ZK_KEY_W;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma nounroll
#endif
    for (u32 d = 0; d < n_dbl; ++d) acc = ec29_dbl<F>(acc);       // X [1, 8], Y [1, 7]
    const ZkKeyDigit g = zk_key_pop(S);
    const Aff29<F> A = C::load(tab + (fix ? 0u : g.row) * stride, h, fix || g.neg);          // y [2, 2]
    acc = ec29_add_mixed<F>(acc, Aff29<F>{A.x, A.y, A.inf || (fix && S.even == 0)});         // X [1, 11], Y [1, 7]
  }
  return acc;
}
// group operations per point: additions (walk, fix-up, table), doublings (walk, table)
#define ZK_KEY_ADDS_PER_POINT (ZK_KEY_DIGITS - 1 + 1 + ZK_KEY_ROWS - 1)
#define ZK_KEY_DBLS_PER_POINT ((ZK_KEY_DIGITS - 1) * ZK_KEY_W + 1)

// ---- the file operation -----------------------------------------------------------------------------------------------------------------
// Input: an UNPREPARED file.  Output: sections 1 - 7 in that order; 1 copied, 2 - 6 multiplied, 7 the caller's payload.
struct ZkPtauKeyFrame {
  ZkPtauFile in;
  u64 off[8], size[8], out_bytes;
};
static inline int zk_ptau_key_frame(const u8* p, u64 len, u64 s7_len, ZkPtauKeyFrame& F, std::string& err) {
  const int rc = zk_ptau_sections(p, len, F.in, err, false);
  if (rc != ZKWG_RC_OK) return rc;
  for (const ZkPtauSection& s : ZK_PTAU_LAGRANGE)
    if (F.in.off[s.id]) return zk_ptau_fail(err, ".ptau: the file is already prepared (it has a section 12 - 15)");
  u64 pos = 12;
  for (u32 id = 1; id <= 7; ++id) {
    pos += 12;
    F.off[id] = pos;
    F.size[id] = id == 7 ? s7_len : F.in.size[id];
    pos += F.size[id];
  }
  F.out_bytes = pos;
  return ZKWG_RC_OK;
}
struct ZkPtauKey { u8 tau[32], alpha[32], beta[32]; };            // reduced, none of them 0
static inline int zk_ptau_key_scalars(const u8* tau, const u8* alpha, const u8* beta, ZkPtauKey& K, std::string& err) {
  const u8* in[3] = {tau, alpha, beta};
  u8* out[3] = {K.tau, K.alpha, K.beta};
  for (int i = 0; i < 3; ++i) {
    Fr k;
    memcpy(k.l, in[i], 32);
    k = zk_key_reduce(k);
    if (fr_is_zero(k)) return zk_ptau_fail(err, "the contribution's tau, alpha or beta is 0 modulo the group order");
    memcpy(out[i], k.l, 32);
  }
  return ZKWG_RC_OK;
}
// powers(group, in, count, c, t, out, section) -> rc: out[k] = c t^k in[k] for `count` points of the file (any byte offset, host memory)
// scale(in, k, out) -> rc: the one G2 point of section 6 times k.  On a refusal the bytes of out are unspecified.
template <class Powers, class Scale>
static inline int zk_ptau_key_apply(const u8* p, const ZkPtauKeyFrame& F, const ZkPtauKey& K, const u8* s7, u8* out, Powers powers, Scale scale) {
  memcpy(out, "ptau", 4);
  const u32 version = 1, nsec = 7;
  memcpy(out + 4, &version, 4); memcpy(out + 8, &nsec, 4);
  for (u32 id = 1; id <= 7; ++id) { memcpy(out + F.off[id] - 12, &id, 4); memcpy(out + F.off[id] - 8, &F.size[id], 8); }
  memcpy(out + F.off[1], p + F.in.off[1], F.size[1]);
  if (F.size[7]) memcpy(out + F.off[7], s7, F.size[7]);
  u8 one[32] = {1};
  const u64 n = 1ull << F.in.power;
  int rc = powers(1, p + F.in.off[2], 2 * n - 1, one, K.tau, out + F.off[2], 2);
  if (rc == ZKWG_RC_OK) rc = powers(2, p + F.in.off[3], n, one, K.tau, out + F.off[3], 3);
  if (rc == ZKWG_RC_OK) rc = powers(1, p + F.in.off[4], n, K.alpha, K.tau, out + F.off[4], 4);
  if (rc == ZKWG_RC_OK) rc = powers(1, p + F.in.off[5], n, K.beta, K.tau, out + F.off[5], 5);
  if (rc == ZKWG_RC_OK) rc = scale(p + F.in.off[6], K.beta, out + F.off[6]);
  return rc;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host mirror ----------------------------------------------------------------------------------------------------------------------
// out[i] = k_i in[i] for n points in the zkey's form through the functions the kernels run, in pieces of `piece` points; the scalar of
// point i is scalar(i) (standard form, below r).  false: a point is not on its curve (or not reduced); out is then untouched
template <class C, class ScalarOf>
static inline bool zk_key_mul_host(const typename C::Affine* in, u64 n, ScalarOf scalar, typename C::Affine* out, u64 piece) {
  typedef typename C::F F;
  typedef typename C::Affine A;
  for (u64 i = 0; i < n; ++i) if (!zk_phase2_prepare_host(C(), in, (A*)nullptr, i)) return false;
  for (u64 first = 0; first < n; first += piece) {
    const u64 m = std::min<u64>(piece, n - first);
    std::vector<A> tab(ZK_KEY_ROWS * m), aff((ZK_KEY_ROWS - 1) * m);
    std::vector<Xyzz29<F>> rows((ZK_KEY_ROWS - 1) * m), acc(m);
    for (u64 i = 0; i < m; ++i) zk_phase2_prepare_host(C(), in + first, tab.data(), i);
    for (u64 i = 0; i < m; ++i) zk_key_table_point<C>(&tab[i], 0, rows.data() + i, m);
    zk_ptau_to_affine_host<C>(rows, aff.data());
    for (u64 i = 0; i < (ZK_KEY_ROWS - 1) * m; ++i) if (!zk_phase2_prepare_host(C(), aff.data(), tab.data() + m, i)) return false;   // (never)
    for (u64 i = 0; i < m; ++i) acc[i] = zk_key_mul<C>(&tab[i], m, 0, zk_key_recode(scalar(first + i)));
    zk_ptau_to_affine_host<C>(acc, out + first);
  }
  return true;
}
static inline int zk_ptau_apply_key_host(const u8* p, u64 len, const u8* tau, const u8* alpha, const u8* beta, const u8* s7, u64 s7_len, u8* out, u64 cap,
                                         u64* out_len, u64 piece, std::string& err) {
  ZkPtauKeyFrame F;
  int rc = zk_ptau_key_frame(p, len, s7_len, F, err);
  if (rc != ZKWG_RC_OK) return rc;
  if (cap < F.out_bytes) return ZKWG_RC_BAD_ARG;
  ZkPtauKey K;
  if ((rc = zk_ptau_key_scalars(tau, alpha, beta, K, err)) != ZKWG_RC_OK) return rc;
  const char* const off_curve = "a point of the powers of tau is not on its curve (or not reduced)";
  rc = zk_ptau_key_apply(p, F, K, s7, out, [&](int group, const u8* in, u64 count, const u8* c, const u8* t, u8* o, int) {
    ZkKeyPowers T;
    zk_key_powers_table(c, t, T);                                 // (neither is 0: zk_ptau_key_scalars)
    auto scalar = [&](u64 i) { return zk_key_power_scalar(&T, i, zk_key_bits(count - 1)); };
    bool ok;
    if (group == 1) {
      std::vector<G1Affine> a(count), b(count);
      memcpy((void*)a.data(), in, 64 * count);
      ok = zk_key_mul_host<ZkEcG1>(a.data(), count, scalar, b.data(), piece);
      if (ok) memcpy(o, (const void*)b.data(), 64 * count);
    } else {
      std::vector<G2Affine> a(count), b(count);
      memcpy((void*)a.data(), in, 128 * count);
      ok = zk_key_mul_host<ZkEcG2>(a.data(), count, scalar, b.data(), piece);
      if (ok) memcpy(o, (const void*)b.data(), 128 * count);
    }
    return ok ? (int)ZKWG_RC_OK : zk_ptau_fail(err, off_curve);
  }, [&](const u8* in, const u8* k, u8* o) {
    G2Affine a, b;
    memcpy((void*)&a, in, 128);
    if (!zk_phase2_scale_host<ZkEcG2>(&a, 1, zk_phase2_recode(k), &b)) return zk_ptau_fail(err, off_curve);
    memcpy(o, (const void*)&b, 128);
    return (int)ZKWG_RC_OK;
  });
  if (rc == ZKWG_RC_OK && out_len) *out_len = F.out_bytes;
  return rc;
}
#endif
