// Phase 2 of the groth16 set-up: a CONTRIBUTION to a .zkey (snarkjs `zkey contribute` / `zkey beacon`, src/zkey_contribute.js [EXT];
// reference workflow: docs/zk-email-docs/UsageGuide/README.md:149,178-180 "Phase 2", whose next command reads the key AFTER it, :206).
// One header for the library (csrc/zkwg_phase2_api.hip, csrc/zkwg_kernels_phase2.hip) and for the host build of the CPU tests
// (tests/native/phase2test.cpp, ZKWG_FQ29_CHECK counting every violated limb-form bound).
//
//   zk_phase2_recode        a scalar below 2^256 -> its non-adjacent form, two bit strings (non-zero, negative) of at most 257 positions
//   zk_phase2_scale_point   s P for one affine P in the tables' form: what a lane (G2: a lane pair) of zk_phase2_scale runs
//   zk_phase2_scale_host    the host mirror of the series  curve check -> scale -> denominators -> batched inversion -> affine
//   zk_phase2_apply         the file operation, over a callback that scales a run of points (the device's series or the host mirror)
//
// THE OPERATION.  A contribution with secret k replaces delta by k delta:  delta1' = k delta1, delta2' = k delta2, and because the C and H
// bases carry 1 / delta,  C_i' = k^-1 C_i (section 8),  H_j' = k^-1 H_j (section 9).  Sections 1, 3 - 7 and alpha, beta, gamma stay as they
// are; section 10 is the caller's (zkwg/phase2.py writes the record).  Everything is "one scalar times many points".
//
// THE DIGIT STRING.  Every lane multiplies by the SAME scalar, so the scalar is recoded once on the host and the kernel's control flow is
// the same in every lane: from the top digit (always +1) down, one ec29_dbl per position and one ec29_add_mixed of +P or -P per non-zero
// digit.  No table, no branch on data.  Non-adjacent form: digits in {-1, 0, 1}, no two neighbours non-zero, on average 1 / 3 of the
// positions non-zero against 1 / 2 of the binary form zk_setup_mul walks (253 doublings + ~127 additions there, 253 or 254 + ~85 here).
// The recoder takes any value below 2^256 (257 positions): the G2 cofactor 2 q - r of zkwg/phase2.py's challenge point is above r.
// The strings are kernel arguments (scalar registers); a word is SELECTED, not indexed (an indexed argument array would be copied to
// scratch memory, which no point kernel here may use).
//
// WHICH P = +-Q CASES THE CHAIN MEETS.  Before the addition at position i the accumulator is 2 m P, m >= 1 the integer of the digits above
// i, and the addend is d P, d = +-1: the mixed addition's generic formulas fail when 2 m = +-d modulo the order of P.
//   - P in the subgroup of prime order r (every G1 point; the key's G2 points): 2 m = +-1 mod r needs 2 m >= r - 1.  A prefix of the
//     non-adjacent form of s is within 2/3 of s / 2^i, so for s < r - 2 the chain NEVER meets the case.  For s = r - 1, r, r + 1 and
//     the scalars of 255 and 256 bits it can (s = r: the last addition gives infinity), and
//   - a G2 point OUTSIDE the subgroup (the cofactor multiplication) may have a small order that divides 2 q - r, so any position can.
//   ec29_add_mixed tests P = 0 mod q on every call (one compare of a normalised value; the rare path doubles P or returns infinity), so
//   both are computed correctly, not excluded: tests/test_phase2_core_cpu.py multiplies by r - 1, r and r + 1 and, points outside
//   the subgroup, by 2 q - r.  An accumulator at infinity (ZZ = 0) passes through ec29_dbl unchanged and takes the addend in ec29_add_mixed.
//   There is no point of order 2 (both group orders are odd), which ec29_dbl relies on.
//
// BOUNDS ([U, V] of zkwg_fq29.h).  The base is a table-form point: x [1, 1], y [1, 1], the negated y [2, 2] (Aff29).  The accumulator
// starts as (x, y, 1, 1) = X [1, 1], Y [1, 2].  ec29_dbl takes X [1, 11], Y [1, 7] and gives X [1, 8], Y [1, 7], ZZ, ZZZ [1, 2];
// ec29_add_mixed takes the same and gives X [1, 11], Y [1, 7], ZZ, ZZZ [1, 2] (zkwg_ec29.h writes the bound beside every intermediate).
// Both results are inside what both accept, so the bounds are an INVARIANT of the loop and hold after any number of steps -- 254 or 256
// alike; the host build counts violations (ZKWG_FQ29_CHECK) and the CPU tests assert zero.
//
// DEVICE MEMORY.  A run of points is scaled in pieces of at most ZK_PHASE2_PIECE points.  Per point: the table-form point (64 / 128
// bytes; the affine result overwrites it), the accumulator (144 / 288), the denominator and its prefix product (36 + 36):
// 280 bytes (G1), 488 (G2); a piece of 2^20 G1 points is 294 MB whatever the key's size (a power-23 key: 8.4 M points a section).
#pragma once
#include "zkwg_setup_core.h"
#include "zkwg_zkey_core.h"

#define ZK_PHASE2_PIECE (1u << 20)    // points per launch series

struct ZkPhase2Digits {
  u32 nz[9], neg[9];      // bit i: digit i is non-zero / is -1
  u32 len, n_nz;          // positions (top digit at len - 1; 0 for the scalar 0), non-zero digits
};
// non-adjacent form of the 256-bit little-endian integer s
static inline ZkPhase2Digits zk_phase2_recode(const u8* s) {
  u64 k[5] = {0, 0, 0, 0, 0};
  memcpy(k, s, 32);
  ZkPhase2Digits D;
  memset(&D, 0, sizeof D);
  for (u32 i = 0; (k[0] | k[1] | k[2] | k[3] | k[4]) != 0; ++i) {
    if (k[0] & 1) {
      if ((k[0] & 3) == 3) {                       // digit -1: k + 1 is a multiple of 4
        D.neg[i >> 5] |= 1u << (i & 31);
        for (int w = 0; w < 5; ++w) if (++k[w]) break;
      } else {
        k[0] -= 1;                                 // digit +1
      }
      D.nz[i >> 5] |= 1u << (i & 31);
      ++D.n_nz;
      D.len = i + 1;
    }
    for (int w = 0; w < 4; ++w) k[w] = (k[w] >> 1) | (k[w + 1] << 63);
    k[4] >>= 1;
  }
  return D;
}
// word w of a digit string, by selection
ZK_HD u32 zk_phase2_word(const u32 (&a)[9], u32 w) {
  u32 r = a[0];
#pragma unroll
  for (u32 k = 1; k < 9; ++k) r = w == k ? a[k] : r;
  return r;
}
ZK_HD Fq29 zk_phase2_neg_if(const Fq29& y, bool neg) { return zk_q29_neg_if(y, neg); }
#if !defined(__HIP_DEVICE_COMPILE__)
static inline Fq29x2 zk_phase2_neg_if(const Fq29x2& y, bool neg) { return Fq29x2{{zk_q29_neg_if(y.c[0], neg), zk_q29_neg_if(y.c[1], neg)}}; }
#endif
// s P for the table-form point at p (half h of a lane pair); the result is an accumulator in the bounds of Xyzz29
template <class C>
ZK_HD Xyzz29<typename C::F> zk_phase2_scale_point(const typename C::Affine* p, u32 h, const ZkPhase2Digits& D) {
  typedef typename C::F F;
  const Aff29<F> P = C::load(p, h, false);                        // x [1, 1], y [1, 1]
  if (D.len == 0) return ec29_inf<F>();
  Xyzz29<F> acc = ec29_from_affine<F>(P);                         // X [1, 1], Y [1, 2]; infinity stays infinity through the loop
  for (int i = (int)D.len - 2; i >= 0; --i) {
    acc = ec29_dbl<F>(acc);                                       // X [1, 8], Y [1, 7]
    const u32 w = (u32)i >> 5, b = (u32)i & 31u;
    if ((zk_phase2_word(D.nz, w) >> b) & 1u) {
      const bool neg = ((zk_phase2_word(D.neg, w) >> b) & 1u) != 0;
      acc = ec29_add_mixed<F>(acc, Aff29<F>{P.x, zk_phase2_neg_if(P.y, neg), P.inf});      // y [2, 2] -> X [1, 11], Y [1, 7]
    }
  }
  return acc;
}
// group operations of one point under D
static inline u64 zk_phase2_adds(const ZkPhase2Digits& D) { return D.n_nz ? D.n_nz - 1 : 0; }
static inline u64 zk_phase2_dbls(const ZkPhase2Digits& D) { return D.len ? D.len - 1 : 0; }

// ---- the file operation ----------------------------------------------------------------------------------------------------------------
#define ZK_PHASE2_DELTA1_AT (84 + 384)     // section 2: alpha1 at 84, beta1, beta2, gamma2, delta1, delta2
#define ZK_PHASE2_DELTA2_AT (84 + 448)
struct ZkPhase2Frame {
  ZkZkeyHeader H;
  u64 out_off[11], out_bytes;
};
static inline int zk_phase2_fail(std::string& err, const char* m) { err = m; return ZKWG_RC_BAD_CONFIG; }
// the key's sections (sizes checked before any read: zk_zkey_header) and where they go in the new file, sections 1 .. 10 in order
static inline int zk_phase2_frame(const u8* z, u64 len, u64 s10_len, ZkPhase2Frame& F, std::string& err) {
  if (zk_zkey_header(z, len, F.H) != ZKWG_RC_OK) return zk_phase2_fail(err, "not a BN254 groth16 .zkey, truncated, or its section sizes disagree with its header");
  if (!F.H.off[3] || F.H.size[3] != 64ull * ((u64)F.H.n_public + 1)) return zk_phase2_fail(err, ".zkey: section 3 is missing or of the wrong size");
  u64 pos = 12;
  for (int id = 1; id <= 10; ++id) {
    pos += 12;
    F.out_off[id] = pos;
    pos += id == 10 ? s10_len : F.H.size[id];
  }
  F.out_bytes = pos;
  return ZKWG_RC_OK;
}
// k (256-bit little-endian) -> the digits of k mod r and of its inverse mod r; k = 0 mod r is refused
static inline int zk_phase2_scalars(const u8* k32, ZkPhase2Digits& dk, ZkPhase2Digits& dkinv, std::string& err) {
  Fr k;
  memcpy(k.l, k32, 32);
  while (fr_geq(k, fr_p())) { u64 borrow; k = fr_sub_raw(k, fr_p(), borrow); }
  if (fr_is_zero(k)) return zk_phase2_fail(err, "the contribution's scalar is 0 modulo the group order");
  const Fr kinv = fr_from_mont(fr_mont_inv(fr_to_mont(k)));
  dk = zk_phase2_recode((const u8*)k.l);
  dkinv = zk_phase2_recode((const u8*)kinv.l);
  return ZKWG_RC_OK;
}
// scale(group, in, n, digits, out, what) -> rc scales n points of the key (host memory in and out; what: 0 = delta1 / delta2, 8, 9 = the
// section).  out: F.out_bytes bytes.  On a refusal the bytes of out are unspecified.
template <class Scale>
static inline int zk_phase2_apply(const u8* z, const ZkPhase2Frame& F, const ZkPhase2Digits& dk, const ZkPhase2Digits& dkinv, const u8* s10, u64 s10_len, u8* out, Scale scale) {
  const ZkZkeyHeader& H = F.H;
  memcpy(out, "zkey", 4);
  const u32 version = 1, nsec = 10;
  memcpy(out + 4, &version, 4); memcpy(out + 8, &nsec, 4);
  for (u32 id = 1; id <= 10; ++id) {
    const u64 size = id == 10 ? s10_len : H.size[id];
    memcpy(out + F.out_off[id] - 12, &id, 4); memcpy(out + F.out_off[id] - 8, &size, 8);
    if (id == 10) { if (s10_len) memcpy(out + F.out_off[10], s10, s10_len); }
    else if (id != 8 && id != 9) memcpy(out + F.out_off[id], z + H.off[id], size);
  }
  int rc = scale(1, z + H.off[2] + ZK_PHASE2_DELTA1_AT, 1, dk, out + F.out_off[2] + ZK_PHASE2_DELTA1_AT, 0);
  if (rc == ZKWG_RC_OK) rc = scale(2, z + H.off[2] + ZK_PHASE2_DELTA2_AT, 1, dk, out + F.out_off[2] + ZK_PHASE2_DELTA2_AT, 0);
  if (rc == ZKWG_RC_OK) rc = scale(1, z + H.off[8], H.size[8] / 64, dkinv, out + F.out_off[8], 8);
  if (rc == ZKWG_RC_OK) rc = scale(1, z + H.off[9], H.size[9] / 64, dkinv, out + F.out_off[9], 9);
  return rc;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host mirror -----------------------------------------------------------------------------------------------------------------------
static inline bool zk_phase2_prepare_host(ZkEcG1, const G1Affine* in, G1Affine* out, u64 i) { return zk_setup_prepare_point_g1(in, out, i); }
static inline bool zk_phase2_prepare_host(ZkEcG2, const G2Affine* in, G2Affine* out, u64 i) { return zk_setup_prepare_point_g2(in, out, i); }
// out[i] = s in[i] for n points in the zkey's form, through the functions the kernels run; false: a point is not on its curve (or not reduced)
template <class C>
static inline bool zk_phase2_scale_host(const typename C::Affine* in, u64 n, const ZkPhase2Digits& D, typename C::Affine* out) {
  typedef typename C::F F;
  std::vector<typename C::Affine> tab(n);
  bool ok = true;
  for (u64 i = 0; i < n; ++i) ok &= zk_phase2_prepare_host(C(), in, tab.data(), i);
  if (!ok) return false;
  std::vector<Xyzz29<F>> acc(n);
  for (u64 i = 0; i < n; ++i) acc[i] = zk_phase2_scale_point<C>(&tab[i], 0, D);
  const u64 n_lanes = (n + ZK_SETUP_INV_BATCH - 1) / ZK_SETUP_INV_BATCH;
  std::vector<Fq29> den(n), pref(n);
  for (u64 i = 0; i < n; ++i) den[i] = zk_setup_den(C(), acc[i]);
  for (u64 l = 0; l < n_lanes; ++l) zk_setup_batch_inv(den.data(), pref.data(), n, l, n_lanes);
  for (u64 i = 0; i < n; ++i) zk_setup_affine<C>(acc[i], den[i], out + i, 0);
  return true;
}
static inline int zk_phase2_apply_host(const u8* z, u64 len, const u8* k32, const u8* s10, u64 s10_len, u8* out, u64 cap, u64* out_len, std::string& err) {
  ZkPhase2Frame F;
  int rc = zk_phase2_frame(z, len, s10_len, F, err);
  if (rc != ZKWG_RC_OK) return rc;
  if (cap < F.out_bytes) return ZKWG_RC_BAD_ARG;
  ZkPhase2Digits dk, dkinv;
  if ((rc = zk_phase2_scalars(k32, dk, dkinv, err)) != ZKWG_RC_OK) return rc;
  rc = zk_phase2_apply(z, F, dk, dkinv, s10, s10_len, out, [&](int group, const u8* in, u64 n, const ZkPhase2Digits& D, u8* o, int) {
    // (sections sit at any byte offset of the file: the points are copied to aligned storage first)
    bool ok;
    if (group == 1) {
      std::vector<G1Affine> a(n), b(n);
      memcpy((void*)a.data(), in, 64 * n);
      ok = zk_phase2_scale_host<ZkEcG1>(a.data(), n, D, b.data());
      if (ok) memcpy(o, (const void*)b.data(), 64 * n);
    } else {
      std::vector<G2Affine> a(n), b(n);
      memcpy((void*)a.data(), in, 128 * n);
      ok = zk_phase2_scale_host<ZkEcG2>(a.data(), n, D, b.data());
      if (ok) memcpy(o, (const void*)b.data(), 128 * n);
    }
    return ok ? (int)ZKWG_RC_OK : zk_phase2_fail(err, "a point of the key is not on its curve (or not reduced)");
  });
  if (rc == ZKWG_RC_OK && out_len) *out_len = F.out_bytes;
  return rc;
}
#endif
