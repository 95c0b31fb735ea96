// The zkey as a constraint system of its own: what `groth16.prove(zkey, wtns)` needs of the two files, for a host build and the device
// alike (reference call site: snarkjs.groth16.fullProve(input, wasm, zkey), packages/helpers/src/chunked-zkey.ts:80-84).
//
//   zk_zkey_header     the section walker and header reader of a groth16 .zkey (layout: zkwg/zkey.py), lengths checked before any read
//   zk_zkey_rows       section 4 -> the row table the device evaluates (below)
//   zk_zkey_b_bitmaps  the B1 and B2 base sets have their points at infinity at the same wires (the sums share one classification)
//   zk_wtns_parse      a `.wtns` file -> where its values are (layout: SURVEY.md a20, zkwg_write_wtns is the writer)
//   zk_zkey_row        the evaluation of one row for G witnesses: the kernels of zkwg_kernels_zkey.hip and the host mirror of the CPU
//                      tests (tests/native/zkeytest.cpp, ZKWG_FR29_CHECK counting every violated bound) compile the same function
//
// THE ROW TABLE.  Constraint j has the rows 2 j (its A terms) and 2 j + 1 (its B terms).  The kind tag of the .r1cs loader
// (ZK_COEF_ONE / ZK_COEF_MINUS_ONE / ZK_COEF_GENERIC, zkwg_r1cs.h) decides where a term goes: the +-1 terms of a row -- two thirds of
// EmailVerifier's -- are `unit` words (wire | sign << 31) and cost additions only, the others are (wire, coefficient) pairs.
//
// WHICH FORM.  Section 4 stores coefficient x 2^512 mod r.  The device reduces with 9 limbs of 29 bits, i.e. divides by 2^261
// (zkwg_fr29.h), and a row's result must be (sum c x) 2^256 mod r for a standard-form witness x.  So the table holds
//     gcoef = coefficient x 2^517 mod r  (the stored value doubled five times; canonical words)        k1 = 2^517 mod r
// and ONE reduction of  sum x gcoef  resp. of  (sum +-x) k1  lands in Montgomery form with R = 2^256, as the transforms want it.
//
// BOUNDS ([U, V] of zkwg_fq29.h: limbs 0 .. 7 < U 2^29, value < V r).  A witness value is only known to be < 2^256 here (a value >= r
// is reported by zk_zkey_range and its witness gets no proof, but its terms are never dropped and no bound depends on it):
//   unit terms   at most ZK_ZKEY_BLOCK = 64 values are added / subtracted word by word into 8 signed 64-bit columns of 32-bit words
//                (|column| < 64 2^32 = 2^38), so |S| < 2^262 < 512 r = 2^262.6: S + 512 r is in (0, 2^263.4), nine words with the top one
//                < 2^8, as limbs [1, .] with l[8] < 2^32 -- fr29_mul's operand a; its result is < 2^263.4 r / 2^261 + r < 6.3 r: fr29_to_fr_v<8>
//   other terms  a product of two [1, .] operands (x: l[8] < 2^24, gcoef: l[8] < 2^22) puts at most 8 products < 2^58 into a column
//                (column 7; column 8 has 7 and two below 2^53), i.e. < 2^61; a carried column is < 2^29 (the last one, 16, keeps the rest:
//                < 2^516 / 2^464).  ZK_ZKEY_CARRY = 7 products between carries: 7 2^61 + 2^29 < 2^64 (an eighth fits only by the 2^37 that (2^29 - 1)^2
//                is short of 2^58, a ninth does not fit).
//                The reduction starts from carried columns and adds at most 9 products < 2^58 and a carry < 2^36 to each.  At most
//                ZK_ZKEY_GBLOCK = 56 products per reduction: value < 56 2^256 r / 2^261 + r = 2.75 r: fr29_to_fr_v<4>.
// Every block result is canonical; blocks, lanes and the two kinds of terms are joined with fr_add.
#pragma once
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/zkwg.h"
#include "zkwg_fq.h"
#include "zkwg_fr29.h"
#include "zkwg_r1cs.h"

#define ZK_ZKEY_BLOCK 64u          // unit terms per lane and reduction
#define ZK_ZKEY_CARRY 7u           // products between two carry propagations of the columns
#define ZK_ZKEY_GBLOCK 56u         // products per lane and reduction
#define ZK_ZKEY_MAX_ROW (1u << 20) // terms of one row (A or B) that creation accepts
#define ZK_ZKEY_LONG 63u           // constraints with more A + B terms than this are evaluated by a wavefront, the others by one lane each
                                   // (the length histogram of EmailVerifier(1024,1536))

struct ZkZkeyHeader {
  u64 off[11], size[11];
  u32 n_vars, n_public, domain, power;
};

// sections (ids 1 .. 10) of a "zkey" container
static inline bool zk_zkey_sections(const u8* z, u64 len, u64 (&off)[11], u64 (&size)[11]) {
  for (int i = 0; i < 11; ++i) off[i] = size[i] = 0;
  if (len < 12 || memcmp(z, "zkey", 4) != 0) return false;
  u32 version, nsec;
  memcpy(&version, z + 4, 4); memcpy(&nsec, z + 8, 4);
  if (version != 1) return false;
  u64 pos = 12;
  for (u32 i = 0; i < nsec; ++i) {
    if (len - pos < 12) return false;
    u32 id; u64 sz;
    memcpy(&id, z + pos, 4); memcpy(&sz, z + pos + 4, 8);
    pos += 12;
    if (sz > len - pos) return false;
    if (id >= 1 && id <= 10) { off[id] = pos; size[id] = sz; }
    pos += sz;
  }
  return true;
}
// header of a groth16 key over BN254; every size is checked before the bytes behind it are read, nPublic + 1 < nVars in 64 bits, and
// only then the sizes of sections 5 .. 9 that derive from them
static inline int zk_zkey_header(const u8* z, u64 len, ZkZkeyHeader& H) {
  if (!zk_zkey_sections(z, len, H.off, H.size)) return ZKWG_RC_BAD_CONFIG;
  for (int need : {1, 2, 4, 5, 6, 7, 8, 9}) if (!H.off[need]) return ZKWG_RC_BAD_CONFIG;
  if (H.size[1] < 4) return ZKWG_RC_BAD_CONFIG;
  u32 protocol;
  memcpy(&protocol, z + H.off[1], 4);
  if (protocol != 1) return ZKWG_RC_BAD_CONFIG;                     // groth16
  // n8q, q, n8r, r, nVars, nPublic, domainSize, alpha1, beta1, beta2, gamma2, delta1, delta2
  if (H.size[2] < 4 + 32 + 4 + 32 + 12 + 64 + 64 + 128 + 128 + 64 + 128) return ZKWG_RC_BAD_CONFIG;
  const u8* h = z + H.off[2];
  u32 n8q, n8r;
  memcpy(&n8q, h, 4); memcpy(&n8r, h + 36, 4);
  const Fq q = fq_p(); const Fr r = fr_p();
  if (n8q != 32 || n8r != 32 || memcmp(h + 4, q.l, 32) != 0 || memcmp(h + 40, r.l, 32) != 0) return ZKWG_RC_BAD_CONFIG;      // BN254
  memcpy(&H.n_vars, h + 72, 4); memcpy(&H.n_public, h + 76, 4); memcpy(&H.domain, h + 80, 4);
  if (H.domain == 0 || (H.domain & (H.domain - 1)) || (u64)H.n_public + 1 >= (u64)H.n_vars) return ZKWG_RC_BAD_CONFIG;
  H.power = 0;
  while ((1u << H.power) < H.domain) ++H.power;
  const u64 nv = H.n_vars, n_priv = nv - H.n_public - 1;
  if (H.size[5] != 64 * nv || H.size[6] != 64 * nv || H.size[7] != 128 * nv || H.size[8] != 64 * n_priv || H.size[9] != 64ull * H.domain) return ZKWG_RC_BAD_CONFIG;
  if (H.size[4] < 4) return ZKWG_RC_BAD_CONFIG;
  u32 n_coef;
  memcpy(&n_coef, z + H.off[4], 4);
  if (H.size[4] != 4 + 44ull * n_coef) return ZKWG_RC_BAD_CONFIG;
  return ZKWG_RC_OK;
}
// the key as the prover's plans take it (pointers into the file)
static inline void zk_zkey_key(const u8* z, const ZkZkeyHeader& H, zkwg_proving_key& key) {
  memset(&key, 0, sizeof key);
  key.n_wires = H.n_vars; key.n_public = H.n_public; key.log2_domain = H.power;
  key.a = z + H.off[5]; key.b1 = z + H.off[6]; key.b2 = z + H.off[7]; key.c = z + H.off[8]; key.h = z + H.off[9]; key.bases_on_device = 0;
  const u8* pts = z + H.off[2] + 84;
  memcpy(key.alpha1, pts, 64); memcpy(key.beta1, pts + 64, 64); memcpy(key.beta2, pts + 128, 128);
  memcpy(key.delta1, pts + 384, 64); memcpy(key.delta2, pts + 448, 128);                           // (gamma2 sits between beta2 and delta1)
}
// (matrix, row, wire) of every coefficient are in range; -> rows = largest row + 1
static inline int zk_zkey_coef_ranges(const u8* z, const ZkZkeyHeader& H, u64& n_rows) {
  u32 n_coef;
  memcpy(&n_coef, z + H.off[4], 4);
  const u8* cf = z + H.off[4] + 4;
  n_rows = 0;
  for (u32 i = 0; i < n_coef; ++i) {
    u32 m, row, wire;
    memcpy(&m, cf + 44ull * i, 4); memcpy(&row, cf + 44ull * i + 4, 4); memcpy(&wire, cf + 44ull * i + 8, 4);
    if (m > 1 || wire >= H.n_vars || row >= H.domain) return ZKWG_RC_BAD_CONFIG;
    n_rows = std::max<u64>(n_rows, (u64)row + 1);
  }
  return n_rows ? ZKWG_RC_OK : ZKWG_RC_BAD_CONFIG;
}
// the points at infinity (all zeros) of sections 6 and 7 sit at the same wires
static inline int zk_zkey_b_bitmaps(const u8* z, const ZkZkeyHeader& H) {
  const u8 *b1 = z + H.off[6], *b2 = z + H.off[7];
  for (u64 i = 0; i < H.n_vars; ++i) {
    u8 o1 = 0, o2 = 0;
    for (int k = 0; k < 64; ++k) o1 |= b1[64 * i + k];
    for (int k = 0; k < 128; ++k) o2 |= b2[128 * i + k];
    if ((o1 == 0) != (o2 == 0)) return ZKWG_RC_BAD_CONFIG;
  }
  return ZKWG_RC_OK;
}

struct ZkZkeyRow {
  u32 unit0, n_unit;   // words unit[unit0 .. unit0 + n_unit): wire | (coefficient == -1) << 31
  u32 gen0, n_gen;     // pairs gwire / gcoef [gen0 .. gen0 + n_gen)
};
struct ZkZkeyHost {
  u64 n_rows = 0;                  // constraints (rows of A resp. B), the public rows included
  std::vector<ZkZkeyRow> rows;     // 2 n_rows
  std::vector<u32> unit, gwire;
  std::vector<Fr> gcoef;
  std::vector<u32> order;          // the constraints by A + B terms, longest first; the first n_long of them are above ZK_ZKEY_LONG
  u32 n_long = 0;
  Fr k1;
};
struct ZkZkeyDev {
  const ZkZkeyRow* rows;
  const u32 *unit, *gwire;
  const Fr* gcoef;
  const u32* order;
  Fr29 k1;
  u64 n_rows;
  u32 n_long;
};
ZK_HD Fr zk_fr_times_32(Fr v) {
  for (int k = 0; k < 5; ++k) v = fr_add(v, v);
  return v;
}
static inline int zk_zkey_rows(const u8* z, const ZkZkeyHeader& H, ZkZkeyHost& T) {
  if (H.n_vars > 0x7fffffffu) return ZKWG_RC_BAD_CONFIG;           // (bit 31 of a unit word is the sign)
  int rc = zk_zkey_coef_ranges(z, H, T.n_rows);
  if (rc != ZKWG_RC_OK) return rc;
  u32 n_coef;
  memcpy(&n_coef, z + H.off[4], 4);
  const u8* cf = z + H.off[4] + 4;
  const Fr r = fr_p(), one = fr_R2(), minus_one = fr_neg(fr_R2());
  T.k1 = zk_fr_times_32(fr_R2());
  T.rows.assign(2 * T.n_rows, ZkZkeyRow{0, 0, 0, 0});
  std::vector<u8> kind(n_coef);
  for (u32 i = 0; i < n_coef; ++i) {
    u32 m, row;
    Fr v;
    memcpy(&m, cf + 44ull * i, 4); memcpy(&row, cf + 44ull * i + 4, 4); memcpy(v.l, cf + 44ull * i + 12, 32);
    if (fr_geq(v, r)) return ZKWG_RC_BAD_CONFIG;
    kind[i] = fr_eq(v, one) ? ZK_COEF_ONE : fr_eq(v, minus_one) ? ZK_COEF_MINUS_ONE : ZK_COEF_GENERIC;
    ZkZkeyRow& rw = T.rows[2ull * row + m];
    if (kind[i] == ZK_COEF_GENERIC) ++rw.n_gen; else ++rw.n_unit;
    if (rw.n_gen + rw.n_unit > ZK_ZKEY_MAX_ROW) return ZKWG_RC_BAD_CONFIG;
  }
  u32 pu = 0, pg = 0;
  for (ZkZkeyRow& rw : T.rows) { rw.unit0 = pu; rw.gen0 = pg; pu += rw.n_unit; pg += rw.n_gen; rw.n_unit = rw.n_gen = 0; }
  T.unit.resize(pu); T.gwire.resize(pg); T.gcoef.resize(pg);
  for (u32 i = 0; i < n_coef; ++i) {
    u32 m, row, wire;
    memcpy(&m, cf + 44ull * i, 4); memcpy(&row, cf + 44ull * i + 4, 4); memcpy(&wire, cf + 44ull * i + 8, 4);
    ZkZkeyRow& rw = T.rows[2ull * row + m];
    if (kind[i] == ZK_COEF_GENERIC) {
      Fr v;
      memcpy(v.l, cf + 44ull * i + 12, 32);
      T.gwire[rw.gen0 + rw.n_gen] = wire; T.gcoef[rw.gen0 + rw.n_gen] = zk_fr_times_32(v); ++rw.n_gen;
    } else {
      T.unit[rw.unit0 + rw.n_unit++] = wire | (kind[i] == ZK_COEF_MINUS_ONE ? 0x80000000u : 0u);
    }
  }
  auto len = [&](u32 j) { return (u64)T.rows[2ull * j].n_unit + T.rows[2ull * j].n_gen + T.rows[2ull * j + 1].n_unit + T.rows[2ull * j + 1].n_gen; };
  T.order.resize(T.n_rows);
  for (u64 j = 0; j < T.n_rows; ++j) T.order[j] = (u32)j;
  std::stable_sort(T.order.begin(), T.order.end(), [&](u32 a, u32 b) { return len(a) > len(b); });
  T.n_long = 0;
  while (T.n_long < T.n_rows && len(T.order[T.n_long]) > ZK_ZKEY_LONG) ++T.n_long;
  return ZKWG_RC_OK;
}
static inline ZkZkeyDev zk_zkey_view(const ZkZkeyHost& T) {
  return ZkZkeyDev{T.rows.data(), T.unit.data(), T.gwire.data(), T.gcoef.data(), T.order.data(), fr29_from_fr(T.k1), T.n_rows, T.n_long};
}

// `.wtns`: "wtns" | u32 version = 2 | u32 nSections | sections (u32 id, u64 size): 1 = u32 n8 (32), prime (r), u32 nWitness;
// 2 = nWitness values of 32 bytes, little-endian standard form.  Sections in either order.
static inline int zk_wtns_parse(const u8* p, u64 len, u64* n_witness, u64* values_offset) {
  if (!p || len < 12 || memcmp(p, "wtns", 4) != 0) return ZKWG_RC_BAD_CONFIG;
  u32 version, nsec;
  memcpy(&version, p + 4, 4); memcpy(&nsec, p + 8, 4);
  if (version != 2) return ZKWG_RC_BAD_CONFIG;
  u64 pos = 12, off[3] = {0, 0, 0}, size[3] = {0, 0, 0};
  for (u32 i = 0; i < nsec; ++i) {
    if (len - pos < 12) return ZKWG_RC_BAD_CONFIG;
    u32 id; u64 sz;
    memcpy(&id, p + pos, 4); memcpy(&sz, p + pos + 4, 8);
    pos += 12;
    if (sz > len - pos) return ZKWG_RC_BAD_CONFIG;
    if (id == 1 || id == 2) { off[id] = pos; size[id] = sz; }
    pos += sz;
  }
  if (!off[1] || !off[2] || size[1] != 40) return ZKWG_RC_BAD_CONFIG;
  u32 n8, nw;
  memcpy(&n8, p + off[1], 4);
  const Fr r = fr_p();
  if (n8 != 32 || memcmp(p + off[1] + 4, r.l, 32) != 0) return ZKWG_RC_BAD_CONFIG;
  memcpy(&nw, p + off[1] + 36, 4);
  if (size[2] != 32ull * nw) return ZKWG_RC_BAD_CONFIG;
  if (n_witness) *n_witness = nw;
  if (values_offset) *values_offset = off[2];
  return ZKWG_RC_OK;
}

// ---- the row evaluation (device and host) ---------------------------------------------------------------------------------------
// a 32-byte witness value as 8 words (p: 16-byte aligned on the device)
ZK_HD void zk_zkey_load(const u8* p, u32 (&x)[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4 lo = ((const uint4*)p)[0], hi = ((const uint4*)p)[1];
  x[0] = lo.x; x[1] = lo.y; x[2] = lo.z; x[3] = lo.w; x[4] = hi.x; x[5] = hi.y; x[6] = hi.z; x[7] = hi.w;
#else
  memcpy(x, p, 32);
#endif
}
ZK_HD Fr zk_zkey_words_fr(const u32 (&x)[8]) {
  return Fr{{x[0] | (u64)x[1] << 32, x[2] | (u64)x[3] << 32, x[4] | (u64)x[5] << 32, x[6] | (u64)x[7] << 32}};
}
// S = sum of +-x over at most ZK_ZKEY_BLOCK values < 2^256, as signed columns of 32-bit words  ->  S 2^256 mod r, canonical
ZK_HD Fr zk_zkey_fold(const long long (&S)[8], const Fr29& k1) {
  const u32 OFF[9] = {0x00000200u, 0xc3eb27e0u, 0x72e12287u, 0x67d090f3u, 0x02b0ba50u, 0xa08b6d03u, 0x63405370u, 0xc89ce5c2u, 0x60u};   // 512 r
  long long c = 0;
  u32 w[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    ZKR29_EXPECT(S[i] > -(1ll << 38) && S[i] < (1ll << 38));
    c += S[i] + (long long)OFF[i];
    w[i] = (u32)c;
    c >>= 32;                                        // (arithmetic: the columns are signed)
  }
  c += OFF[8];
  ZKR29_EXPECT(c >= 0 && c < 256);                   // 0 < S + 512 r < 2^264
  Fr29 a = fr29_from_fr(zk_zkey_words_fr(w));
  a.l[8] |= (u32)c << 24;
  return fr29_to_fr_v<8>(fr29_mul(a, k1));
}
struct ZkZkeyCols { u64 c[17]; };
ZK_HD void zk_zkey_cols_mac(ZkZkeyCols& C, const Fr29& x, const Fr29& k) {
#pragma unroll
  for (int i = 0; i < 9; ++i) {
#pragma unroll
    for (int j = 0; j < 9; ++j) {
#if !defined(__HIP_DEVICE_COMPILE__) && defined(ZKWG_FR29_CHECK)
      ZKR29_EXPECT((((unsigned __int128)C.c[i + j] + (unsigned __int128)x.l[i] * k.l[j]) >> 64) == 0);
#endif
      C.c[i + j] += (u64)x.l[i] * k.l[j];
    }
  }
}
ZK_HD void zk_zkey_cols_carry(ZkZkeyCols& C) {
  u64 c = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const u64 t = C.c[k] + c;
    ZKR29_EXPECT(t >= c);
    C.c[k] = t & ZK29_M;
    c = t >> 29;
  }
  C.c[16] += c;
  ZKR29_EXPECT(C.c[16] >= c);
}
// the columns of at most ZK_ZKEY_GBLOCK products  ->  their sum / 2^261 mod r, canonical
ZK_HD Fr zk_zkey_cols_reduce(ZkZkeyCols& C) {
  zk_zkey_cols_carry(C);
  u32 q[9];
  Fr29 r;
  u64 acc = 0;
#if !defined(__HIP_DEVICE_COMPILE__) && defined(ZKWG_FR29_CHECK)
  unsigned __int128 wide = 0;
#define ZK_ZKEY_WIDE(v) wide += (v)
#define ZK_ZKEY_WIDE_STEP() do { ZKR29_EXPECT((wide >> 64) == 0); wide >>= 29; } while (0)
#else
#define ZK_ZKEY_WIDE(v) do { } while (0)
#define ZK_ZKEY_WIDE_STEP() do { } while (0)
#endif
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    acc += C.c[k]; ZK_ZKEY_WIDE(C.c[k]);
#pragma unroll
    for (int i = 0; i < k; ++i) { acc += (u64)q[i] * ZKR29_P(k - i); ZK_ZKEY_WIDE((unsigned __int128)q[i] * ZKR29_P(k - i)); }
    q[k] = ((u32)acc * ZK29_N0) & ZK29_M;
    acc += (u64)q[k] * ZKR29_P(0); ZK_ZKEY_WIDE((unsigned __int128)q[k] * ZKR29_P(0));
    ZK_ZKEY_WIDE_STEP();
    acc >>= 29;
  }
#pragma unroll
  for (int k = 9; k < 17; ++k) {
    acc += C.c[k]; ZK_ZKEY_WIDE(C.c[k]);
#pragma unroll
    for (int i = k - 8; i < 9; ++i) { acc += (u64)q[i] * ZKR29_P(k - i); ZK_ZKEY_WIDE((unsigned __int128)q[i] * ZKR29_P(k - i)); }
    r.l[k - 9] = (u32)acc & ZK29_M;
    ZK_ZKEY_WIDE_STEP();
    acc >>= 29;
  }
  ZKR29_EXPECT(acc < (1ull << 32));
  r.l[8] = (u32)acc;
#undef ZK_ZKEY_WIDE
#undef ZK_ZKEY_WIDE_STEP
  return fr29_to_fr_v<4>(r);
}

// One lane's share of row `rw` -- its terms lane, lane + step, ... -- for G witnesses w[0 .. G): out[g] = that share of (row . w[g]) 2^256
// mod r, canonical.  A row's terms are read once for the G witnesses where they are +-1 (the gathers of the G values are independent loads),
// and once per witness where they carry a coefficient; a value 0 skips its product there.
template <int G>
ZK_HD void zk_zkey_row(const ZkZkeyDev& T, const ZkZkeyRow& rw, u32 lane, u32 step, const u8* const (&w)[G], Fr (&out)[G]) {
#pragma unroll
  for (int g = 0; g < G; ++g) out[g] = fr_zero();
  for (u32 t = lane; t < rw.n_unit;) {
    long long S[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
      for (int i = 0; i < 8; ++i) S[g][i] = 0;
    }
    for (u32 k = 0; k < ZK_ZKEY_BLOCK && t < rw.n_unit; ++k, t += step) {
      const u32 tw = T.unit[rw.unit0 + t];
      const bool neg = (tw >> 31) != 0;
      const u64 at = 32ull * (tw & 0x7fffffffu);
      u32 x[G][8];
#pragma unroll
      for (int g = 0; g < G; ++g) zk_zkey_load(w[g] + at, x[g]);
#pragma unroll
      for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int i = 0; i < 8; ++i) S[g][i] += neg ? -(long long)x[g][i] : (long long)x[g][i];
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) out[g] = fr_add(out[g], zk_zkey_fold(S[g], T.k1));
  }
  for (u32 t0 = lane; t0 < rw.n_gen; t0 += step * ZK_ZKEY_GBLOCK) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      ZkZkeyCols C;
#pragma unroll
      for (int i = 0; i < 17; ++i) C.c[i] = 0;
      u32 t = t0, pending = 0;
      for (u32 k = 0; k < ZK_ZKEY_GBLOCK && t < rw.n_gen; ++k, t += step) {
        u32 x[8];
        zk_zkey_load(w[g] + 32ull * T.gwire[rw.gen0 + t], x);
        if ((x[0] | x[1] | x[2] | x[3] | x[4] | x[5] | x[6] | x[7]) == 0) continue;
        zk_zkey_cols_mac(C, fr29_from_fr(zk_zkey_words_fr(x)), fr29_from_fr(T.gcoef[rw.gen0 + t]));
        if (++pending == ZK_ZKEY_CARRY) { zk_zkey_cols_carry(C); pending = 0; }
      }
      out[g] = fr_add(out[g], zk_zkey_cols_reduce(C));
    }
  }
}

// host mirror of zk_zkey_abc: n witnesses `stride` bytes apart -> per witness A.w | B.w | C.w (n_rows values each, Montgomery form),
// `abc_stride` bytes apart, through the same split as the kernels (one lane for a constraint up to ZK_ZKEY_LONG terms, 64 lanes above)
static inline void zk_zkey_abc_host(const ZkZkeyHost& H, const u8* wit, u64 stride, u64 n, u8* abc, u64 abc_stride) {
  const ZkZkeyDev T = zk_zkey_view(H);
  for (u64 e = 0; e < n; ++e) {
    const u8* const w[1] = {wit + e * stride};
    Fr* out = (Fr*)(abc + e * abc_stride);
    for (u64 o = 0; o < T.n_rows; ++o) {
      const u32 j = T.order[o];
      const u32 lanes = o < T.n_long ? 64u : 1u;
      Fr ab[2] = {fr_zero(), fr_zero()};
      for (u32 l = 0; l < lanes; ++l) {
        for (int m = 0; m < 2; ++m) {
          Fr part[1];
          zk_zkey_row<1>(T, T.rows[2ull * j + m], l, lanes, w, part);
          ab[m] = fr_add(ab[m], part[0]);
        }
      }
      out[j] = ab[0]; out[T.n_rows + j] = ab[1]; out[2 * T.n_rows + j] = fr_mont_mul(ab[0], ab[1]);
    }
  }
}
// values >= r among the n_vars values of one witness
static inline bool zk_zkey_range_host(const u8* wit, u64 n_vars) {
  for (u64 i = 0; i < n_vars; ++i) {
    Fr v;
    memcpy(v.l, wit + 32 * i, 32);
    if (fr_geq(v, fr_p())) return false;
  }
  return true;
}
