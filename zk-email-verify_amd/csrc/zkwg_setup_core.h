// The groth16 set-up `zKey.newZKey(r1cs, ptau)`: a compiler-format .r1cs and a PREPARED powers-of-tau file -> the .zkey the prover reads
// (reference workflow: docs/zk-email-docs/UsageGuide/README.md:145-180, "Step 6 ... generate the keys"; snarkjs src/zkey_new.js [EXT]).
// One header for the library (csrc/zkwg_setup_api.hip, csrc/zkwg_kernels_setup.hip) and for the host build of the CPU tests
// (tests/native/setuptest.cpp, ZKWG_FQ29_CHECK counting every violated limb-form bound).
//
//   zk_ptau_parse      the section walker of a "ptau" container, sizes checked before any read, -> the five slices of Lagrange-form points
//   zk_setup_plan      a wire-major CSR of one segmented sum  out[wire] = sum_t coef_t table[row_t]  and its work items
//   zk_setup_sum       one lane's share of a work item (device and host)
//   zk_setup_den / zk_setup_batch_inv / zk_setup_affine   accumulators -> canonical affine points, one inversion per ZK_SETUP_INV_BATCH
//   zk_setup_host      the whole set-up on the CPU through the functions above: the mirror the CPU tests compare with the oracle's key
//
// THE KEY (gamma = delta = 1: snarkjs' initial key, before contributions).  m constraints, n = 2^p the domain (smallest p >= 1 with
// 2^p >= m + nPublic + 1), L_j the Lagrange basis of the domain; the prepared file holds [L_j(tau)]_1, [L_j(tau)]_2, [alpha L_j(tau)]_1,
// [beta L_j(tau)]_1 for level p and [L_j(tau)]_1 for level p + 1:
//     A_i  (section 5) = sum_{(j, i, v) in A} v [L_j(tau)]_1, plus [L_{m + i}(tau)]_1 for i <= nPublic (the public rows the set-up appends)
//     B1_i (section 6) = sum_{(j, i, v) in B} v [L_j(tau)]_1            B2_i (section 7): the same over [L_j(tau)]_2
//     K_i = sum_A v [beta L_j(tau)]_1 + sum_B v [alpha L_j(tau)]_1 + sum_C v [L_j(tau)]_1   -> IC (section 3) for i <= nPublic, C (section 8) above
//     H_j  (section 9) = the entry 2 j + 1 of level p + 1 (a strided copy)
//
// THE SUMS.  Terms are grouped by wire.  A coefficient is brought to its least-magnitude signed form (v or r - v: the sign negates y of the
// base); magnitude 1 -- 64 % of the A and B terms of EmailVerifier(1024,1536), DESIGN.md section 23.1 -- is one mixed addition, any other
// magnitude a double-and-add from its top bit (bits - 1 doublings: k for 2^k, which most of the rest are) and one full addition.  The terms
// of a wire are sorted by the magnitude's bit length, the one-lane work items by their cost.  A wire of at most ZK_SETUP_LONG terms is one
// lane's (G2: one lane pair's) work; a longer one is cut into chunks of at most ZK_SETUP_CHUNK terms, one wavefront each (at most
// ZK_SETUP_CHUNK / 32 terms per lane, a reduction through LDS), and one wavefront joins the chunks of a wire (at most ZK_SETUP_MAX_WIRE /
// ZK_SETUP_CHUNK partial sums, so no lane walks an unbounded list; a wire with more terms is refused).
//
// ARITHMETIC: the lazy 29-bit limb formulas of zkwg_fq29.h / zkwg_ec29.h, bounds as stated there; accumulators are stored as Xyzz29
// (X [1, 11], Y [1, 7], ZZ, ZZZ [1, 2]).  The slices arrive in the zkey's form (canonical words, x 2^256) and are brought to the tables'
// form (x 2^261) by zk_setup_prepare_point, which also checks that the words are below q and the point is on its curve.
#pragma once
#include <string.h>
#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>
#include "../../include/zkwg.h"
#include "zkwg_ec29.h"
#include "zkwg_r1cs.h"

#define ZK_SETUP_LONG 64u             // wires with more terms than this are summed by wavefronts
#define ZK_SETUP_CHUNK 2048u          // terms of one wavefront's work item
#define ZK_SETUP_MAX_WIRE (1u << 27)  // terms of one wire in one sum: ZK_SETUP_MAX_WIRE / ZK_SETUP_CHUNK = 65,536 partial sums for the joining wavefront (<= 2,048 per lane)
#define ZK_SETUP_INV_BATCH 32u        // denominators per inversion
#define ZK_SETUP_MAX_POWER 28u        // the largest ceremony (and the row field of a term: 30 bits)

// ---- the "ptau" container [EXT: snarkjs src/powersoftau_utils.js, src/powersoftau_prepare_phase2.js; restated, not in the reference] -------
//   "ptau" | u32 version = 1 | u32 nSections | sections (u32 id, u64 size, payload)
//   1       u32 n8 (32), q, u32 power, u32 ceremonyPower
//   2 .. 6  tau^k G1 (2^(power + 1) - 1 points), tau^k G2, alpha tau^k G1, beta tau^k G1 (2^power each), beta G2
//   7       contributions
//   12 - 15 the Lagrange forms of 2 - 5: levels q = 0 .. power back to back (level q starts at point 2^q - 1); 12 has one level more
// Points: uncompressed, little-endian Montgomery words, x | y -- the zkey's form.
struct ZkPtauSection { u32 id; u32 point; u32 extra_level; };     // table of the point sections: bytes per point, levels beyond `power`
static const ZkPtauSection ZK_PTAU_LAGRANGE[4] = {{12, 64, 1}, {13, 128, 0}, {14, 64, 0}, {15, 64, 0}};
struct ZkPtauFile {
  u64 off[16], size[16];
  u32 power, ceremony_power;
};
static inline int zk_ptau_fail(std::string& err, const char* m) { err = m; return ZKWG_RC_BAD_CONFIG; }
// need_lagrange = false: the walk of an UNPREPARED file (zkwg_ptau_core.h); sections 12 - 15 are then recorded if present, not checked
static inline int zk_ptau_sections(const u8* p, u64 len, ZkPtauFile& F, std::string& err, bool need_lagrange = true) {
  for (int i = 0; i < 16; ++i) F.off[i] = F.size[i] = 0;
  if (!p || len < 12 || memcmp(p, "ptau", 4) != 0) return zk_ptau_fail(err, "not a .ptau file (magic)");
  u32 version, nsec;
  memcpy(&version, p + 4, 4); memcpy(&nsec, p + 8, 4);
  if (version != 1) return zk_ptau_fail(err, "unsupported .ptau version");
  u64 pos = 12;
  for (u32 i = 0; i < nsec; ++i) {
    if (len - pos < 12) return zk_ptau_fail(err, ".ptau: truncated section table");
    u32 id; u64 sz;
    memcpy(&id, p + pos, 4); memcpy(&sz, p + pos + 4, 8);
    pos += 12;
    if (sz > len - pos) return zk_ptau_fail(err, ".ptau: a section runs past the end of the file");
    if (id >= 1 && id < 16) { F.off[id] = pos; F.size[id] = sz; }
    pos += sz;
  }
  if (!F.off[1] || F.size[1] != 4 + 32 + 8) return zk_ptau_fail(err, ".ptau: header section missing or of the wrong size");
  u32 n8;
  memcpy(&n8, p + F.off[1], 4);
  const Fq q = fq_p();
  if (n8 != 32 || memcmp(p + F.off[1] + 4, q.l, 32) != 0) return zk_ptau_fail(err, ".ptau: the prime is not the BN254 base field");
  memcpy(&F.power, p + F.off[1] + 36, 4); memcpy(&F.ceremony_power, p + F.off[1] + 40, 4);
  if (F.power == 0 || F.power > ZK_SETUP_MAX_POWER) return zk_ptau_fail(err, ".ptau: power out of range");
  const u64 n = 1ull << F.power;
  const u64 want[7] = {0, 0, (2 * n - 1) * 64, n * 128, n * 64, n * 64, 128};
  for (int id = 2; id <= 6; ++id)
    if (!F.off[id] || F.size[id] != want[id]) return zk_ptau_fail(err, ".ptau: a point section (2 - 6) is missing or of the wrong size");
  if (!need_lagrange) return ZKWG_RC_OK;
  for (const ZkPtauSection& s : ZK_PTAU_LAGRANGE)
    if (!F.off[s.id]) return zk_ptau_fail(err, "Powers of tau is not prepared");
  for (const ZkPtauSection& s : ZK_PTAU_LAGRANGE)
    if (F.size[s.id] != ((2 * n - 1) + (s.extra_level ? 2 * n : 0)) * s.point) return zk_ptau_fail(err, ".ptau: a Lagrange section (12 - 15) is of the wrong size");
  return ZKWG_RC_OK;
}
// level `power` of sections 12 - 15 and level power + 1 of section 12, as pointers INTO the file
static inline int zk_ptau_parse(const u8* p, u64 len, u32 power, zkwg_setup_slices& S, std::string& err) {
  ZkPtauFile F;
  const int rc = zk_ptau_sections(p, len, F, err);
  if (rc != ZKWG_RC_OK) return rc;
  if (power == 0 || power > F.power) return zk_ptau_fail(err, ".ptau: the power of the file is too small for the circuit");
  memset(&S, 0, sizeof S);
  const u64 first = (1ull << power) - 1, next = (2ull << power) - 1;
  S.power = power; S.on_device = 0;
  S.tau_g1 = p + F.off[12] + first * 64; S.tau_g1_next = p + F.off[12] + next * 64;
  S.tau_g2 = p + F.off[13] + first * 128;
  S.alpha_tau_g1 = p + F.off[14] + first * 64; S.beta_tau_g1 = p + F.off[15] + first * 64;
  memcpy(S.alpha1, p + F.off[4], 64); memcpy(S.beta1, p + F.off[5], 64); memcpy(S.beta2, p + F.off[6], 128);
  return ZKWG_RC_OK;
}

// ---- the shape of the key ---------------------------------------------------------------------------------------------------------------
struct ZkSetupShape {
  u32 n_vars, n_public, m, power;
  u64 domain, n_coef, zkey_bytes;
};
static inline u32 zk_setup_domain_power(u64 m, u64 n_public) {
  u32 p = 1;
  while ((1ull << p) < m + n_public + 1) ++p;
  return p;
}
#define ZK_SETUP_HEADER_BYTES (4 + 32 + 4 + 32 + 12 + 64 + 64 + 128 + 128 + 64 + 128)
static inline int zk_setup_shape(const ZkR1csHost& R, ZkSetupShape& S, std::string& err) {
  S.n_vars = R.n_wires; S.m = R.n_constraints;
  const u64 n_public = (u64)R.n_pub_out + R.n_pub_in;
  if (n_public + 1 >= (u64)R.n_wires) return zk_ptau_fail(err, "the .r1cs has no private wire (nPublic + 1 >= nVars)");
  S.n_public = (u32)n_public;
  S.power = zk_setup_domain_power(S.m, n_public);
  if (S.power > ZK_SETUP_MAX_POWER) return zk_ptau_fail(err, "the .r1cs needs a domain above 2^28");
  S.domain = 1ull << S.power;
  S.n_coef = n_public + 1;
  for (u64 j = 0; j < S.m; ++j)
    for (u64 t = R.row_ptr[3 * j]; t < R.row_ptr[3 * j + 2]; ++t) if (!fr_is_zero(R.coef[t])) ++S.n_coef;
  if (S.n_coef > 0xffffffffull) return zk_ptau_fail(err, "too many coefficients for section 4");
  const u64 nv = S.n_vars;
  S.zkey_bytes = 12 + 10 * 12 + 4 + ZK_SETUP_HEADER_BYTES + 64 * (n_public + 1) + 4 + 44 * S.n_coef + 64 * nv + 64 * nv + 128 * nv + 64 * (nv - n_public - 1) + 64 * S.domain + 68;
  return ZKWG_RC_OK;
}
// the generators (Montgomery form): delta1 = G1's (1, 2), gamma2 = delta2 = the EIP-197 generator of G2 (oracle/pyref/bn254_g2.py)
static inline G1Affine zk_setup_g1_generator() { return G1Affine{fq_to_mont(Fq{{1, 0, 0, 0}}), fq_to_mont(Fq{{2, 0, 0, 0}})}; }
static inline G2Affine zk_setup_g2_generator() {
  const Fq x0{{0x46debd5cd992f6edULL, 0x674322d4f75edaddULL, 0x426a00665e5c4479ULL, 0x1800deef121f1e76ULL}};
  const Fq x1{{0x97e485b7aef312c2ULL, 0xf1aa493335a9e712ULL, 0x7260bfb731fb5d25ULL, 0x198e9393920d483aULL}};
  const Fq y0{{0x4ce6cc0166fa7daaULL, 0xe3d1e7690c43d37bULL, 0x4aab71808dcb408fULL, 0x12c85ea5db8c6debULL}};
  const Fq y1{{0x55acdadcd122975bULL, 0xbc4b313370b38ef3ULL, 0xec9e99ad690c3395ULL, 0x090689d0585ff075ULL}};
  return G2Affine{Fq2{fq_to_mont(x0), fq_to_mont(x1)}, Fq2{fq_to_mont(y0), fq_to_mont(y1)}};
}
// where the sections of the new file start (the order zkwg.zkey.write_zkey writes: 1 .. 10)
struct ZkSetupLayout { u64 off[11]; };
// writes the container, sections 1, 2, 4 and 10 and the section headers; the point sections (3, 5 - 9) are left for the sums
static inline void zk_setup_write_frame(const ZkR1csHost& R, const ZkSetupShape& S, const zkwg_setup_slices& sl, u8* z, ZkSetupLayout& L) {
  const u64 nv = S.n_vars, np1 = (u64)S.n_public + 1;
  const u64 size[11] = {0, 4, ZK_SETUP_HEADER_BYTES, 64 * np1, 4 + 44 * S.n_coef, 64 * nv, 64 * nv, 128 * nv, 64 * (nv - np1), 64 * S.domain, 68};
  memcpy(z, "zkey", 4);
  const u32 version = 1, nsec = 10;
  memcpy(z + 4, &version, 4); memcpy(z + 8, &nsec, 4);
  u64 pos = 12;
  for (u32 id = 1; id <= 10; ++id) {
    memcpy(z + pos, &id, 4); memcpy(z + pos + 4, &size[id], 8);
    pos += 12;
    L.off[id] = pos;
    pos += size[id];
  }
  const u32 protocol = 1, n8 = 32, domain = (u32)S.domain;
  memcpy(z + L.off[1], &protocol, 4);
  u8* h = z + L.off[2];
  const Fq q = fq_p(); const Fr r = fr_p();
  memcpy(h, &n8, 4); memcpy(h + 4, q.l, 32); memcpy(h + 36, &n8, 4); memcpy(h + 40, r.l, 32);
  memcpy(h + 72, &S.n_vars, 4); memcpy(h + 76, &S.n_public, 4); memcpy(h + 80, &domain, 4);
  const G1Affine g1 = zk_setup_g1_generator(); const G2Affine g2 = zk_setup_g2_generator();
  memcpy(h + 84, sl.alpha1, 64); memcpy(h + 148, sl.beta1, 64); memcpy(h + 212, sl.beta2, 128);
  memcpy(h + 340, &g2, 128); memcpy(h + 468, &g1, 64); memcpy(h + 532, &g2, 128);
  // section 4: the A and B coefficients times R^2 (R.coef is the coefficient times R), then the public rows
  u8* c = z + L.off[4];
  const u32 n_coef = (u32)S.n_coef;
  memcpy(c, &n_coef, 4);
  c += 4;
  for (u32 j = 0; j < S.m; ++j)
    for (u32 mtx = 0; mtx < 2; ++mtx)
      for (u64 t = R.row_ptr[3ull * j + mtx]; t < R.row_ptr[3ull * j + mtx + 1]; ++t) {
        if (fr_is_zero(R.coef[t])) continue;
        const Fr v = fr_to_mont(R.coef[t]);
        memcpy(c, &mtx, 4); memcpy(c + 4, &j, 4); memcpy(c + 8, &R.wire[t], 4); memcpy(c + 12, v.l, 32);
        c += 44;
      }
  const Fr one = fr_R2();
  for (u32 s = 0; s <= S.n_public; ++s) {
    const u32 mtx = 0, row = S.m + s;
    memcpy(c, &mtx, 4); memcpy(c + 4, &row, 4); memcpy(c + 8, &s, 4); memcpy(c + 12, one.l, 32);
    c += 44;
  }
  memset(z + L.off[10], 0, 68);          // csHash and the contribution count: not computed (`snarkjs zkey verify` wants them, no prover does)
}

// ---- the plan of one segmented sum -------------------------------------------------------------------------------------------------------
struct ZkSetupTerm { u32 src, coef; };       // src = row | table << 30; coef = (negative) << 31 | index of the magnitude (0: magnitude 1)
struct ZkSetupMag { Fr v; u32 bits, pad[3]; };   // |coefficient|, standard form, and its bit length (>= 2)
struct ZkSetupJob { u32 t0, n, out; };       // terms (or partial sums) [t0, t0 + n) -> accumulator / partial sum `out`
struct ZkSetupMags {
  std::vector<ZkSetupMag> mag;
  struct Hash { size_t operator()(const Fr& a) const { return (size_t)(a.l[0] * 0x9e3779b97f4a7c15ull ^ a.l[1] ^ (a.l[2] << 1) ^ (a.l[3] << 2)); } };
  struct Eq { bool operator()(const Fr& a, const Fr& b) const { return fr_eq(a, b); } };
  std::unordered_map<Fr, u32, Hash, Eq> index;
  ZkSetupMags() { mag.push_back(ZkSetupMag{fr_from_u64(1), 1, {0, 0, 0}}); }
  static u32 bit_length(const Fr& a) {
    for (int i = 3; i >= 0; --i) if (a.l[i]) return 64u * i + 64u - (u32)__builtin_clzll(a.l[i]);
    return 0;
  }
  // coefficient (Montgomery form, kind tag of zk_r1cs_parse) -> the coef word of a term; 0xffffffff for a zero coefficient
  u32 code(const Fr& coef_mont, u8 kind) {
    if (kind == ZK_COEF_ONE) return 0;
    if (kind == ZK_COEF_MINUS_ONE) return 0x80000000u;
    Fr v = fr_from_mont(coef_mont);
    if (fr_is_zero(v)) return 0xffffffffu;
    const Fr neg = fr_neg(v);
    const bool negative = !fr_geq(neg, v);         // r - v < v
    if (negative) v = neg;
    const u32 sign = negative ? 0x80000000u : 0u;
    auto it = index.find(v);
    if (it != index.end()) return sign | it->second;
    const u32 at = (u32)mag.size();
    mag.push_back(ZkSetupMag{v, bit_length(v), {0, 0, 0}});
    index.emplace(v, at);
    return sign | at;
  }
};
struct ZkSetupSource { int matrix; u32 table; bool public_rows; };      // matrix 0 / 1 / 2 = A / B / C of the .r1cs
struct ZkSetupPlan {
  std::vector<ZkSetupTerm> terms;
  std::vector<ZkSetupJob> shorts, chunks, joins;     // one lane each (by cost, largest first); one wavefront each
  std::vector<u32> seg_wire;                         // accumulator -> wire
  u32 n_part = 0;                                    // partial sums the chunks write
  u64 n_add = 0, n_dbl = 0, longest = 0;             // group operations of the sums (mixed + full additions, doublings), terms of the longest wire
};
// group operations of one term
static inline void zk_setup_term_cost(const ZkSetupMags& M, u32 coef, u64& add, u64& dbl) {
  const u32 mi = coef & 0x7fffffffu;
  if (mi == 0) { add += 1; return; }
  const ZkSetupMag& g = M.mag[mi];
  u32 pop = 0;
  for (int i = 0; i < 4; ++i) pop += (u32)__builtin_popcountll(g.v.l[i]);
  add += pop; dbl += g.bits - 1;            // pop - 1 mixed additions and the full addition into the accumulator
}
static inline int zk_setup_plan(const ZkR1csHost& R, const ZkSetupShape& S, const ZkSetupSource* src, int n_src, ZkSetupMags& M, ZkSetupPlan& P, std::string& err) {
  const u32 nv = S.n_vars;
  std::vector<u64> ptr((size_t)nv + 1, 0);
  auto each = [&](auto f) {
    for (int s = 0; s < n_src; ++s) {
      for (u32 j = 0; j < S.m; ++j)
        for (u64 t = R.row_ptr[3ull * j + src[s].matrix]; t < R.row_ptr[3ull * j + src[s].matrix + 1]; ++t) f(src[s], R.wire[t], j, t);
      if (src[s].public_rows) for (u32 w = 0; w <= S.n_public; ++w) f(src[s], w, S.m + w, ~0ull);
    }
  };
  std::vector<u32> codes;                      // (the magnitudes are looked up once)
  each([&](const ZkSetupSource&, u32 w, u32, u64 t) {
    const u32 c = t == ~0ull ? 0u : M.code(R.coef[t], R.kind[t]);
    codes.push_back(c);
    if (c != 0xffffffffu) ++ptr[w + 1];
  });
  for (u32 w = 0; w < nv; ++w) {
    if (ptr[w + 1] > ZK_SETUP_MAX_WIRE) return zk_ptau_fail(err, "a wire occurs in more terms than the set-up accepts");
    ptr[w + 1] += ptr[w];
  }
  if (ptr[nv] >= 0xffffffffull) return zk_ptau_fail(err, "too many terms");
  P.terms.resize(ptr[nv]);
  {
    std::vector<u64> at(ptr.begin(), ptr.end() - 1);
    size_t k = 0;
    each([&](const ZkSetupSource& s, u32 w, u32 row, u64) {
      const u32 c = codes[k++];
      if (c != 0xffffffffu) P.terms[at[w]++] = ZkSetupTerm{row | s.table << 30, c};
    });
  }
  auto bits = [&](const ZkSetupTerm& t) { return M.mag[t.coef & 0x7fffffffu].bits; };
  std::vector<u64> cost;
  for (u32 w = 0; w < nv; ++w) {
    const u64 n = ptr[w + 1] - ptr[w];
    if (!n) continue;
    std::stable_sort(P.terms.begin() + ptr[w], P.terms.begin() + ptr[w + 1], [&](const ZkSetupTerm& a, const ZkSetupTerm& b) { return bits(a) < bits(b); });
    u64 add = 0, dbl = 0;
    for (u64 t = ptr[w]; t < ptr[w + 1]; ++t) zk_setup_term_cost(M, P.terms[t].coef, add, dbl);
    P.n_add += add; P.n_dbl += dbl; P.longest = std::max(P.longest, n);
    const u32 seg = (u32)P.seg_wire.size();
    P.seg_wire.push_back(w);
    if (n <= ZK_SETUP_LONG) {
      P.shorts.push_back(ZkSetupJob{(u32)ptr[w], (u32)n, seg});
      cost.push_back(add + dbl);
    } else {
      const u32 p0 = P.n_part;
      for (u64 t = 0; t < n; t += ZK_SETUP_CHUNK) P.chunks.push_back(ZkSetupJob{(u32)(ptr[w] + t), (u32)std::min<u64>(ZK_SETUP_CHUNK, n - t), P.n_part++});
      P.joins.push_back(ZkSetupJob{p0, P.n_part - p0, seg});
      P.n_add += P.n_part - p0 + 63;
    }
  }
  std::vector<u32> order(P.shorts.size());
  for (u32 i = 0; i < order.size(); ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](u32 a, u32 b) { return cost[a] > cost[b]; });
  std::vector<ZkSetupJob> sorted(P.shorts.size());
  for (u32 i = 0; i < order.size(); ++i) sorted[i] = P.shorts[order[i]];
  P.shorts.swap(sorted);
  return ZKWG_RC_OK;
}
// the four sums of a key: A, B1, B2 (B's plan serves both), K
static const ZkSetupSource ZK_SETUP_SRC_A[1] = {{0, 0, true}};
static const ZkSetupSource ZK_SETUP_SRC_B[1] = {{1, 0, false}};
static const ZkSetupSource ZK_SETUP_SRC_K[3] = {{0, 1, true}, {1, 2, false}, {2, 0, false}};      // tables of K: 0 = tau, 1 = beta tau, 2 = alpha tau

// ---- the sums (device and host) -------------------------------------------------------------------------------------------------------
struct ZkSetupDev {
  const ZkSetupTerm* terms;
  const ZkSetupMag* mag;
};
template <class C> struct ZkSetupTab { const typename C::Affine *t0, *t1, *t2; };        // bases in the tables' form (x 2^261)

// v P for an affine P and a magnitude v of `bits` >= 2 bits: from the top bit, bits - 1 doublings and a mixed addition per further set bit
template <class C>
ZK_HD Xyzz29<typename C::F> zk_setup_mul(const Aff29<typename C::F>& P, const ZkSetupMag& g) {
  typedef typename C::F F;
  Xyzz29<F> acc = ec29_from_affine<F>(P);
  for (int i = (int)g.bits - 2; i >= 0; --i) {
    acc = ec29_dbl<F>(acc);
    if ((g.v.l[i >> 6] >> (i & 63)) & 1ull) acc = ec29_add_mixed<F>(acc, P);
  }
  return acc;
}
// one lane's share of the terms [t0, t0 + n): the terms lane, lane + step, ...
template <class C>
ZK_HD Xyzz29<typename C::F> zk_setup_sum(const ZkSetupDev& T, const ZkSetupTab<C>& tab, u32 t0, u32 n, u32 lane, u32 step, u32 h) {
  typedef typename C::F F;
  Xyzz29<F> acc = ec29_inf<F>();
  for (u32 t = lane; t < n; t += step) {
    const ZkSetupTerm tm = T.terms[t0 + t];
    const u32 sel = tm.src >> 30, mi = tm.coef & 0x7fffffffu;
    const typename C::Affine* base = (sel == 0 ? tab.t0 : sel == 1 ? tab.t1 : tab.t2) + (tm.src & 0x3fffffffu);
    const Aff29<F> P = C::load(base, h, (tm.coef >> 31) != 0);
    if (mi == 0) acc = ec29_add_mixed<F>(acc, P);
    else if (!P.inf) acc = ec29_add<F>(acc, zk_setup_mul<C>(P, T.mag[mi]));
  }
  return acc;
}
// one lane's share of the partial sums [t0, t0 + n)
template <class C>
ZK_HD Xyzz29<typename C::F> zk_setup_join(const Xyzz29<typename C::F>* part, u32 t0, u32 n, u32 lane, u32 step, u32 h) {
  typedef typename C::F F;
  Xyzz29<F> acc = ec29_inf<F>();
  for (u32 t = lane; t < n; t += step) acc = ec29_add<F>(acc, part[(u64)(t0 + t) * C::LANES + h]);
  return acc;
}

// one plan's launch series over device memory (csrc/zkwg_kernels_setup.hip): acc / part hold n_seg / n_part accumulators of 144 (G1) or
// 288 (G2) bytes, den / pref n_seg values, out the n_vars points of the section (zeroed by the caller)
struct ZkSetupRun {
  ZkSetupDev T;
  const void *t0, *t1, *t2;
  const ZkSetupJob *shorts, *chunks, *joins;
  u32 n_short, n_chunk, n_join, n_seg;
  const u32* seg_wire;
  void *acc, *part;
  Fq29 *den, *pref;
  void* out;
};

// ---- a slice point: the zkey's form -> the tables' form, words below q, on the curve ----------------------------------------------------
ZK_HD Fq29 zk_setup_b_g1() { return Fq29{{0x00766463u, 0x1c54760au, 0x08f6927au, 0x03e40c4du, 0x1fea4f2bu, 0x17c6c26au, 0x157fe417u, 0x0f8056f9u, 0x002958a2u}}; }   // 3 x 2^261 mod q
ZK_HD Fq29 zk_setup_b_g2_c0() { return Fq29{{0x0b489658u, 0x00cfd255u, 0x0fdb9a77u, 0x02ce89f7u, 0x0033a0d4u, 0x1a768545u, 0x06ee3ddcu, 0x106a7dc1u, 0x0019316bu}}; }   // 3 / (9 + i), x 2^261
ZK_HD Fq29 zk_setup_b_g2_c1() { return Fq29{{0x1b9fece0u, 0x07ecccd1u, 0x1069f1c7u, 0x0cdf64f3u, 0x0154cbe1u, 0x0dd22ac0u, 0x06eba4e8u, 0x1929a235u, 0x00283739u}}; }
ZK_HD Fq29 zk_setup_curve_b(ZkEcG1) { return zk_setup_b_g1(); }
// y^2 == x^3 + b for a point in limb form (x [1, 1], y [1, 1])
template <class C>
ZK_HD bool zk_setup_on_curve(const typename C::F::E& x, const typename C::F::E& y) {
  typedef typename C::F F;
  ZKQ29_ASSUME(x, 1, 1); ZKQ29_ASSUME(y, 1, 1);          // relies on: every caller passes words out of zk_fq_r256_to_r261, whose fq29_to_fq<2> reduces below q
  const typename F::E y2 = F::template sqr<1>(y);                                       // [1, 2]
  const typename F::E x3 = F::template mul<1>(F::template sqr<1>(x), x);                // [1, 2]
  const typename F::E rhs = F::add(x3, zk_setup_curve_b(C()));                          // [2, 3]
  return F::template is_zero_mod<6>(F::template sub<4, 2>(y2, rhs));                    // value < 2 q + 4 q
}
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ Fq29 zk_setup_curve_b(ZkEcG2) { return ZkF2::odd() ? zk_setup_b_g2_c1() : zk_setup_b_g2_c0(); }
__device__ __forceinline__ bool zk_setup_both(ZkEcG1, bool mine) { return mine; }
__device__ __forceinline__ bool zk_setup_both(ZkEcG2, bool mine) { return ZkF2::both(mine); }
// half h of point i: in -> out (out may be null: check only); false: a word >= q or the point is not on the curve
template <class C>
__device__ __forceinline__ bool zk_setup_prepare_point(const typename C::Affine* in, typename C::Affine* out, u64 i, u32 h) {
  const Fq* w = (const Fq*)(in + i);                        // G1: x | y; G2: x.c0 | x.c1 | y.c0 | y.c1
  const Fq x = zk_ld_fq(w + h), y = zk_ld_fq(w + C::LANES + h);
  const bool inf = zk_setup_both(C(), fq_is_zero(x) && fq_is_zero(y));
  const bool small = !fq_geq(x, fq_p()) && !fq_geq(y, fq_p());
  const Fq tx = zk_fq_r256_to_r261(x), ty = zk_fq_r256_to_r261(y);
  if (out) { Fq* o = (Fq*)(out + i); o[h] = tx; o[C::LANES + h] = ty; }
  const bool on = zk_setup_on_curve<C>(fq29_from_fq(tx), fq29_from_fq(ty));
  return zk_setup_both(C(), small) && (inf || on);
}
#else
static inline Fq29x2 zk_setup_curve_b(ZkEcG2) { return Fq29x2{{zk_setup_b_g2_c0(), zk_setup_b_g2_c1()}}; }
static inline bool zk_setup_prepare_point_g1(const G1Affine* in, G1Affine* out, u64 i) {
  const G1Affine p = in[i];
  const bool small = !fq_geq(p.x, fq_p()) && !fq_geq(p.y, fq_p());
  const G1Affine t = zk_g1_to_table_form(p);
  if (out) out[i] = t;
  return small && (g1_is_inf(p) || zk_setup_on_curve<ZkEcG1>(fq29_from_fq(t.x), fq29_from_fq(t.y)));
}
static inline bool zk_setup_prepare_point_g2(const G2Affine* in, G2Affine* out, u64 i) {
  const G2Affine p = in[i];
  const bool small = !fq_geq(p.x.c0, fq_p()) && !fq_geq(p.x.c1, fq_p()) && !fq_geq(p.y.c0, fq_p()) && !fq_geq(p.y.c1, fq_p());
  const G2Affine t = zk_g2_to_table_form(p);
  if (out) out[i] = t;
  return small && (g2_is_inf(p) || zk_setup_on_curve<ZkEcG2>(Fq29x2{{fq29_from_fq(t.x.c0), fq29_from_fq(t.x.c1)}}, Fq29x2{{fq29_from_fq(t.y.c0), fq29_from_fq(t.y.c1)}}));
}
#endif

// ---- accumulators -> canonical affine points ---------------------------------------------------------------------------------------------
// x = X / ZZ, y = Y / ZZZ from ONE inverse per point: 1 / ZZZ, and 1 / ZZ = (ZZ / ZZZ)^2 (ZZ^3 = ZZZ^2).  G2's ZZZ = a + b i is inverted
// through its norm a^2 + b^2 in Fq, so both groups share the batched inversion of Fq values.
// the value to invert (1 for the point at infinity): [1, 4]
ZK_HD Fq29 zk_setup_den(ZkEcG1, const Xyzz29<ZkF1>& p) { return ec29_is_inf<ZkF1>(p) ? fq29_one() : p.zzz; }
// 1 / ZZZ from the inverse of the value above: [1, 3]
ZK_HD Fq29 zk_setup_iz3(ZkEcG1, const Fq29& zzz, const Fq29& dinv) { return dinv; }
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ Fq29 zk_setup_den(ZkEcG2, const Xyzz29<ZkF2>& p) {
  if (ec29_is_inf<ZkF2>(p)) return fq29_one();
  const Fq29 s = fq29_sqr(p.zzz);                                                       // this half squared: [1, 2]
  return fq29_norm(fq29_add(s, zk_pair_xchg(s)));
}
__device__ __forceinline__ Fq29 zk_setup_iz3(ZkEcG2, const Fq29& zzz, const Fq29& dinv) {
  const Fq29 t = fq29_mul(zzz, dinv);                                                   // [1, 2]
  const Fq29 n = fq29_norm(fq29_neg<3, 1>(t));                                          // the conjugate's odd half
  Fq29 r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = ZkF2::odd() ? n.l[i] : t.l[i];
  return r;
}
#else
static inline Fq29 zk_setup_den(ZkEcG2, const Xyzz29<ZkF2>& p) {
  if (ec29_is_inf<ZkF2>(p)) return fq29_one();
  return fq29_norm(fq29_add(fq29_sqr(p.zzz.c[0]), fq29_sqr(p.zzz.c[1])));
}
static inline Fq29x2 zk_setup_iz3(ZkEcG2, const Fq29x2& zzz, const Fq29& dinv) {
  return Fq29x2{{fq29_mul(zzz.c[0], dinv), fq29_norm(fq29_neg<3, 1>(fq29_mul(zzz.c[1], dinv)))}};
}
#endif
// (what a kernel calls: one name for both compile passes)
template <class C> ZK_HD Fq29 zk_setup_den_of(const Xyzz29<typename C::F>& p) { return zk_setup_den(C(), p); }
template <class C> ZK_HD bool zk_setup_prepare_half(const typename C::Affine* in, typename C::Affine* out, u64 i, u32 h) {
#if defined(__HIP_DEVICE_COMPILE__)
  return zk_setup_prepare_point<C>(in, out, i, h);
#else
  return false;          // (the host mirror calls zk_setup_prepare_point_g1 / _g2)
#endif
}
// a^(q - 2) for a = [1, <= 4], a != 0: [1, 2]
ZK_HD Fq29 zk_setup_fq29_inv(const Fq29& a) {
  Fq29 r = a;
  for (int i = 252; i >= 0; --i) {             // (bit 253 is the top bit of q - 2)
    const u64 e = i >= 192 ? ZK_Q3 : i >= 128 ? ZK_Q2 : i >= 64 ? ZK_Q1 : ZK_Q0 - 2;       // (selects, not a table: a lane's private array would live in scratch)
    r = fq29_sqr(r);
    if ((e >> (i & 63)) & 1ull) r = fq29_mul(r, a);
  }
  return r;
}
// lane `lane` of n_lanes inverts the values d[lane + k n_lanes], k < ZK_SETUP_INV_BATCH, in place (none of them 0); pref: n values of room
ZK_HD void zk_setup_batch_inv(Fq29* d, Fq29* pref, u64 n, u64 lane, u64 n_lanes) {
  if (lane >= n) return;
  Fq29 run = d[lane];
  u32 cnt = 1;
  for (u64 i = lane + n_lanes; i < n && cnt < ZK_SETUP_INV_BATCH; i += n_lanes, ++cnt) {
    pref[i] = run;                               // the product of the values before i
    run = fq29_mul(run, d[i]);
  }
  Fq29 inv = zk_setup_fq29_inv(run);
  for (u32 k = cnt; k-- > 1;) {
    const u64 i = lane + (u64)k * n_lanes;
    const Fq29 v = d[i];
    d[i] = fq29_mul(inv, pref[i]);
    inv = fq29_mul(inv, v);
  }
  d[lane] = inv;
}
ZK_HD Fq zk_setup_out_fq(const Fq29& v) { return fq29_to_fq<2>(fq29_mul(v, fq29_r256())); }
#if !defined(__HIP_DEVICE_COMPILE__)
static inline void zk_setup_put(G1Affine* out, const Fq29& x, const Fq29& y) { *out = G1Affine{zk_setup_out_fq(x), zk_setup_out_fq(y)}; }
static inline void zk_setup_put(G2Affine* out, const Fq29x2& x, const Fq29x2& y) {
  *out = G2Affine{Fq2{zk_setup_out_fq(x.c[0]), zk_setup_out_fq(x.c[1])}, Fq2{zk_setup_out_fq(y.c[0]), zk_setup_out_fq(y.c[1])}};
}
#endif
// accumulator + the inverse of its denominator -> the affine point, canonical words in the zkey's form; zeros for infinity
template <class C>
ZK_HD void zk_setup_affine(const Xyzz29<typename C::F>& p, const Fq29& dinv, typename C::Affine* out, u32 h) {
  typedef typename C::F F;
  typedef typename F::E E;
  const bool inf = ec29_is_inf<F>(p);
  const E iz3 = zk_setup_iz3(C(), p.zzz, dinv);                   // [1, 3]
  const E iz2 = F::template sqr<2>(F::template mul<2>(iz3, p.zz));
  const E x = F::template mul<2>(p.x, iz2), y = F::template mul<3>(p.y, iz3);
#if defined(__HIP_DEVICE_COMPILE__)
  Fq* w = (Fq*)out;
  w[h] = inf ? fq_zero() : zk_setup_out_fq(x); w[C::LANES + h] = inf ? fq_zero() : zk_setup_out_fq(y);
#else
  if (inf) { memset(out, 0, sizeof *out); return; }
  zk_setup_put(out, x, y);
#endif
}
#if !defined(__HIP_DEVICE_COMPILE__)

// ---- the host mirror ------------------------------------------------------------------------------------------------------------------------
// one plan over tables in the tables' form -> out[wire] (n_vars points, zeros where a wire has no term), through the work items the kernels run
template <class C>
static inline void zk_setup_run_host(const ZkSetupPlan& P, const ZkSetupMags& M, const ZkSetupTab<C>& tab, u32 n_vars, typename C::Affine* out) {
  typedef typename C::F F;
  const ZkSetupDev T{P.terms.data(), M.mag.data()};
  const u32 per = 64u / C::DEV_LANES;
  memset((void*)out, 0, sizeof(typename C::Affine) * (size_t)n_vars);
  std::vector<Xyzz29<F>> acc(P.seg_wire.size()), part(P.n_part);
  for (const ZkSetupJob& j : P.shorts) acc[j.out] = zk_setup_sum<C>(T, tab, j.t0, j.n, 0, 1, 0);
  for (const ZkSetupJob& j : P.chunks) {
    Xyzz29<F> s = ec29_inf<F>();
    for (u32 l = 0; l < per; ++l) s = ec29_add<F>(s, zk_setup_sum<C>(T, tab, j.t0, j.n, l, per, 0));
    part[j.out] = s;
  }
  for (const ZkSetupJob& j : P.joins) {
    Xyzz29<F> s = ec29_inf<F>();
    for (u32 l = 0; l < per; ++l) s = ec29_add<F>(s, zk_setup_join<C>(part.data(), j.t0, j.n, l, per, 0));
    acc[j.out] = s;
  }
  const u64 n = acc.size(), n_lanes = (n + ZK_SETUP_INV_BATCH - 1) / ZK_SETUP_INV_BATCH;
  std::vector<Fq29> den(n), pref(n);
  for (u64 i = 0; i < n; ++i) den[i] = zk_setup_den(C(), acc[i]);
  for (u64 l = 0; l < n_lanes; ++l) zk_setup_batch_inv(den.data(), pref.data(), n, l, n_lanes);
  for (u64 i = 0; i < n; ++i) zk_setup_affine<C>(acc[i], den[i], out + P.seg_wire[i], 0);
}
// the whole set-up on the CPU; slices: host pointers.  info (may be null): {terms of A, B, K, distinct magnitudes, chunks of A, B, K}
static inline int zk_setup_host(const u8* r1cs, u64 len, const zkwg_setup_slices& sl, u8* out, u64 cap, u64* out_len, u64* info, std::string& err) {
  ZkR1csHost R;
  if (!zk_r1cs_parse(r1cs, len, R)) return zk_ptau_fail(err, R.err.c_str());
  ZkSetupShape S;
  int rc = zk_setup_shape(R, S, err);
  if (rc != ZKWG_RC_OK) return rc;
  if (sl.power != S.power) return zk_ptau_fail(err, "the slices are not of the circuit's domain");
  if (cap < S.zkey_bytes) return ZKWG_RC_BAD_ARG;
  const u64 n = S.domain;
  std::vector<G1Affine> t1(n), ta(n), tb(n);
  std::vector<G2Affine> t2(n);
  bool ok = true;
  for (u64 i = 0; i < n; ++i) {
    ok &= zk_setup_prepare_point_g1((const G1Affine*)sl.tau_g1, t1.data(), i) && zk_setup_prepare_point_g1((const G1Affine*)sl.alpha_tau_g1, ta.data(), i) &&
          zk_setup_prepare_point_g1((const G1Affine*)sl.beta_tau_g1, tb.data(), i) && zk_setup_prepare_point_g2((const G2Affine*)sl.tau_g2, t2.data(), i);
  }
  for (u64 i = 0; i < 2 * n; ++i) ok &= zk_setup_prepare_point_g1((const G1Affine*)sl.tau_g1_next, nullptr, i);
  if (!ok) return zk_ptau_fail(err, "a point of the powers of tau is not on its curve");
  ZkSetupLayout L;
  zk_setup_write_frame(R, S, sl, out, L);
  ZkSetupMags M;
  ZkSetupPlan pa, pb, pk;
  if ((rc = zk_setup_plan(R, S, ZK_SETUP_SRC_A, 1, M, pa, err)) != ZKWG_RC_OK) return rc;
  if ((rc = zk_setup_plan(R, S, ZK_SETUP_SRC_B, 1, M, pb, err)) != ZKWG_RC_OK) return rc;
  if ((rc = zk_setup_plan(R, S, ZK_SETUP_SRC_K, 3, M, pk, err)) != ZKWG_RC_OK) return rc;
  std::vector<G1Affine> g1(S.n_vars);
  std::vector<G2Affine> g2(S.n_vars);
  zk_setup_run_host<ZkEcG1>(pa, M, ZkSetupTab<ZkEcG1>{t1.data(), nullptr, nullptr}, S.n_vars, g1.data());
  memcpy(out + L.off[5], g1.data(), 64ull * S.n_vars);
  zk_setup_run_host<ZkEcG1>(pb, M, ZkSetupTab<ZkEcG1>{t1.data(), nullptr, nullptr}, S.n_vars, g1.data());
  memcpy(out + L.off[6], g1.data(), 64ull * S.n_vars);
  zk_setup_run_host<ZkEcG2>(pb, M, ZkSetupTab<ZkEcG2>{t2.data(), nullptr, nullptr}, S.n_vars, g2.data());
  memcpy(out + L.off[7], g2.data(), 128ull * S.n_vars);
  zk_setup_run_host<ZkEcG1>(pk, M, ZkSetupTab<ZkEcG1>{t1.data(), tb.data(), ta.data()}, S.n_vars, g1.data());
  memcpy(out + L.off[3], g1.data(), 64ull * (S.n_public + 1));
  memcpy(out + L.off[8], g1.data() + S.n_public + 1, 64ull * (S.n_vars - S.n_public - 1));
  for (u64 j = 0; j < n; ++j) memcpy(out + L.off[9] + 64 * j, (const u8*)sl.tau_g1_next + 64 * (2 * j + 1), 64);
  if (out_len) *out_len = S.zkey_bytes;
  if (info) { info[0] = pa.terms.size(); info[1] = pb.terms.size(); info[2] = pk.terms.size(); info[3] = M.mag.size(); info[4] = pa.chunks.size(); info[5] = pb.chunks.size(); info[6] = pk.chunks.size(); }
  return ZKWG_RC_OK;
}
#endif
