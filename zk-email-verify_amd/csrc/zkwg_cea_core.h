// CleanEmailAddress(L) -- utils/email.circom:16-140, the main of tests/test-circuits/clean-email-address-test.circom: proves that
// `decoded` is `encoded` without the periods of the local part and without the "+alias" in front of the '@'.
//
//   r = PoseidonModular(2 L)(encoded || decoded)          (utils/hash.circom:49-82): L / 8 x Poseidon(16), L / 8 - 1 x Poseidon(2)
//   rEnc / muxEnc[i].c[0], rDec, sumEnc, sumDec             four chains over powers of r
//   isValid = IsEqual()([sumEnc[L-1], sumDec[L-1]])         one inversion
//
// Two phases, plain functions that also compile for the host (tests/native/ceatest.cpp):
//   zk_cea_chunk_core  one (email, chunk): gathers the chunk's 16 elements from the two record slots and hashes them (zk_poseidon29<17>)
//   zk_cea_tail_core   one email: the merge chain (zk_poseidon29<3>), the flag scan over encoded[], the four chains, the inversion
// The byte-derived arrays (isPlusAndAt ... processed, the IsZero pairs of the IsEqual call sites) are not stored: zk_expand decodes them
// from the byte, the index of the first '+' and the index of the first '@' (zkwg_expand_dec.h ZkDecCea).
//
// THE LITERAL CIRCUIT.  The template has no assert and its flags are products, not booleans of the intended meaning:
//   afterPlus[i] = 1 while no '+' has occurred up to i, afterAt[i] likewise for '@'; hasAliasPart = 1 - afterPlus[L-1] is 1 whenever ANY
//   '+' occurs (also behind the '@'); inAliasPartTemp[i] = afterAt[i] - afterPlus[i] is r - 1 where an '@' comes before the first '+'.
// Hence shouldRemove[i] = isLocalPeriod[i] + inAliasPart[i] is -1, 0 or 1, processed[i] = (1 - shouldRemove[i]) encoded[i] is 0, the
// byte or TWICE the byte, and the Mux1 -- out = (c[1] - c[0]) s + c[0] for any s -- gives
//   rEnc[i] = c[0]            = rEnc[i-1] r          shouldRemove = 0
//   rEnc[i] = c[1]            = rEnc[i-1]            shouldRemove = 1
//   rEnc[i] = 2 c[0] - c[1]   = rEnc[i-1] (2 r - 1)  shouldRemove = -1      (rEnc[-1] = 1; c[0] = rEnc[i-1] r is kept whatever s is)
#pragma once
#include "zkwg_sched.h"
#include "zkwg_fr_inv.h"
#include "zkwg_poseidon29.h"

// element j (< 16) of chunk c of encoded || decoded: for L not a multiple of 16 the chunk L / 16 straddles the two record slots
ZK_HD u32 zk_cea_element(const ZkCeaLayout& E, const u8* rec, u32 c, u32 j) {
  const u32 k = 16u * c + j;
  return k < E.L ? rec[E.in_enc + k] : rec[E.in_dec + (k - E.L)];
}

// One chunk.  st: 17 state elements in limb form (element j, limb l at st[l * ls + j * js]); pos16: the Poseidon(16) table in limb
// form; stage / ss: the dense mixes' staging words of this unit (V & 4).  Writes the 612 S-box signals and the chunk's digest.
template <int V>
ZK_HD void zk_cea_chunk_core(const ZkCeaLayout& E, const u8* rec, Fr* frv, u32 c, u32* st, const u32 js, const u32 ls, const u32* pos16,
                        u32* stage, const size_t ss) {
  for (u32 l = 0; l < 9; ++l)
    for (u32 j = 0; j < 17; ++j) st[l * ls + j * js] = (l == 0 && j > 0) ? zk_cea_element(E, rec, c, j - 1) : 0u;
  frv[E.f_chunk + c] = zk_poseidon29<17, V>(st, js, ls, pos16, 68, frv + E.f_hash + zk_rs_chunk_off(c), stage, ss);
}

// the index of the first byte `ch` of encoded[], L if there is none
ZK_HD u32 zk_cea_first(const u8* enc, u32 L, u32 ch) {
  u32 p = L;
  for (u32 i = L; i-- > 0;) if (enc[i] == ch) p = i;
  return p;
}

// One email, after its chunks.  st: 3 state elements in limb form with strides js / ls; pos2: the Poseidon(2) table in limb form.
// Returns the status: 4 if the generic input path flagged an element that did not fit a byte (the record then does not hold the
// input), else 0 -- every byte input has a witness.
ZK_HD int zk_cea_tail_core(const ZkCeaLayout& E, u32 m_one, u32 range_flags_off, const u8* rec, Fr* frv, u32* small, u32* st, const u32 js,
                      const u32 ls, const u32* pos2) {
  const u32 L = E.L;
  const u8* enc = rec + E.in_enc;
  const u8* dec = rec + E.in_dec;
  // r: _out = Poseidon(2)([_out, chunk_hash]) over the chunk digests (utils/hash.circom:75-79)
  Fr r = frv[E.f_chunk];
  for (u32 c = 1; c < E.nch; ++c) {
    u32 a[9], b[9];
    zk_l29_from_fr(r, a);
    zk_l29_from_fr(frv[E.f_chunk + c], b);
    for (u32 l = 0; l < 9; ++l) { st[l * ls] = 0u; st[l * ls + js] = a[l]; st[l * ls + 2 * js] = b[l]; }
    r = zk_poseidon29<3, 2>(st, js, ls, pos2, 57, frv + E.f_hash + zk_rs_chunk_off(c) + ZK_P16_KEPT);
  }
  frv[E.f_chunk + E.nch] = r;
  // the flags are functions of the byte and of these two positions (header comment)
  const u32 P = zk_cea_first(enc, L, 43u), A = zk_cea_first(enc, L, 64u);
  small[m_one] = 1u;
  small[E.m_pos] = P; small[E.m_pos + 1] = A;
  const bool alias = P < L;                                            // hasAliasPart
  const Fr rm = fr_to_mont(r);
  Fr* mux = frv + E.f_mux;
  Fr rEnc = fr_from_u64(1), rDec = r, sumEnc = fr_zero(), sumDec = fr_zero();
  for (u32 i = 0; i < L; ++i) {
    const u32 b = enc[i];
    const int sr = (int)(i < P && i < A && b == 46u) + (alias ? (int)(i < A) - (int)(i < P) : 0);   // shouldRemove[i]
    const Fr c0 = i ? fr_mont_mul(rEnc, rm) : r;                       // muxEnc[i].c[0]
    if (sr == 0) rEnc = c0;
    else if (sr < 0) rEnc = fr_sub(fr_add(c0, c0), rEnc);              // (c[1] - c[0]) (-1) + c[0]
    if (i) mux[2 * i - 1] = c0;
    mux[2 * i] = rEnc;
    const u32 proc = (u32)(1 - sr) * b;                                // processed[i]: 0, the byte or twice the byte
    if (proc) sumEnc = fr_add(sumEnc, fr_mont_mul(rEnc, fr_to_mont(fr_from_u64(proc))));
    frv[E.f_sum_enc + i] = sumEnc;
    if (i) { rDec = fr_mont_mul(rDec, rm); frv[E.f_rdec + i - 1] = rDec; }
    const u32 d = dec[i];
    if (d) sumDec = fr_add(sumDec, fr_mont_mul(rDec, fr_to_mont(fr_from_u64(d))));
    frv[E.f_sum_dec + i] = sumDec;
  }
  // isValid <== IsEqual()([sumEnc[L-1], sumDec[L-1]]): isz.in = in[1] - in[0]; the hint's inverse is 0 for 0
  const Fr diff = fr_sub(sumDec, sumEnc);
  const bool valid = fr_is_zero(diff);
  small[E.m_valid] = valid ? 1u : 0u;
  frv[E.f_final] = fr_from_u64(valid ? 1 : 0);
  frv[E.f_final + 1] = fr_inv_by(diff);
  return *(const u32*)(rec + range_flags_off) != 0u ? 4 : 0;
}
