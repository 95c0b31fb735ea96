// DKIM verification of raw emails -- the cores: body canonicalisation, SHA-256 of a byte stream and the RSA check of one
// (email, key) pair.  Restates packages/helpers/src/lib/mailauth/body/relaxed.ts:113-155,157-266 and body/simple.ts:59-106 as a per-byte
// emission rule, and the verification of dkim-verifier.ts:245-312 (rsa-sha256 only).
//
// Three builds of this header: the gfx950 kernels (csrc/zkwg_kernels_dkim.hip), the host path of the C-ABI (device = -1, the serial
// functions below and csrc/zkwg_dkim_host.h) and the CPU tests, which run the wavefront functions on a simulated wavefront
// (tests/native/dkimtest.cpp with ZKWG_WAVESIM).
//
// The emission rule.  Every raw body byte c emits 0, 1 or 2 bytes, looking at the byte before it and the byte after it only:
//   relaxed   LF -> CR LF | CR directly before LF -> nothing | SP, TAB -> nothing | any other c -> SP c when the byte before is SP or
//             TAB, else c.  A CR that is not followed by LF is such an "other" byte.
//   simple    c -> c
// A byte is CONTENT when it is an "other" byte (relaxed) or neither CR nor LF (simple).  The canonical body is the emitted stream cut
// after the last byte a content byte emitted, plus CR LF when there was a content byte (simple: always plus CR LF); l= then cuts it.
// What a stream has emitted after its last content byte so far is PENDING: it is written only when a later content byte shows up, so
// nothing beyond the canonical length is ever stored.
#pragma once
#include "zkwg_rsa_core.h"

#define ZK_DKIM_RELAXED 0u
#define ZK_DKIM_SIMPLE 1u
#define ZK_DKIM_NONE 256u                             // "no byte" before the first / after the last one
#define ZK_DKIM_LANE_BYTES 16u
#define ZK_DKIM_TILE (64u * ZK_DKIM_LANE_BYTES)      // raw bytes a wavefront takes per step
#define ZK_DKIM_STAGE (2u * ZK_DKIM_TILE)            // what they can emit
#define ZK_DKIM_MAX_RAW 0x7ffffff0u                  // a longer body is refused (32-bit output offsets)

// what the kernels know of one email (the host parser's result); 80 bytes
struct ZkDkimRec {
  u64 raw_off;        // its raw body in the uploaded buffer (16-byte aligned)
  u64 l;              // l=, when has_l
  u32 raw_len, body_mode, has_l;
  int pre_status;     // the parser's status: not 0 = nothing more is computed for this email
  u32 key_first, key_count;
  u32 pad[2];
  u8 bh[32];          // bh= decoded
};
struct ZkDkimKey {    // = zkwg_dkim_key (include/zkwg.h)
  u8 modulus_be[256];
  u32 bits, exponent;
};
// enum zkwg_dkim_status (include/zkwg.h)
#define ZK_DKIM_ST_NO_KEY 103
#define ZK_DKIM_ST_BODY_HASH 104
#define ZK_DKIM_ST_BAD_SIGNATURE 105
#define ZK_DKIM_ST_UNSUPPORTED 106
#define ZK_DKIM_ST_DOES_NOT_FIT 107
ZK_HD bool zk_dkim_key_usable(u32 bits, u32 exponent) { return bits <= 2048u && exponent == 65537u; }

struct ZkDkimEmit {
  u32 n;          // emitted bytes
  u32 b0, b1;
  bool content;
};
ZK_HD ZkDkimEmit zk_dkim_emit(u32 mode, u32 prev, u32 c, u32 next) {
  if (mode == ZK_DKIM_SIMPLE) return ZkDkimEmit{1u, c, 0u, c != 13u && c != 10u};
  if (c == 10u) return ZkDkimEmit{2u, 13u, 10u, false};
  if ((c == 13u && next == 10u) || c == 32u || c == 9u) return ZkDkimEmit{0u, 0u, 0u, false};
  if (prev == 32u || prev == 9u) return ZkDkimEmit{2u, 32u, c, true};
  return ZkDkimEmit{1u, c, 0u, true};
}
// byte k of a pending run that ends right before raw position `at`
ZK_HD u32 zk_dkim_pending_byte(u32 mode, const u8* raw, u32 at, u32 pend, u32 k) {
  return mode == ZK_DKIM_SIMPLE ? raw[at - pend + k] : ((k & 1u) ? 10u : 13u);
}
// where the stores stop, and when the rest of the body cannot change the result any more
ZK_HD u32 zk_dkim_limit(bool has_l, u64 l, u32 stride) { return has_l && l < stride ? (u32)l : stride; }
ZK_HD bool zk_dkim_decided(bool has_l, u64 l, u32 stride, u32 out_off) { return has_l && l <= stride ? out_off >= l : out_off > stride; }
ZK_HD u32 zk_dkim_final_len(bool has_l, u64 l, u32 stride, u32 out_off, u32* fits) {
  const u32 len = has_l && l < out_off ? (u32)l : out_off;
  *fits = len <= stride ? 1u : 0u;
  return *fits ? len : 0u;
}

// ------------------------------------------------------------------ serial body canonicaliser (the host path)
// out[0 .. min(stride, l)) receives the canonical bytes that lie there; returns the canonical length, or 0 with *fits = 0 when it
// exceeds the stride.  Nothing at or beyond min(stride, l, length) is written.
inline u32 zk_dkim_body_serial(const u8* raw, u32 len, u32 mode, bool has_l, u64 l, u8* out, u32 stride, u32* fits) {
  const u32 limit = zk_dkim_limit(has_l, l, stride);
  u32 out_off = 0, pend = 0;
  bool any = false;
  for (u32 i = 0; i < len; ++i) {
    if ((i % ZK_DKIM_TILE) == 0 && zk_dkim_decided(has_l, l, stride, out_off)) break;
    const ZkDkimEmit e = zk_dkim_emit(mode, i ? raw[i - 1] : ZK_DKIM_NONE, raw[i], i + 1 < len ? raw[i + 1] : ZK_DKIM_NONE);
    if (!e.content) { pend += e.n; continue; }
    for (u32 k = 0; k < pend && out_off + k < limit; ++k) out[out_off + k] = (u8)zk_dkim_pending_byte(mode, raw, i, pend, k);
    out_off += pend; pend = 0;
    if (out_off < limit) out[out_off] = (u8)e.b0;
    if (e.n == 2 && out_off + 1 < limit) out[out_off + 1] = (u8)e.b1;
    out_off += e.n;
    any = true;
  }
  if (any || mode == ZK_DKIM_SIMPLE) {
    if (out_off < limit) out[out_off] = 13;
    if (out_off + 1 < limit) out[out_off + 1] = 10;
    out_off += 2;
  }
  return zk_dkim_final_len(has_l, l, stride, out_off, fits);
}

// ------------------------------------------------------------------ SHA-256 of one byte stream
// compress(st, 64-byte block) is the caller's: zk_sha256_compress of csrc/zkwg_dev.h on the device, zk_dkim_compress_host on the host.
// `tail`: 64 bytes of the caller's (LDS on the device) for the padded last blocks.
template <class Compress>
ZK_HD void zk_dkim_sha256(const u8* data, u32 len, u8* tail, u32* st, Compress compress) {
  st[0] = 0x6a09e667u; st[1] = 0xbb67ae85u; st[2] = 0x3c6ef372u; st[3] = 0xa54ff53au;
  st[4] = 0x510e527fu; st[5] = 0x9b05688cu; st[6] = 0x1f83d9abu; st[7] = 0x5be0cd19u;
  const u32 nfull = len >> 6, rem = len & 63u;
  for (u32 b = 0; b < nfull; ++b) compress(st, data + 64u * b);
  for (u32 k = 0; k < 64; ++k) tail[k] = k < rem ? data[64u * nfull + k] : (k == rem ? 0x80 : 0);
  if (rem >= 56) {
    compress(st, tail);
    for (u32 k = 0; k < 64; ++k) tail[k] = 0;
  }
  const u64 bits = (u64)len * 8;
  for (u32 k = 0; k < 8; ++k) tail[63 - k] = (u8)(bits >> (8 * k));
  compress(st, tail);
}
ZK_HD void zk_dkim_digest_bytes(const u32* st, u8* out32) {
  for (u32 j = 0; j < 8; ++j)
    for (u32 k = 0; k < 4; ++k) out32[4 * j + k] = (u8)(st[j] >> (24 - 8 * k));
}

ZK_HD u32 zk_dkim_be32(const u8* p) { return ((u32)p[0] << 24) | ((u32)p[1] << 16) | ((u32)p[2] << 8) | (u32)p[3]; }

// 32-bit limb w (little-endian limb order) of EMSA-PKCS1-v1_5 for a modulus of k bytes:
// 00 01 FF..FF 00 | DigestInfo(SHA-256) | digest (RFC 8017 9.2); digest32 = the 32 digest bytes
ZK_HD u32 zk_dkim_em_limb(u32 w, u32 k, const u8* digest32) {
  if (w < 8) return zk_dkim_be32(digest32 + 4 * (7 - w));
  if (w == 8) return 0x05000420u;
  if (w == 9) return 0x03040201u;
  if (w == 10) return 0x86480165u;
  if (w == 11) return 0x0d060960u;
  if (w == 12) return 0x00303130u;       // (with the 00 that ends the padding)
  u32 v = 0;
  for (u32 b = 0; b < 4; ++b) {
    const u32 j = 4 * w + b;             // byte position from the least significant end
    const u32 byte = j + 2 < k ? 0xffu : (j + 2 == k ? 1u : 0u);
    v |= byte << (8 * b);
  }
  return v;
}

// ------------------------------------------------------------------ one wavefront per email (device, or the simulated wavefront)
#if defined(__HIPCC__) || defined(ZKWG_WAVESIM)
#include "zkwg_rsa_wave.h"

// The canonical body of one email.  raw: its body bytes; stage: ZK_DKIM_STAGE bytes of LDS.  Same result and same stores as
// zk_dkim_body_serial.  Per step a lane takes 16 consecutive bytes: it counts what they emit, a wave-exclusive scan places them in the
// stage, and the wavefront stores the stage to contiguous addresses.  Between steps it carries the output offset, the pending count
// and whether there was content.
ZK_DEV inline u32 zkw_dkim_body(const u8* raw, u32 len, u32 mode, bool has_l, u64 l, u8* out, u32 stride, u8* stage, u32* fits) {
  const u32 lane = ZK_LANE();
  const u32 limit = zk_dkim_limit(has_l, l, stride);
  u32 out_off = 0, pend = 0;
  bool any = false;
  for (u32 t0 = 0; t0 < len; t0 += ZK_DKIM_TILE) {
    if (zk_dkim_decided(has_l, l, stride, out_off)) break;
    const u32 i0 = t0 + ZK_DKIM_LANE_BYTES * lane;
    const u32 nvalid = i0 >= len ? 0u : zk_minu(ZK_DKIM_LANE_BYTES, len - i0);
    u32 w[4] = {0, 0, 0, 0};
    if (nvalid == ZK_DKIM_LANE_BYTES && (((uintptr_t)(raw + i0)) & 3u) == 0) {
      const u32* p = (const u32*)(raw + i0);
      w[0] = p[0]; w[1] = p[1]; w[2] = p[2]; w[3] = p[3];
    } else {
#pragma unroll
      for (u32 k = 0; k < ZK_DKIM_LANE_BYTES; ++k)
        if (k < nvalid) w[k >> 2] |= (u32)raw[i0 + k] << (8 * (k & 3));
    }
    const u32 before = nvalid && i0 ? raw[i0 - 1] : ZK_DKIM_NONE;
    const u32 after = i0 + ZK_DKIM_LANE_BYTES < len ? raw[i0 + ZK_DKIM_LANE_BYTES] : ZK_DKIM_NONE;
    // what this lane emits, and where its last content byte ends
    u32 cnt = 0, cut = 0, pv = before;
#pragma unroll
    for (u32 k = 0; k < ZK_DKIM_LANE_BYTES; ++k) {
      const u32 c = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
      const u32 nx = k + 1 < ZK_DKIM_LANE_BYTES ? (k + 1 < nvalid ? (w[(k + 1) >> 2] >> (8 * ((k + 1) & 3))) & 0xffu : ZK_DKIM_NONE) : after;
      if (k < nvalid) {
        const ZkDkimEmit e = zk_dkim_emit(mode, pv, c, nx);
        cnt += e.n;
        if (e.content) cut = cnt;
        pv = c;
      }
    }
    u32 incl = cnt;
    for (u32 d = 1; d < 64; d <<= 1) {
      const u32 o = zkw_up(incl, d);
      if (lane >= d) incl += o;
    }
    const u32 excl = incl - cnt;
    const u32 tile_total = zkw_rl(incl, 63);
    const u64 has = zkw_ballot(cut != 0);
    u32 tile_cut = 0;
    if (has) tile_cut = (u32)__shfl((int)(excl + cut), 63 - (int)__builtin_clzll(has));
    // the emitted bytes, in order, into the stage
    u32 o = excl;
    pv = before;
#pragma unroll
    for (u32 k = 0; k < ZK_DKIM_LANE_BYTES; ++k) {
      const u32 c = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
      const u32 nx = k + 1 < ZK_DKIM_LANE_BYTES ? (k + 1 < nvalid ? (w[(k + 1) >> 2] >> (8 * ((k + 1) & 3))) & 0xffu : ZK_DKIM_NONE) : after;
      if (k < nvalid) {
        const ZkDkimEmit e = zk_dkim_emit(mode, pv, c, nx);
        if (e.n) stage[o] = (u8)e.b0;
        if (e.n == 2) stage[o + 1] = (u8)e.b1;
        o += e.n;
        pv = c;
      }
    }
    ZK_SYNC();
    if (tile_cut) {
      for (u32 k = lane; k < pend && out_off + k < limit; k += 64) out[out_off + k] = (u8)zk_dkim_pending_byte(mode, raw, t0, pend, k);
      out_off += pend;
      for (u32 k = lane; k < tile_cut && out_off + k < limit; k += 64) out[out_off + k] = stage[k];
      out_off += tile_cut;
      pend = tile_total - tile_cut;
      any = true;
    } else {
      pend += tile_total;
    }
    ZK_SYNC();
  }
  if (any || mode == ZK_DKIM_SIMPLE) {
    if (lane < 2 && out_off + lane < limit) out[out_off + lane] = lane ? 10 : 13;
    out_off += 2;
  }
  return zk_dkim_final_len(has_l, l, stride, out_off, fits);
}

// sig^65537 mod n == EMSA-PKCS1-v1_5(digest)?  mod_be, sig_be: 256 bytes, big-endian, right-aligned; digest32: the SHA-256 of the
// canonical header.  The modulus has 1024 .. 2048 bits and is odd, and sig < n: otherwise false.  16 squarings and one product with the
// wavefront Barrett product of csrc/zkwg_rsa_wave.h.  Uniform result.
ZK_DEV inline bool zkw_dkim_rsa(ZkRsaLds& S, const u8* mod_be, const u8* sig_be, const u8* digest32) {
  const u32 lane = ZK_LANE();
  for (u32 w = lane; w < ZK_BIG; w += 64) {
    S.p[w] = w < 64 ? zk_dkim_be32(mod_be + 252 - 4 * w) : 0u;
    const u32 sv = w < 64 ? zk_dkim_be32(sig_be + 252 - 4 * w) : 0u;
    S.base[w] = sv; S.a[w] = sv; S.b[w] = sv;
  }
  ZK_SYNC();
  const u32 L = zkw_bitlen(S.p, 65);
  if (lane == 0) { S.L = L; S.ok = 1; }
  const u32 odd = S.p[0] & 1u;
  ZK_SYNC();
  if (L < 1024 || !odd) return false;
  if (!zkw_sub(S.q1, S.base, S.p, 65, false)) return false;          // no borrow: sig >= n
  zkw_barrett_mu(S);
  for (u32 m = 0; m < 17; ++m) {
    if (m > 0) {
      for (u32 w = lane; w < ZK_BIG; w += 64) {
        const u32 rv = w < 66 ? S.r[w] : 0u;
        S.b[w] = rv;
        S.a[w] = m < 16 ? rv : S.base[w];
      }
      ZK_SYNC();
    }
    zkw_mulmod(S);
  }
  const u32 k = (L + 7) / 8;
  bool bad = false;
  for (u32 w = lane; w < 66; w += 64) bad = bad || S.r[w] != (w < 64 ? zk_dkim_em_limb(w, k, digest32) : 0u);
  const bool ok = zkw_ballot(bad) == 0 && S.ok != 0;
  ZK_SYNC();
  return ok;
}
#endif  // __HIPCC__ || ZKWG_WAVESIM
