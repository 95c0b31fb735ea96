// DKIM verification of raw emails -- the host side: the message parser behind zkwg_dkim_parse, and the host forms of
// SHA-256 and of the RSA check for device = -1.  Plain C++, no GPU.  Restates, for the one signature that is verified,
//   lib/mailauth/message-parser.ts:43-86     where the header block ends
//   lib/mailauth/tools.ts:75-105             parseHeaders: rows, continuation rows, key = the text before the first colon
//   lib/mailauth/parse-dkim-headers.ts:123-309   the tag list (comments in parentheses are dropped, quotes are kept as they stand)
//   lib/mailauth/dkim-verifier.ts:85-175     From addresses, the signature's fields and the signatures that are skipped
//   lib/mailauth/tools.ts:107-140            getSigningHeaderLines: every name of h= takes the lowest field of that name still there
//   lib/mailauth/header/relaxed.ts:20-78, header/simple.ts:23-83, tools.ts:441-454 formatRelaxedLine
//   dkim/index.ts:140-153                    which signature: the one of `domain`, else of the single From address
// Every index is checked against the buffer: malformed input gives a status, never a read outside it.
#pragma once
#include <string.h>
#include <string>
#include <vector>
#include "../../include/zkwg.h"
#include "zkwg_dkim_core.h"

namespace zkdkim {

inline bool is_ws(unsigned char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n' || c == '\v' || c == '\f'; }   // JS \s, ASCII part
inline std::string trim(const std::string& s) {
  size_t a = 0, b = s.size();
  while (a < b && is_ws((unsigned char)s[a])) ++a;
  while (b > a && is_ws((unsigned char)s[b - 1])) --b;
  return s.substr(a, b - a);
}
inline std::string lower(std::string s) {
  for (char& c : s) if (c >= 'A' && c <= 'Z') c = (char)(c + 32);
  return s;
}
inline std::string collapse_ws(const std::string& s) {       // .replace(/\s+/g, ' ')
  std::string o;
  bool in = false;
  for (char c : s) {
    if (is_ws((unsigned char)c)) { if (!in) o.push_back(' '); in = true; }
    else { o.push_back(c); in = false; }
  }
  return o;
}
inline std::string strip_ws(const std::string& s) {
  std::string o;
  for (char c : s) if (!is_ws((unsigned char)c)) o.push_back(c);
  return o;
}

struct Field {
  std::string key;      // lower-cased, trimmed text before the first colon
  std::string line;     // the rows of the field joined with CR LF, no line end after the last one
  bool used = false;
};

// the offset of the body: right after the first LF that follows LF or LF CR (message-parser.ts:57-61); len when there is none
inline size_t body_offset(const uint8_t* raw, size_t len) {
  for (size_t i = 1; i < len; ++i)
    if (raw[i] == '\n' && (raw[i - 1] == '\n' || (i >= 2 && raw[i - 1] == '\r' && raw[i - 2] == '\n'))) return i + 1;
  return len;
}

inline std::vector<Field> parse_fields(const uint8_t* raw, size_t hlen) {
  while (hlen && (raw[hlen - 1] == '\r' || raw[hlen - 1] == '\n')) --hlen;       // .replace(/[\r\n]+$/, '')
  std::vector<Field> out;
  size_t pos = 0;
  for (;;) {
    size_t e = pos;
    while (e < hlen && raw[e] != '\n') ++e;
    size_t re = e;
    if (re > pos && e < hlen && raw[re - 1] == '\r') --re;                        // split(/\r?\n/)
    std::string row((const char*)raw + pos, re - pos);
    if (!out.empty() && !row.empty() && is_ws((unsigned char)row[0])) out.back().line += "\r\n" + row;
    else { Field f; f.line = row; out.push_back(f); }
    if (e >= hlen) break;
    pos = e + 1;
  }
  for (Field& f : out) {
    const size_t c = f.line.find(':');
    f.key = lower(trim(f.line.substr(0, c == std::string::npos ? f.line.size() : c)));
  }
  return out;
}

// tools.ts:441-454
inline std::string relaxed_line(const std::string& line) {
  std::string s;
  for (size_t i = 0; i < line.size(); ++i) {                                      // .replace(/\r?\n/g, '')
    if (line[i] == '\n') continue;
    if (line[i] == '\r' && i + 1 < line.size() && line[i + 1] == '\n') continue;
    s.push_back(line[i]);
  }
  const size_t c = s.find(':');
  if (c != std::string::npos) {                                                   // /^([^:]*):\s*/ -> lower-cased trimmed key + ':'
    size_t v = c + 1;
    while (v < s.size() && is_ws((unsigned char)s[v])) ++v;
    s = lower(trim(s.substr(0, c))) + ":" + s.substr(v);
  }
  return trim(collapse_ws(s));
}
// .replace(/([;:\s]+b=)[^;]+/, '$1'): the first b= that follows ; : or white space and has a value loses it
inline std::string empty_b(const std::string& s) {
  for (size_t i = 1; i + 2 < s.size(); ++i) {
    const unsigned char p = (unsigned char)s[i - 1];
    if (s[i] == 'b' && s[i + 1] == '=' && (p == ';' || p == ':' || is_ws(p)) && s[i + 2] != ';') {
      size_t e = i + 2;
      while (e < s.size() && s[e] != ';') ++e;
      return s.substr(0, i + 2) + s.substr(e);
    }
  }
  return s;
}

struct Tags {
  std::vector<std::pair<std::string, std::string>> kv;      // the last entry of a key wins (parse-dkim-headers.ts:301)
  const std::string* get(const char* k) const {
    for (size_t i = kv.size(); i-- > 0;) if (kv[i].first == k) return &kv[i].second;
    return nullptr;
  }
};
inline Tags parse_tags(const std::string& line) {
  Tags t;
  const size_t c = line.find(':');
  const std::string v = trim(c == std::string::npos ? line : line.substr(c + 1));
  std::string key, val;
  bool in_val = false;
  int depth = 0;
  auto flush = [&]() {
    std::string k = lower(trim(collapse_ws(key))), x = trim(collapse_ws(val));
    if (k == "bh" || k == "b" || k == "p" || k == "h") x = strip_ws(x);
    if (!k.empty() && in_val) t.kv.push_back({k, x});
    key.clear(); val.clear(); in_val = false;
  };
  for (char ch : v) {
    if (depth) { if (ch == ')') --depth; continue; }
    if (ch == '(') { ++depth; continue; }
    if (ch == ';') { flush(); continue; }
    if (!in_val && ch == '=') { in_val = true; continue; }
    (in_val ? val : key).push_back(ch);
  }
  flush();
  return t;
}

inline int b64_value(unsigned char c) {
  if (c >= 'A' && c <= 'Z') return c - 'A';
  if (c >= 'a' && c <= 'z') return c - 'a' + 26;
  if (c >= '0' && c <= '9') return c - '0' + 52;
  if (c == '+') return 62;
  if (c == '/') return 63;
  return -1;
}
// strict base64 (padding optional) -> false on any other character
inline bool b64_decode(const std::string& s, std::vector<uint8_t>& out) {
  out.clear();
  uint32_t acc = 0;
  int bits = 0;
  size_t n = s.size();
  while (n && s[n - 1] == '=') --n;
  if (s.size() - n > 2) return false;
  for (size_t i = 0; i < n; ++i) {
    const int v = b64_value((unsigned char)s[i]);
    if (v < 0) return false;
    acc = (acc << 6) | (uint32_t)v;
    bits += 6;
    if (bits >= 8) { bits -= 8; out.push_back((uint8_t)(acc >> bits)); acc &= (1u << bits) - 1u; }
  }
  return (n & 3) != 1;
}

// the addresses of one From value (a reduced addressparser: comma-separated mailboxes, "quoted names", <angle addresses>, (comments))
inline void from_addresses(const std::string& value, std::vector<std::string>& out) {
  std::string plain, angle;
  bool in_q = false, in_a = false, had_a = false;
  int depth = 0;
  auto flush = [&]() {
    std::string a = trim(had_a ? angle : plain);
    if (!had_a) {                                     // a bare mailbox: its last blank-separated word with an @
      std::string best, cur;
      for (char c : a + " ") {
        if (is_ws((unsigned char)c)) { if (cur.find('@') != std::string::npos) best = cur; cur.clear(); }
        else cur.push_back(c);
      }
      a = best;
    }
    if (a.find('@') != std::string::npos) out.push_back(a);
    plain.clear(); angle.clear(); had_a = false;
  };
  for (size_t i = 0; i < value.size(); ++i) {
    const char c = value[i];
    if (in_q) { if (c == '\\' && i + 1 < value.size()) ++i; else if (c == '"') in_q = false; continue; }
    if (depth) { if (c == ')') --depth; else if (c == '(') ++depth; continue; }
    if (in_a) { if (c == '>') in_a = false; else angle.push_back(c); continue; }
    if (c == '"') { in_q = true; continue; }
    if (c == '(') { ++depth; continue; }
    if (c == '<') { in_a = true; had_a = true; continue; }
    if (c == ',' || c == ';') { flush(); continue; }
    plain.push_back(c);
  }
  flush();
}

inline void put(char* dst, size_t cap, const std::string& s) {
  const size_t n = s.size() < cap - 1 ? s.size() : cap - 1;
  memcpy(dst, s.data(), n);
  dst[n] = 0;
}

// include/zkwg.h zkwg_dkim_parse
inline int parse(const uint8_t* raw, uint64_t len, const char* domain_arg, uint8_t* header_out, uint32_t header_cap, zkwg_dkim_parsed* P) {
  memset(P, 0, sizeof *P);
  const size_t boff = body_offset(raw, (size_t)len);
  P->body_offset = boff;
  P->body_len = len - boff;
  std::vector<Field> fields = parse_fields(raw, boff);
  std::vector<std::string> from;
  for (const Field& f : fields)
    if (f.key == "from") {
      const size_t c = f.line.find(':');
      from_addresses(trim(c == std::string::npos ? f.line : f.line.substr(c + 1)), from);
    }
  std::string domain = domain_arg ? domain_arg : "";
  if (domain.empty()) {
    if (from.size() > 1) return P->status = ZKWG_DKIM_MULTIPLE_FROM;
    if (!from.empty()) {                              // headerFrom[0].split('@')[1]
      const size_t a = from[0].find('@');
      const size_t b = from[0].find('@', a + 1);
      domain = from[0].substr(a + 1, b == std::string::npos ? std::string::npos : b - a - 1);
    }
  }
  put(P->d, sizeof P->d, domain);
  // the first signature of that domain among the ones dkim-verifier.ts:146-161 does not skip
  const Field* sig = nullptr;
  Tags T;
  std::string algo, hcanon, bcanon;
  for (const Field& f : fields) {
    if (f.key != "dkim-signature") continue;
    Tags t = parse_tags(f.line);
    const std::string *a = t.get("a"), *c = t.get("c"), *d = t.get("d"), *s = t.get("s");
    const std::string al = lower(a ? *a : std::string());
    const size_t dash = al.find('-'), rdash = al.rfind('-');
    const std::string sign = trim(dash == std::string::npos ? al : al.substr(0, dash)), hash = trim(rdash == std::string::npos ? al : al.substr(rdash + 1));
    const std::string cv = lower(c ? *c : std::string());
    const size_t slash = cv.find('/');
    std::string hc = trim(slash == std::string::npos ? cv : cv.substr(0, slash)), bc;
    if (slash != std::string::npos) { const size_t s2 = cv.find('/', slash + 1); bc = trim(cv.substr(slash + 1, s2 == std::string::npos ? std::string::npos : s2 - slash - 1)); }
    if (hc.empty()) hc = "simple";
    if (bc.empty()) bc = "simple";
    if ((sign != "rsa" && sign != "ed25519") || (hash != "sha256" && hash != "sha1") || (hc != "relaxed" && hc != "simple") || (bc != "relaxed" && bc != "simple") ||
        !d || d->empty() || !s || s->empty())
      continue;
    if (*d != domain) continue;
    sig = &f; T = t; algo = trim(al); hcanon = hc; bcanon = bc;
    break;
  }
  if (!sig) return P->status = ZKWG_DKIM_NOT_FOUND;
  put(P->s, sizeof P->s, *T.get("s"));
  put(P->a, sizeof P->a, T.get("a") ? *T.get("a") : std::string());
  put(P->c, sizeof P->c, T.get("c") ? *T.get("c") : std::string());
  P->header_canon = hcanon == "simple" ? ZK_DKIM_SIMPLE : ZK_DKIM_RELAXED;
  P->body_canon = bcanon == "simple" ? ZK_DKIM_SIMPLE : ZK_DKIM_RELAXED;
  const std::string *h = T.get("h"), *bh = T.get("bh"), *b = T.get("b"), *l = T.get("l");
  if (algo != "rsa-sha256" || !h || !bh || !b || T.get("d")->size() >= sizeof P->d || T.get("s")->size() >= sizeof P->s || P->body_len > ZK_DKIM_MAX_RAW)
    return P->status = ZKWG_DKIM_UNSUPPORTED;
  if (l) {
    if (l->empty() || l->size() > 18) return P->status = ZKWG_DKIM_UNSUPPORTED;
    uint64_t v = 0;
    for (char ch : *l) { if (ch < '0' || ch > '9') return P->status = ZKWG_DKIM_UNSUPPORTED; v = v * 10 + (uint64_t)(ch - '0'); }
    P->has_l = 1; P->l = v;
  }
  std::vector<uint8_t> raw_bh, raw_b;
  if (!b64_decode(*bh, raw_bh) || raw_bh.size() != 32 || bh->size() != 44 || !b64_decode(*b, raw_b) || raw_b.empty() || raw_b.size() > 256)
    return P->status = ZKWG_DKIM_UNSUPPORTED;
  memcpy(P->bh, raw_bh.data(), 32);
  put(P->bh_b64, sizeof P->bh_b64, *bh);
  memcpy(P->signature + 256 - raw_b.size(), raw_b.data(), raw_b.size());
  P->signature_len = (uint32_t)raw_b.size();
  // the canonical signed header
  std::string canon;
  size_t start = 0;
  const std::string& hv = *h;
  while (start <= hv.size()) {
    size_t e = hv.find(':', start);
    if (e == std::string::npos) e = hv.size();
    const std::string name = lower(trim(hv.substr(start, e - start)));
    start = e + 1;
    if (name.empty()) continue;
    for (size_t i = fields.size(); i-- > 0;)
      if (!fields[i].used && fields[i].key == name) {
        fields[i].used = true;
        canon += (P->header_canon == ZK_DKIM_RELAXED ? relaxed_line(fields[i].line) : fields[i].line) + "\r\n";
        break;
      }
  }
  canon += empty_b(P->header_canon == ZK_DKIM_RELAXED ? relaxed_line(sig->line) : sig->line);
  if (canon.size() > header_cap) { P->header_len = (uint32_t)(canon.size() > 0xffffffffu ? 0xffffffffu : canon.size()); return P->status = ZKWG_DKIM_UNSUPPORTED; }
  if (header_out) memcpy(header_out, canon.data(), canon.size());
  P->header_len = (uint32_t)canon.size();
  return P->status = ZKWG_DKIM_PASS;
}

// ------------------------------------------------------------------ SHA-256 and RSA on the host (device = -1)
inline uint32_t rotr(uint32_t x, int r) { return (x >> r) | (x << (32 - r)); }
inline void compress_host(uint32_t* st, const uint8_t* blk) {
  static const uint32_t K[64] = {
      0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74,
      0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d,
      0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e,
      0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5,
      0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
  uint32_t w[64];
  for (int t = 0; t < 16; ++t) w[t] = zk_dkim_be32(blk + 4 * t);
  for (int t = 16; t < 64; ++t) w[t] = (rotr(w[t - 2], 17) ^ rotr(w[t - 2], 19) ^ (w[t - 2] >> 10)) + w[t - 7] + (rotr(w[t - 15], 7) ^ rotr(w[t - 15], 18) ^ (w[t - 15] >> 3)) + w[t - 16];
  uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
  for (int t = 0; t < 64; ++t) {
    const uint32_t t1 = h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[t] + w[t];
    const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
    h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
  }
  st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}
inline void sha256_host(const uint8_t* data, uint32_t len, uint8_t* out32) {
  uint32_t st[8];
  uint8_t tail[64];
  zk_dkim_sha256(data, len, tail, st, [](uint32_t* s, const uint8_t* blk) { compress_host(s, blk); });
  zk_dkim_digest_bytes(st, out32);
}

// the same verdict as zkw_dkim_rsa (csrc/zkwg_dkim_core.h), by Montgomery products over 64-bit limbs (R = 2^(64 nl)); R^2 mod n comes from
// R mod n -- a few doublings of 2^(L-1) -- by square-and-double along the bits of 64 nl
inline bool rsa_host(const uint8_t* mod_be, const uint8_t* sig_be, const uint8_t* digest32) {
  typedef unsigned __int128 u128;
  uint32_t n32[64], s32[64];
  for (int w = 0; w < 64; ++w) { n32[w] = zk_dkim_be32(mod_be + 252 - 4 * w); s32[w] = zk_dkim_be32(sig_be + 252 - 4 * w); }
  const uint32_t L = zk_seq_bitlen(n32, 64);
  if (L < 1024 || !(n32[0] & 1u) || zk_seq_cmp(s32, n32, 64) >= 0) return false;
  const uint32_t nl = (L + 63) / 64;
  uint64_t n[32], s[32];
  for (uint32_t i = 0; i < 32; ++i) { n[i] = (uint64_t)n32[2 * i] | ((uint64_t)n32[2 * i + 1] << 32); s[i] = (uint64_t)s32[2 * i] | ((uint64_t)s32[2 * i + 1] << 32); }
  uint64_t ninv = 1;                                   // -n^-1 mod 2^64
  for (int i = 0; i < 6; ++i) ninv *= 2u - n[0] * ninv;
  ninv = 0u - ninv;
  auto geq_n = [&](const uint64_t* x) { for (uint32_t i = nl; i-- > 0;) { if (x[i] != n[i]) return x[i] > n[i]; } return true; };
  auto sub_n = [&](uint64_t* x) { uint64_t bw = 0; for (uint32_t i = 0; i < nl; ++i) { const u128 d = (u128)x[i] - n[i] - bw; x[i] = (uint64_t)d; bw = (uint64_t)(d >> 64) & 1; } };
  auto dbl = [&](uint64_t* x) {                        // x = 2 x mod n, x < n
    uint64_t top = 0;
    for (uint32_t j = 0; j < nl; ++j) { const uint64_t v = x[j]; x[j] = (v << 1) | top; top = v >> 63; }
    if (top || geq_n(x)) sub_n(x);
  };
  auto mont = [&](const uint64_t* a, const uint64_t* b, uint64_t* out) {
    uint64_t t[34];
    for (uint32_t i = 0; i < nl + 2; ++i) t[i] = 0;
    for (uint32_t i = 0; i < nl; ++i) {
      uint64_t c = 0;
      for (uint32_t j = 0; j < nl; ++j) { const u128 v = (u128)a[j] * b[i] + t[j] + c; t[j] = (uint64_t)v; c = (uint64_t)(v >> 64); }
      u128 v = (u128)t[nl] + c; t[nl] = (uint64_t)v; t[nl + 1] = (uint64_t)(v >> 64);
      const uint64_t m = t[0] * ninv;
      c = (uint64_t)(((u128)m * n[0] + t[0]) >> 64);
      for (uint32_t j = 1; j < nl; ++j) { const u128 u = (u128)m * n[j] + t[j] + c; t[j - 1] = (uint64_t)u; c = (uint64_t)(u >> 64); }
      v = (u128)t[nl] + c; t[nl - 1] = (uint64_t)v;
      t[nl] = t[nl + 1] + (uint64_t)(v >> 64);
    }
    if (t[nl] || geq_n(t)) sub_n(t);
    for (uint32_t i = 0; i < nl; ++i) out[i] = t[i];
  };
  uint64_t r1[32] = {0};                               // R mod n
  r1[(L - 1) / 64] = 1ull << ((L - 1) & 63);           // 2^(L-1) < n
  for (uint32_t i = L - 1; i < 64 * nl; ++i) dbl(r1);
  uint64_t r2[32];                                     // 2^e R mod n for the leading bits e of 64 nl; ends as R^2 mod n
  for (uint32_t i = 0; i < nl; ++i) r2[i] = r1[i];
  const uint32_t e = 64 * nl;
  for (int bit = 31 - __builtin_clz(e); bit >= 0; --bit) {
    if (bit != 31 - __builtin_clz(e)) mont(r2, r2, r2);
    if ((e >> bit) & 1u) dbl(r2);
  }
  uint64_t x[32], y[32], one[32] = {1};
  mont(s, r2, x);
  for (uint32_t i = 0; i < nl; ++i) y[i] = x[i];
  for (int i = 0; i < 16; ++i) mont(y, y, y);
  mont(y, x, y);
  mont(y, one, y);
  const uint32_t k = (L + 7) / 8;
  for (uint32_t w = 0; w < 2 * nl; ++w)
    if ((uint32_t)(y[w >> 1] >> (32 * (w & 1))) != (w < 64 ? zk_dkim_em_limb(w, k, digest32) : 0u)) return false;
  return true;
}

}  // namespace zkdkim
