// Test-only host build of the SHA-256 round records (csrc/zkwg_sha_rounds.h): the product's writer and slot decoders against a
// plain restatement of the 952-group trace.  NOT part of the product.
// With -DSHACOMPACT_MAIN the file is a stand-alone program (built with the sanitizers by tests/test_sha_compact_cpu.py):
//   shacompacttest <file>   file = n x (8 x u32 chaining state | 64 block bytes) -> prints the first bad slot of every case (-1: none)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "zkwg_sha_rounds.h"

static const uint32_t K256[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
    0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
    0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
    0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
    0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
    0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
static uint32_t rotr(uint32_t x, int r) { return (x >> r) | (x << (32 - r)); }

// the trace as zk_sha_trace wrote it before the records: one u64 per kept bit-group, in layout order; also the next chaining
// state by the textbook 32-bit compression, and the largest t1 sum met
static void trace_groups(const uint32_t hin[8], const uint8_t blk[64], uint64_t tr[952], uint32_t next[8], uint64_t* t1_max) {
  uint32_t w[64];
  for (int t = 0; t < 16; ++t) w[t] = ((uint32_t)blk[4 * t] << 24) | ((uint32_t)blk[4 * t + 1] << 16) | ((uint32_t)blk[4 * t + 2] << 8) | blk[4 * t + 3];
  for (int t = 16; t < 64; ++t) {
    uint32_t x2 = w[t - 2], x15 = w[t - 15];
    uint32_t a1 = rotr(x2, 17), b1 = rotr(x2, 19), c1 = x2 >> 10;
    uint32_t a0 = rotr(x15, 7), b0 = rotr(x15, 18), c0 = x15 >> 3;
    uint32_t s1 = a1 ^ b1 ^ c1, s0 = a0 ^ b0 ^ c0;
    uint64_t sum = (uint64_t)s1 + w[t - 7] + s0 + w[t - 16];
    uint64_t* g = tr + 0 + (t - 16) * 5;
    g[0] = s1; g[1] = b1 & c1; g[2] = s0; g[3] = b0 & c0; g[4] = sum;
    w[t] = (uint32_t)sum;
  }
  uint32_t a = hin[0], b = hin[1], c = hin[2], d = hin[3], e = hin[4], f = hin[5], g_ = hin[6], h = hin[7];
  uint32_t pa = a, pb = b, pc = c, pd = d, pe = e, pf = f, pg = g_, ph = h;   // the textbook compression beside it
  *t1_max = 0;
  for (int t = 0; t < 64; ++t) {
    uint32_t eb = rotr(e, 11), ec = rotr(e, 25);
    uint32_t bs1 = rotr(e, 6) ^ eb ^ ec;
    uint32_t ch = (e & f) ^ (~e & g_);
    uint64_t t1 = (uint64_t)h + bs1 + ch + K256[t] + w[t];
    if (t1 > *t1_max) *t1_max = t1;
    uint64_t* g1 = tr + 240 + t * 4;
    g1[0] = ch; g1[1] = bs1; g1[2] = eb & ec; g1[3] = t1;
    uint32_t ab = rotr(a, 13), ac = rotr(a, 22);
    uint32_t bs0 = rotr(a, 2) ^ ab ^ ac;
    uint32_t mmid = b & c;
    uint32_t maj = (a & (b ^ c)) | mmid;
    uint64_t t2 = (uint64_t)bs0 + maj;
    uint64_t* g2 = tr + 496 + t * 5;
    g2[0] = bs0; g2[1] = ab & ac; g2[2] = maj; g2[3] = mmid; g2[4] = t2;
    uint64_t sume = (uint64_t)d + (uint32_t)t1;
    uint64_t suma = (uint64_t)(uint32_t)t1 + (uint32_t)t2;
    tr[816 + t] = suma;
    tr[880 + t] = sume;
    h = g_; g_ = f; f = e; e = (uint32_t)sume; d = c; c = b; b = a; a = (uint32_t)suma;
    uint32_t q1 = ph + (rotr(pe, 6) ^ rotr(pe, 11) ^ rotr(pe, 25)) + ((pe & pf) ^ (~pe & pg)) + K256[t] + w[t];
    uint32_t q2 = (rotr(pa, 2) ^ rotr(pa, 13) ^ rotr(pa, 22)) + ((pa & pb) ^ (pa & pc) ^ (pb & pc));
    ph = pg; pg = pf; pf = pe; pe = pd + q1; pd = pc; pc = pb; pb = pa; pa = q1 + q2;
  }
  const uint32_t fin[8] = {a, b, c, d, e, f, g_, h}, pfin[8] = {pa, pb, pc, pd, pe, pf, pg, ph};
  for (int j = 0; j < 8; ++j) { tr[944 + j] = (uint64_t)hin[j] + fin[j]; next[j] = hin[j] + pfin[j]; }
}
// bit of kept signal `slot` (0 .. 30,951, layout order) in the trace: the decoders zk_expand ran before the records
static uint32_t trace_bit(const uint64_t tr[952], uint32_t slot) {
  struct { uint32_t n, per, words, base; } part[3] = {{48 * 162, 162, 5, 0}, {64 * 131, 131, 4, 240}, {64 * 161, 161, 5, 496}};
  for (auto& p : part) {
    if (slot < p.n) {
      const uint32_t i = slot / p.per, q = slot % p.per, sub = (q >> 5) < p.words - 1 ? (q >> 5) : p.words - 1;
      return (uint32_t)(tr[p.base + i * p.words + sub] >> (q - sub * 32)) & 1u;
    }
    slot -= p.n;
  }
  return (uint32_t)(tr[816 + slot / 33] >> (slot % 33)) & 1u;
}

extern "C" {
// one (state, block): the product's writer leaves the record, the product's decoders give all 30,952 slots from it.
// -> first slot that differs from the trace's bit (-1: none); -2: the product's own trace writer differs from the restatement.
// rec_next = hin + {A[63..60], E[63..60]} from the record, ref_next = the textbook compression's next state
long long sc_check(const uint32_t* hin, const uint8_t* blk, uint32_t* rec_next, uint32_t* ref_next, uint64_t* t1_max) {
  std::vector<uint64_t> tr(952), tr2(952);
  trace_groups(hin, blk, tr.data(), ref_next, t1_max);
  // (heap buffers of the exact sizes: the sanitizer build sees any access outside the record)
  std::vector<uint32_t> rec(ZK_SHAR_WORDS + 3);
  uint32_t* r = rec.data();
  while ((uintptr_t)r & 15) ++r;   // the writer's stores are 16-byte aligned
  uint32_t w[64];
  for (int t = 0; t < 16; ++t) w[t] = ((uint32_t)blk[4 * t] << 24) | ((uint32_t)blk[4 * t + 1] << 16) | ((uint32_t)blk[4 * t + 2] << 8) | blk[4 * t + 3];
  zk_sha_rounds<true, true>(w, hin, r, tr2.data());
  if (tr != tr2) return -2;
  std::vector<uint32_t> rec2(r, r + ZK_SHAR_WORDS);   // an exact-size copy for the decoders
  for (int j = 0; j < 8; ++j) rec_next[j] = hin[j] + rec2[(j < 4 ? ZK_SHAR_A : ZK_SHAR_E + 4) + 63 - j];
  const uint32_t n_sp = 48 * ZK_SP_SLOTS, n_t1 = 64 * ZK_T1_SLOTS, n_t2 = 64 * ZK_T2_SLOTS;
  for (uint32_t slot = 0; slot < ZK_COMP_SLOTS; ++slot) {
    uint32_t got;
    if (slot < n_sp) got = zk_shar_sp(rec2.data(), slot);
    else if (slot < n_sp + n_t1) got = zk_shar_t1(rec2.data(), slot - n_sp);
    else if (slot < n_sp + n_t1 + n_t2) got = zk_shar_t2(rec2.data(), slot - n_sp - n_t1);
    else got = zk_shar_sum(rec2.data(), slot - n_sp - n_t1 - n_t2);
    if (got != trace_bit(tr.data(), slot)) return slot;
  }
  return -1;
}
}

#ifdef SHACOMPACT_MAIN
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint8_t buf[96];
  int bad = 0;
  while (fread(buf, 1, 96, f) == 96) {
    uint32_t hin[8], a[8], b[8];
    uint64_t t1;
    memcpy(hin, buf, 32);
    const long long r = sc_check(hin, buf + 32, a, b, &t1);
    printf("%lld\n", r);
    if (r != -1 || memcmp(a, b, 32)) bad = 1;
  }
  fclose(f);
  return bad;
}
#endif
