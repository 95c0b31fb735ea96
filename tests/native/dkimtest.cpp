// Host build of DKIM verification of raw emails (TEST INFRASTRUCTURE): the parser and the host cores of csrc/zkwg_dkim_host.h as the
// C-ABI's device = -1 path runs them, and the wavefront functions of csrc/zkwg_dkim_core.h -- the bodies of zk_dkim_body and
// zk_dkim_verify -- on the 64-fiber wavefront of tests/native/wavesim.h.
//
// With -DDKIMTEST_MAIN and without the wavefront (fibers and sanitisers do not mix) this file is a stand-alone program: it reads a
// corpus of messages (u32 count, then u32 length + bytes each), runs the parser and the serial body canonicaliser and the hash over
// every one and prints how many it took.  tests/test_dkim_cpu.py builds that with -fsanitize=address,undefined.
#if !defined(DKIMTEST_MAIN)
#define ZKWG_WAVESIM 1
#include "wavesim.h"
#endif
#include <stdio.h>
#include <string.h>
#include "../../include/zkwg.h"
#include "zkwg_dkim_host.h"

extern "C" {
int dt_parse(const uint8_t* raw, uint64_t len, const char* domain, uint8_t* header_out, uint32_t header_cap, zkwg_dkim_parsed* out) {
  return zkdkim::parse(raw, len, domain && domain[0] ? domain : nullptr, header_out, header_cap, out);
}
uint32_t dt_body_serial(const uint8_t* raw, uint32_t len, uint32_t mode, int has_l, uint64_t l, uint8_t* out, uint32_t stride, uint32_t* fits) {
  return zk_dkim_body_serial(raw, len, mode, has_l != 0, l, out, stride, fits);
}
void dt_sha256(const uint8_t* data, uint32_t len, uint8_t* out32) { zkdkim::sha256_host(data, len, out32); }
int dt_rsa_host(const uint8_t* mod_be, const uint8_t* sig_be, const uint8_t* digest32) { return zkdkim::rsa_host(mod_be, sig_be, digest32) ? 1 : 0; }
uint32_t dt_tile(void) { return ZK_DKIM_TILE; }

#if !defined(DKIMTEST_MAIN)
uint32_t dt_body_wave(const uint8_t* raw, uint32_t len, uint32_t mode, int has_l, uint64_t l, uint8_t* out, uint32_t stride, uint32_t* fits) {
  std::vector<uint8_t> stage(ZK_DKIM_STAGE);
  uint32_t res[64], f[64];
  wavesim::run([&] {
    const unsigned lane = zk_wavesim_lane();
    res[lane] = zkw_dkim_body(raw, len, mode, has_l != 0, l, out, stride, stage.data(), &f[lane]);
  }, 1u << 16);
  for (int i = 1; i < 64; ++i)
    if (res[i] != res[0] || f[i] != f[0]) return 0xffffffffu;      // the result is uniform
  *fits = f[0];
  return res[0];
}
int dt_rsa_wave(const uint8_t* mod_be, const uint8_t* sig_be, const uint8_t* digest32) {
  ZkRsaLds* S = new ZkRsaLds();
  int res[64];
  wavesim::run([&] { res[zk_wavesim_lane()] = zkw_dkim_rsa(*S, mod_be, sig_be, digest32) ? 1 : 0; }, 1u << 18);
  delete S;
  for (int i = 1; i < 64; ++i)
    if (res[i] != res[0]) return -1;
  return res[0];
}
#endif
}

#if defined(DKIMTEST_MAIN)
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t count = 0, done = 0, passed = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  for (uint32_t i = 0; i < count; ++i) {
    uint32_t len = 0;
    if (fread(&len, 4, 1, f) != 1) return 2;
    // exactly `len` bytes on the heap: a read past either end is the sanitiser's to report
    uint8_t* raw = new uint8_t[len ? len : 1];
    if (len && fread(raw, 1, len, f) != len) return 2;
    for (int with_domain = 0; with_domain < 2; ++with_domain) {
      zkwg_dkim_parsed P;
      std::vector<uint8_t> header(1024), body(4096);
      const int st = zkdkim::parse(raw, len, with_domain ? "icloud.com" : nullptr, header.data(), (uint32_t)header.size(), &P);
      if (st == ZKWG_DKIM_PASS) {
        uint32_t fits = 0;
        uint8_t d[32];
        const uint32_t bl = zk_dkim_body_serial(raw + P.body_offset, (uint32_t)P.body_len, P.body_canon, P.has_l != 0, P.l, body.data(), (uint32_t)body.size(), &fits);
        zkdkim::sha256_host(body.data(), bl, d);
        zkdkim::sha256_host(header.data(), P.header_len, d);
        ++passed;
      }
    }
    delete[] raw;
    ++done;
  }
  fclose(f);
  printf("dkimtest: %u messages, %u parses with a signature\n", done, passed);
  return done == count ? 0 : 1;
}
#endif
