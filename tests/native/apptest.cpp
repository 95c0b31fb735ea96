// Test-only host build of EmailReveal's own prepare cores (zkwg_app_core.h, and zkwg_substr_core.h for its RevealSubstring
// component) over the product's schedule builder.  NOT part of the product: the CPU suite runs the cores on packed records and
// expands the images with zkwg_expand_host; EmailVerifier's words of the image are left zero (its kernels have no host build).
// With -DAPPTEST_MAIN the file is a stand-alone program (built with the sanitizers by tests/test_email_reveal_cpu.py):
//   apptest <file>   file = 10 x u32 zkwg_config | 4 x u32 zkwg_app_config | u32 n | u32 stride | n records
//                    -> prints per record the status and a checksum of the field elements written
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "zkwg_build.h"
#include "zkwg_substr_core.h"
#include "zkwg_app_core.h"

struct AT {
  ZkSched s;
  std::vector<ZkSeg> segs;
  std::vector<u8> ws;
  std::vector<Fr> pos9, pos1;
};

extern "C" {
void* at_create(const zkwg_config* cfg, const zkwg_app_config* app) {
  AT* h = new AT();
  if (!build_sched(*cfg, h->s, h->segs, nullptr, app) || !h->s.app.present) { delete h; return nullptr; }
  h->ws.resize(zk_sub_lds_bytes(h->s.sub.L, h->s.sub.S));
  std::vector<Fr> C, M;
  build_poseidon_constants(10, 8, 60, C, M);
  bool ok = zk_build_poseidon_sparse(10, 60, C, M, h->pos9);
  build_poseidon_constants(2, 8, 56, C, M);
  ok = ok && zk_build_poseidon_sparse(2, 56, C, M, h->pos1);
  if (!ok) { delete h; return nullptr; }
  return h;
}
void at_destroy(void* p) { delete (AT*)p; }
// img_bits, img_small, img_fr, in_stride
void at_sizes(void* p, uint32_t* out) {
  AT* h = (AT*)p;
  out[0] = h->s.img_bits; out[1] = h->s.img_small; out[2] = h->s.img_fr; out[3] = h->s.in_stride;
}
// one email: image words into bits[img_bits] / small[img_small] / frv[img_fr]; returns RevealSubstring's status (0 or 4)
int at_run(void* p, const uint8_t* rec, uint64_t* bits, uint32_t* small, void* frv) {
  AT* h = (AT*)p;
  const int st = zk_substr_core(h->s.sub, h->s.m_one, h->s.in_off[ZK_IN_RANGE_FLAGS], rec, bits, small, h->ws.data());
  Fr state[10], tmp[10];
  zk_app_core(h->s.app, rec, (Fr*)frv, h->pos9.data(), h->pos1.data(), state, tmp, 1);
  return st;
}
}

#ifdef APPTEST_MAIN
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  zkwg_config cfg;
  zkwg_app_config app;
  uint32_t n = 0, stride = 0;
  if (fread(&cfg, sizeof(cfg), 1, f) != 1 || fread(&app, sizeof(app), 1, f) != 1 || fread(&n, 4, 1, f) != 1 || fread(&stride, 4, 1, f) != 1) return 2;
  void* h = at_create(&cfg, &app);
  if (!h) return 3;
  uint32_t sz[4];
  at_sizes(h, sz);
  if (stride != sz[3]) return 3;
  // exact-size heap blocks: a word written past the image is reported
  for (uint32_t e = 0; e < n; ++e) {
    std::vector<uint8_t> rec(stride);
    if (fread(rec.data(), stride, 1, f) != 1) return 2;
    std::vector<uint64_t> bits(sz[0]);
    std::vector<uint32_t> small(sz[1]);
    std::vector<Fr> frv(sz[2]);
    const int st = at_run(h, rec.data(), bits.data(), small.data(), frv.data());
    uint64_t sum = 0;
    for (const Fr& v : frv) sum = sum * 1099511628211ull + (v.l[0] ^ v.l[1] ^ v.l[2] ^ v.l[3]);
    printf("%d %016llx\n", st, (unsigned long long)sum);
  }
  at_destroy(h);
  fclose(f);
  return 0;
}
#endif
