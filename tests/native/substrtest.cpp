// Test-only host build of the substring mains' prepare core (zkwg_substr_core.h) over the product's schedule builder.
// NOT part of the product: the CPU suite runs the core on packed records and expands the images with zkwg_expand_host.
// With -DSUBSTRTEST_MAIN the file is a stand-alone program (built with the sanitizers by tests/test_substring_cpu.py):
//   substrtest <file>   file = 10 x u32 zkwg_config | u32 n | u32 stride | n records -> prints one status per record
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "zkwg_build.h"
#include "zkwg_substr_core.h"

struct ST {
  ZkSched s;
  std::vector<ZkSeg> segs;
  std::vector<u8> ws;
};

extern "C" {
void* st_create(const zkwg_config* cfg) {
  ST* h = new ST();
  if (!build_sched(*cfg, h->s, h->segs) || !h->s.sub.present) { delete h; return nullptr; }
  h->ws.resize(zk_sub_lds_bytes(h->s.sub.L, h->s.sub.S));
  return h;
}
void st_destroy(void* p) { delete (ST*)p; }
// img_bits, img_small, in_stride, bytes of the core's working set
void st_sizes(void* p, uint32_t* out) {
  ST* h = (ST*)p;
  out[0] = h->s.img_bits; out[1] = h->s.img_small; out[2] = h->s.in_stride; out[3] = (uint32_t)h->ws.size();
}
// one email: image words into bits[img_bits] / small[img_small]; returns the status (0 or 4)
int st_run(void* p, const uint8_t* rec, uint64_t* bits, uint32_t* small) {
  ST* h = (ST*)p;
  return zk_substr_core(h->s.sub, h->s.m_one, h->s.in_off[ZK_IN_RANGE_FLAGS], rec, bits, small, h->ws.data());
}
}

#ifdef SUBSTRTEST_MAIN
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  zkwg_config cfg;
  uint32_t n = 0, stride = 0;
  if (fread(&cfg, sizeof(cfg), 1, f) != 1 || fread(&n, 4, 1, f) != 1 || fread(&stride, 4, 1, f) != 1) return 2;
  void* h = st_create(&cfg);
  if (!h) return 3;
  uint32_t sz[4];
  st_sizes(h, sz);
  if (stride != sz[2]) return 3;
  // exact-size heap blocks: a word written past the image is reported
  for (uint32_t e = 0; e < n; ++e) {
    std::vector<uint8_t> rec(stride);
    if (fread(rec.data(), stride, 1, f) != 1) return 2;
    std::vector<uint64_t> bits(sz[0]);
    std::vector<uint32_t> small(sz[1]);
    printf("%d\n", st_run(h, rec.data(), bits.data(), small.data()));
  }
  st_destroy(h);
  fclose(f);
  return 0;
}
#endif
