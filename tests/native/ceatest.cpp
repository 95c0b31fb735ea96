// Test-only host build of CleanEmailAddress's prepare core (zkwg_cea_core.h) over the product's schedule builder.  NOT part of the
// product: the CPU suite runs the core on packed records and expands the images with zkwg_expand_host.
// With -DCEATEST_MAIN the file is a stand-alone program (built with the sanitizers by tests/test_clean_address_cpu.py):
//   ceatest <file>   file = 10 x u32 zkwg_config | u32 n | u32 stride | n records
//                    -> prints per record the status, isValid and a checksum of the field elements written
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "zkwg_build.h"
#include "zkwg_poseidon_sparse.h"
#include "zkwg_cea_core.h"

struct CT {
  ZkSched s;
  std::vector<ZkSeg> segs;
  std::vector<u32> pos16, pos2;   // the two tables in limb form (zkwg_poseidon29.h)
};

extern "C" {
void* ct_create(const zkwg_config* cfg) {
  CT* h = new CT();
  if (!build_sched(*cfg, h->s, h->segs) || !h->s.cea.present) { delete h; return nullptr; }
  std::vector<Fr> C, M, t16, t2;
  build_poseidon_constants(17, 8, 68, C, M);
  bool ok = zk_build_poseidon_sparse(17, 68, C, M, t16);
  build_poseidon_constants(3, 8, 57, C, M);
  ok = ok && zk_build_poseidon_sparse(3, 57, C, M, t2);
  if (!ok) { delete h; return nullptr; }
  zk_build_poseidon29(17, 68, t16, h->pos16);
  zk_build_poseidon29(3, 57, t2, h->pos2);
  return h;
}
void ct_destroy(void* p) { delete (CT*)p; }
// img_bits, img_small, img_fr, in_stride
void ct_sizes(void* p, uint32_t* out) {
  CT* h = (CT*)p;
  out[0] = h->s.img_bits; out[1] = h->s.img_small; out[2] = h->s.img_fr; out[3] = h->s.in_stride;
}
// one email: image words into small[img_small] / frv[img_fr] (the main has no bit groups); returns the status
int ct_run(void* p, const uint8_t* rec, uint32_t* small, void* frv) {
  CT* h = (CT*)p;
  const ZkCeaLayout& E = h->s.cea;
  // exact-size state blocks (element j, limb l at st[l * T + j]): an access past the state is reported by the sanitizers
  std::vector<u32> st16(9 * 17), st2(9 * 3);
  for (u32 c = 0; c < E.nch; ++c) zk_cea_chunk_core<0>(E, rec, (Fr*)frv, c, st16.data(), 1, 17, h->pos16.data(), nullptr, 0);
  return zk_cea_tail_core(E, h->s.m_one, h->s.in_off[ZK_IN_RANGE_FLAGS], rec, (Fr*)frv, small, st2.data(), 1, 3, h->pos2.data());
}
}

#ifdef CEATEST_MAIN
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  zkwg_config cfg;
  uint32_t n = 0, stride = 0;
  if (fread(&cfg, sizeof(cfg), 1, f) != 1 || fread(&n, 4, 1, f) != 1 || fread(&stride, 4, 1, f) != 1) return 2;
  void* h = ct_create(&cfg);
  if (!h) return 3;
  uint32_t sz[4];
  ct_sizes(h, sz);
  if (stride != sz[3]) return 3;
  const uint32_t m_valid = ((CT*)h)->s.cea.m_valid;
  // exact-size heap blocks: a word written past the image is reported
  for (uint32_t e = 0; e < n; ++e) {
    std::vector<uint8_t> rec(stride);
    if (fread(rec.data(), stride, 1, f) != 1) return 2;
    std::vector<uint32_t> small(sz[1]);
    std::vector<Fr> frv(sz[2]);
    const int st = ct_run(h, rec.data(), small.data(), frv.data());
    uint64_t sum = 0;
    for (const Fr& v : frv) sum = sum * 1099511628211ull + (v.l[0] ^ v.l[1] ^ v.l[2] ^ v.l[3]);
    printf("%d %u %016llx\n", st, small[m_valid], (unsigned long long)sum);
  }
  ct_destroy(h);
  fclose(f);
  return 0;
}
#endif
