// Host build of the substring search of csrc/zkwg_locate_core.h (TEST INFRASTRUCTURE): zkw_locate -- what zk_gen_reveal_inputs finds and
// counts the needle with -- on the 64-fiber wavefront of tests/native/wavesim.h, and its serial statement.
#define ZKWG_WAVESIM 1
#include "wavesim.h"
#include <string.h>
#include <vector>
#include "zkwg_locate_core.h"

extern "C" {
uint32_t lt_tile(void) { return ZK_LOC_TILE; }
uint32_t lt_chunk(void) { return ZK_LOC_CHUNK; }
uint32_t lt_serial(const uint8_t* src, uint32_t len, const uint8_t* nd, uint32_t L, uint32_t what) { return zk_locate_serial(src, len, nd, L, what); }
// src_off: the source is copied to a 16-byte aligned buffer at this offset, so that both load paths are reached on purpose.  The copy
// has exactly `len` bytes behind the offset and the needle exactly L: a read beyond either is outside the allocation.
// Returns the uniform result, or 0xfffffffe when the lanes disagree.
uint32_t lt_wave(const uint8_t* src, uint32_t len, const uint8_t* nd, uint32_t L, uint32_t what, uint32_t src_off) {
  std::vector<uint8_t> raw(len + src_off + 16), pat(L ? L : 1);
  uint8_t* base = raw.data() + ((16 - ((uintptr_t)raw.data() & 15)) & 15) + src_off;
  if (len) memcpy(base, src, len);
  if (L) memcpy(pat.data(), nd, L);
  alignas(16) static thread_local uint8_t lds[ZK_LOC_LDS];
  uint8_t* l = lds;
  uint32_t res[64];
  wavesim::run([&] { res[zk_wavesim_lane()] = zkw_locate(base, len, pat.data(), L, what, l); }, 1u << 16);
  for (int i = 1; i < 64; ++i)
    if (res[i] != res[0]) return 0xfffffffeu;
  return res[0];
}
}
