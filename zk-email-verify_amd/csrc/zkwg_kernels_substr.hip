// zk_substr -- main = RevealSubstring(L, S, uniq) / CountSubstringOccurrences(L, S): one wavefront per email
//           (zkwg_substr_core.h), in[] and the substring staged in LDS.
// zk_expand3_subm -- zk_expand (zkwg_expand3_body.h) instantiated with the match matrix decoder (ZSEG_SUBM) beside the common
//           ones: the expansion kernel of these two mains.  The headline kernel's switch does not carry the type.
#include "zkwg_dev.h"
#include "zkwg_kernels.h"
#include "zkwg_substr_core.h"
#include "zkwg_expand3_body.h"

__global__ __launch_bounds__(64) void zk_substr(ZkSched s, ZkBufs B) {
  extern __shared__ __align__(16) u8 zk_sub_ws[];
  const u32 e = blockIdx.x;
  if (e >= B.n_emails) return;
  const u8* rec = B.in + (u64)e * s.in_stride;
  const int st = zk_substr_core(s.sub, s.m_one, s.in_off[ZK_IN_RANGE_FLAGS], rec, B.bits + (u64)e * s.img_bits,
                                B.small + (u64)e * s.img_small, zk_sub_ws);
  if (threadIdx.x == 0 && st) B.status[e] = st;
}

__global__ __launch_bounds__(256) void zk_expand3_subm(ZkX3 A) { zk_expand3_body<false, ZK_X3_SLOTS, true>(A); }
