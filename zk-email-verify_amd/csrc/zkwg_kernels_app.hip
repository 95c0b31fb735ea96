// zk_app_tail -- main = EmailReveal(...) (circuits/email-reveal.circom): the packed revealed bytes and the email nullifier
//           with its 636 S-box signals (zkwg_app_core.h), one LANE per email as zk_poseidon9 runs the same sparse-round
//           evaluator: the state and the dense mixes' temporaries are LDS columns, one per lane (40 KiB per wavefront), so no
//           lane-indexed array ends up in scratch memory.  It reads the input record only: EmailVerifier's roles and
//           zk_substr (the RevealSubstring component, unchanged) run beside it.
// The expansion kernels of this main are zk_expand3 (no match matrix) and zk_expand3_subm (check_uniqueness: the layout has
// a ZSEG_SUBM segment); both carry every other segment type of the layout.
#include "zkwg_dev.h"
#include "zkwg_kernels.h"
#include "zkwg_app_core.h"

__global__ __launch_bounds__(64) void zk_app_tail(ZkSched s, ZkBufs B) {
  __shared__ Fr st[10 * 64];
  __shared__ Fr tmp[10 * 64];
  const u32 lane = threadIdx.x;
  const u32 e = blockIdx.x * 64u + lane;
  if (e >= B.n_emails) return;        // (no barrier below: a lane only touches its own columns)
  zk_app_core(s.app, B.in + (u64)e * s.in_stride, B.frv + (u64)e * s.img_fr, B.pos_c, B.pos1, st + lane, tmp + lane, 64u);
}
