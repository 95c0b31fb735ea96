// main = CleanEmailAddress(L) (utils/email.circom:16-140; zkwg_cea_core.h has the circuit and its literal semantics):
//   zk_cea_chunks   one LANE per (email, chunk), L / 8 chunks per email: Poseidon(16) of 16 elements of encoded || decoded through the
//                   limb-form evaluator zk_rslb_chunks runs (zkwg_poseidon29.h, variant 6: state in LDS, dense mixes through the staging
//                   words), 612 S-box signals + the digest into the image's Fr area
//   zk_cea_tail     one lane per email: the Poseidon(2) merge chain, the flag scan, the four chains over powers of r, the inversion
//   zk_expand3_cea  zk_expand (zkwg_expand3_body.h) instantiated with the byte-local decoder ZSEG_CEA beside the common ones: the
//                   expansion kernel of this main.  The headline kernel's switch does not carry the type.
#include "zkwg_dev.h"
#include "zkwg_kernels.h"
#include "zkwg_cea_core.h"
#include "zkwg_expand3_body.h"

// (one wavefront per SIMD: the 39 KB of LDS state allow four per CU, and the evaluator's 124 registers leave zk_expand its wavefronts)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void zk_cea_chunks(ZkSched s, ZkBufs B) {
  __shared__ u32 st[9 * 17 * 64];
  const u32 lane = threadIdx.x;
  const u64 unit = (u64)blockIdx.x * 64 + lane;
  const u32 e = (u32)(unit / s.cea.nch), c = (u32)(unit % s.cea.nch);
  if (e >= B.n_emails) return;
  zk_cea_chunk_core<6>(s.cea, B.in + (u64)e * s.in_stride, B.frv + (u64)e * s.img_fr, c, st + lane, 64, 17 * 64, B.pos16_l29,
                  B.rs_stage + unit, (size_t)B.rs_units);
}

__global__ __launch_bounds__(64) void zk_cea_tail(ZkSched s, ZkBufs B) {
  __shared__ u32 st[9 * 3 * 64];
  const u32 lane = threadIdx.x, e = blockIdx.x * 64 + lane;
  if (e >= B.n_emails) return;
  const int status = zk_cea_tail_core(s.cea, s.m_one, s.in_off[ZK_IN_RANGE_FLAGS], B.in + (u64)e * s.in_stride, B.frv + (u64)e * s.img_fr,
                                 B.small + (u64)e * s.img_small, st + lane, 64, 3 * 64, B.pos2_l29);
  if (status) B.status[e] = status;
}

__global__ __launch_bounds__(256) void zk_expand3_cea(ZkX3 A) { zk_expand3_body<false, ZK_X3_SLOTS, false, true>(A); }
