// C-ABI of `powersoftau verify` (include/zkwg.h "powers of tau: verification"): zkwg_pairing_check (host only: csrc/zkwg_pairing.h),
// zkwg_g2_subgroup_device (csrc/zkwg_verify_core.h on lane pairs) and zkwg_point_rlc_device / zkwg_point_rlc32_device, the sums
// sum_i s_i P_i that fold a section into the two points of one pairing check.  The device calls are one-shot like zkwg_point_scale_device:
// they allocate what one piece needs, synchronise and free everything before they return.
//
// The sums are NOT a second bucket method: every piece is one multi-exponentiation plan in the classic layout (zkwg_msm_create_ex with
// bases on the device and a table budget too small for shifted copies: K bucket sets and a Horner pass -- right for bases used once).
// The plan converts its piece of the points into a table of its own, so the two arrays of a call may overlap (d_b = d_a + one point: the
// shifted form of the powers checks); the partial sums of the pieces are added on the host (zkwg_g1.h / zkwg_g2.h).
#include <string.h>
#include <algorithm>
#include "zkwg_pairing.h"
#include "zkwg_points_host.h"

namespace {
#define ZK_VERIFY_RLC_PIECE (1ull << 22)

// the multi-exponentiation plan of one piece: destroyed on every way out
struct Plan {
  zkwg_msm_t* p = nullptr;
  ~Plan() { if (p) zkwg_msm_destroy(p); }
};

// the host accumulator of the pieces' partial sums
struct Sum {
  G1Xyzz a1 = g1_xyzz_inf();
  G2Xyzz a2 = g2_xyzz_inf();
  void add(int group, const u8* pt) {
    if (group == 1) { G1Affine p; memcpy((void*)&p, pt, 64); a1 = g1_add(a1, g1_from_affine(p)); }
    else { G2Affine p; memcpy((void*)&p, pt, 128); if (!g2_is_inf(p)) a2 = g2_add(a2, G2Xyzz{p.x, p.y, fq2_one(), fq2_one()}); }
  }
  void store(int group, u8* out) const {
    if (group == 1) { const G1Affine p = g1_to_affine(a1); memcpy(out, (const void*)&p, 64); }
    else { const G2Affine p = g2_to_affine(a2); memcpy(out, (const void*)&p, 128); }
  }
};

int rlc(int device, int group, const void* d_a, const void* d_b, u64 n, const void* d_scalars, u32 scalar_bytes, u64 piece_points, u8* out_a, u8* out_b, hipStream_t st) {
  const u64 pt = zk_pt_bytes(group);
  if (zk_bad_point_args(group, d_a, n, d_scalars) || !out_a || (d_b && !out_b) || ((uintptr_t)d_b & 15) || piece_points >= (1ull << 31)) return ZKWG_RC_BAD_ARG;
  if (device < 0) return ZKWG_RC_NO_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  const u64 piece = piece_points ? piece_points : ZK_VERIFY_RLC_PIECE;
  Sum sa, sb;
  if (n) {
    DevBufs B;
    Plan plan;
    u32* d_bad = (u32*)B.get(4);
    void *wide = scalar_bytes == 16 ? B.get(std::min(n, piece) * 32) : nullptr, *work = nullptr;
    if (B.oom) return ZKWG_RC_OOM;
    if (hipMemsetAsync(d_bad, 0, 4, st) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    // every point of both arrays is checked before anything is summed
    zk_setup_prepare_launch(group, d_a, nullptr, n, d_bad, st);
    if (d_b) zk_setup_prepare_launch(group, d_b, nullptr, n, d_bad, st);
    u32 bad = 0;
    if (zk_read_flags(st, d_bad, &bad, 1) != ZKWG_RC_OK) return ZKWG_RC_HIP_ERROR;
    if (bad) return fail(NOT_ON_CURVE);
    u64 work_for = 0;
    for (u64 at = 0; at < n; at += piece) {
      const u64 m = std::min(piece, n - at);
      const void* s = (const u8*)d_scalars + at * scalar_bytes;
      if (scalar_bytes == 16) { zk_verify_widen_launch(s, wide, m, st); s = wide; }
      for (int which = 0; which < (d_b ? 2 : 1); ++which) {
        const u8* base = (const u8*)(which ? d_b : d_a) + at * pt;
        int rc = zkwg_msm_create_ex(device, group, base, 1, m, 0, 0, 1, &plan.p);       // (a budget of one byte: the classic layout)
        if (rc != ZKWG_RC_OK) return rc;
        if (work_for != m) {                                                           // (the layout depends on the group and the count only)
          B.drop(work);
          work = B.get(zkwg_msm_work_bytes(plan.p));
          if (B.oom) return ZKWG_RC_OOM;
          work_for = m;
        }
        u8 part[128];
        rc = group == 1 ? zkwg_msm_g1_device(plan.p, s, 0, 0, work, part, st) : zkwg_msm_g2_device(plan.p, s, 0, 0, work, part, st);
        zkwg_msm_destroy(plan.p); plan.p = nullptr;
        if (rc != ZKWG_RC_OK) return rc;
        (which ? sb : sa).add(group, part);
      }
    }
  }
  sa.store(group, out_a);
  if (d_b) sb.store(group, out_b);
  return ZKWG_RC_OK;
}
}  // namespace

extern "C" {

#if !defined(__HIP_DEVICE_COMPILE__)
int zkwg_pairing_check(const uint8_t* g1, const uint8_t* g2, uint32_t n, int* is_one) {
  if (!is_one || (n && (!g1 || !g2))) return ZKWG_RC_BAD_ARG;
  try {
    Fq12 f;
    std::string err;
    if (zk_pairing_product(g1, g2, n, f, err) != ZKWG_RC_OK) return fail(err);
    *is_one = fq12_eq(f, fq12_one()) ? 1 : 0;
    return ZKWG_RC_OK;
  } catch (const std::bad_alloc&) {
    return ZKWG_RC_OOM;
  }
}
#endif

int zkwg_g2_subgroup_device(int device, const void* d_points, uint64_t n, uint64_t* n_bad, uint64_t* first_bad, void* hip_stream) {
  if (!n_bad || !first_bad || zk_bad_point_args(2, d_points, n, d_points)) return ZKWG_RC_BAD_ARG;
  if (device < 0) return ZKWG_RC_NO_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  *n_bad = 0;
  if (!n) return ZKWG_RC_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  DevBufs B;
  void* tab = B.get(std::min<u64>(n, ZK_VERIFY_PIECE) * 128);
  u32* d_flags = (u32*)B.get(12);
  if (B.oom) return ZKWG_RC_OOM;
  const ZkPhase2Digits Du = zk_verify_u_digits();
  bool found = false;
  for (u64 at = 0; at < n; at += ZK_VERIFY_PIECE) {
    const u32 m = (u32)std::min<u64>(ZK_VERIFY_PIECE, n - at);
    u32 flags[3] = {0, 0, 0xffffffffu};                          // off the curve | outside the subgroup | the lowest index of one
    if (hipMemcpyAsync(d_flags, flags, 12, hipMemcpyHostToDevice, st) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    zk_setup_prepare_launch(2, (const u8*)d_points + at * 128, tab, m, d_flags, st);        // the curve check; -> the tables' form
    zk_verify_g2_subgroup_launch(tab, m, Du, d_flags + 1, st);
    if (zk_read_flags(st, d_flags, flags, 3) != ZKWG_RC_OK) return ZKWG_RC_HIP_ERROR;
    if (flags[0]) return fail(NOT_ON_CURVE);
    if (flags[1] && !found) { *first_bad = at + flags[2]; found = true; }
    *n_bad += flags[1];
  }
  return ZKWG_RC_OK;
}

int zkwg_point_rlc_device(int device, int group, const void* d_a, const void* d_b, uint64_t n, const void* d_scalars, uint64_t piece_points,
                          uint8_t* out_a, uint8_t* out_b, void* hip_stream) {
  return rlc(device, group, d_a, d_b, n, d_scalars, 16, piece_points, out_a, out_b, (hipStream_t)hip_stream);
}
int zkwg_point_rlc32_device(int device, int group, const void* d_a, const void* d_b, uint64_t n, const void* d_scalars, uint64_t piece_points,
                            uint8_t* out_a, uint8_t* out_b, void* hip_stream) {
  return rlc(device, group, d_a, d_b, n, d_scalars, 32, piece_points, out_a, out_b, (hipStream_t)hip_stream);
}

}
