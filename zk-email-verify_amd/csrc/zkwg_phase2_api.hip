// C-ABI of phase 2 (include/zkwg.h "phase 2"): zkwg_point_scale_device, zkwg_zkey_apply_delta_size, zkwg_zkey_apply_delta, _stats.
// Both calls are one-shot like zkwg_zkey_new: they allocate the buffers of ONE piece (ZK_PHASE2_PIECE points: 280 bytes a G1 point, 488
// a G2 point), run every piece through  curve check -> zk_phase2_scale -> denominators -> batched inversion -> affine,  synchronise and
// free everything before they return.
#include <string.h>
#include "zkwg_phase2_core.h"
#include "zkwg_points_host.h"

namespace {
thread_local ZkStats<5, 4> g_stats;

// out[i] = s in[i], n points; in / out: host memory (on_device = false: staged through the piece) or device memory.  seconds (may be
// null): {upload + curve check, scaling, conversion + download} are added to seconds[0 .. 2], a synchronisation after each stage.
int scale_points(int group, const void* in, u64 n, const ZkPhase2Digits& D, void* out, bool on_device, hipStream_t st, double* seconds) {
  if (!n) return ZKWG_RC_OK;
  const u64 pt = zk_pt_bytes(group), cap = std::min<u64>(n, ZK_PHASE2_PIECE);
  DevBufs B;                                                        // the buffers of one piece
  void *pts = B.get(cap * pt), *acc = B.get(cap * zk_acc_bytes(group));
  Fq29 *den = (Fq29*)B.get(cap * sizeof(Fq29)), *pref = (Fq29*)B.get(cap * sizeof(Fq29));
  u32* d_bad = (u32*)B.get(4);
  if (B.oom) return ZKWG_RC_OOM;
  if (hipMemset(d_bad, 0, 4) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  ZkStageClock clock(st, seconds);
  for (u64 first = 0; first < n; first += ZK_PHASE2_PIECE) {
    const u32 m = (u32)std::min<u64>(ZK_PHASE2_PIECE, n - first);
    const u8* src = (const u8*)in + first * pt;
    u8* dst = (u8*)out + first * pt;
    clock.start();
    if (!on_device && hipMemcpyAsync(pts, src, m * pt, hipMemcpyHostToDevice, st) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    zk_setup_prepare_launch(group, on_device ? (const void*)src : pts, pts, m, d_bad, st);          // -> the tables' form, in pts
    if (!clock.lap(0)) return ZKWG_RC_HIP_ERROR;
    zk_phase2_scale_launch(group, pts, acc, m, D, st);
    if (!clock.lap(1)) return ZKWG_RC_HIP_ERROR;
    zk_setup_to_affine_launch(group, acc, den, pref, nullptr, on_device ? (void*)dst : pts, m, st);
    if (!on_device && hipMemcpyAsync(dst, pts, m * pt, hipMemcpyDeviceToHost, st) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    // (the piece's buffers are reused: the next upload must not overtake this download -- same stream, so it does not)
    if (!clock.lap(2)) return ZKWG_RC_HIP_ERROR;
  }
  u32 bad = 0;
  if (zk_read_flags(st, d_bad, &bad, 1) != ZKWG_RC_OK) return ZKWG_RC_HIP_ERROR;
  return bad ? fail(NOT_ON_CURVE) : ZKWG_RC_OK;
}
}  // namespace

extern "C" {

int zkwg_point_scale_device(int device, int group, const void* d_points, uint64_t n, const uint8_t* scalar, void* d_out, void* hip_stream) {
  if (zk_bad_point_args(group, d_points, n, d_out) || !scalar) return ZKWG_RC_BAD_ARG;
  if (device < 0) return ZKWG_RC_NO_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  return scale_points(group, d_points, n, zk_phase2_recode(scalar), d_out, true, (hipStream_t)hip_stream, nullptr);
}

int zkwg_zkey_apply_delta_size(const uint8_t* zkey, uint64_t len, uint64_t section10_len, uint64_t* out_bytes) {
  if (!zkey || !out_bytes) return ZKWG_RC_BAD_ARG;
  ZkPhase2Frame F;
  std::string err;
  if (zk_phase2_frame(zkey, len, section10_len, F, err) != ZKWG_RC_OK) return fail(err);
  *out_bytes = F.out_bytes;
  return ZKWG_RC_OK;
}

int zkwg_zkey_apply_delta(int device, const uint8_t* zkey, uint64_t len, const uint8_t* k, const uint8_t* section10, uint64_t section10_len,
                          uint8_t* out, uint64_t cap, uint64_t* out_len) {
  if (!zkey || !k || !out || (section10_len && !section10)) return ZKWG_RC_BAD_ARG;
  if (device < 0) return ZKWG_RC_NO_DEVICE;
  try {
    g_stats.reset();
    double t = now();
    ZkPhase2Frame F;
    std::string err;
    if (zk_phase2_frame(zkey, len, section10_len, F, err) != ZKWG_RC_OK) return fail(err);
    if (cap < F.out_bytes) return ZKWG_RC_BAD_ARG;
    ZkPhase2Digits dk, dkinv;
    if (zk_phase2_scalars(k, dk, dkinv, err) != ZKWG_RC_OK) return fail(err);
    g_stats.ops[0] = F.H.size[8] / 64 * zk_phase2_adds(dkinv); g_stats.ops[1] = F.H.size[8] / 64 * zk_phase2_dbls(dkinv);
    g_stats.ops[2] = F.H.size[9] / 64 * zk_phase2_adds(dkinv); g_stats.ops[3] = F.H.size[9] / 64 * zk_phase2_dbls(dkinv);
    if (hipSetDevice(device) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    double host_copy = 0;
    const int rc = zk_phase2_apply(zkey, F, dk, dkinv, section10, section10_len, out, [&](int group, const u8* in, u64 n, const ZkPhase2Digits& D, u8* o, int what) {
      if (what == 0) host_copy = now() - t;          // (the first call comes after the copies of the unchanged sections)
      double s[3] = {0, 0, 0};
      const int r = scale_points(group, in, n, D, o, false, nullptr, s);
      g_stats.seconds[1] += s[0]; g_stats.seconds[what == 9 ? 3 : 2] += what == 0 ? 0 : s[1]; g_stats.seconds[4] += s[2];
      return r;
    });
    g_stats.seconds[0] = host_copy;
    if (rc == ZKWG_RC_OK && out_len) *out_len = F.out_bytes;
    return rc;
  } catch (const std::bad_alloc&) {
    return ZKWG_RC_OOM;
  }
}

void zkwg_zkey_apply_delta_stats(double seconds[5], uint64_t ops[4]) {
  g_stats.copy(seconds, ops);
}

}
