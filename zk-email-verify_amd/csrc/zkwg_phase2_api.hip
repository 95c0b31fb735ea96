// C-ABI of phase 2 (include/zkwg.h "phase 2"): zkwg_point_scale_device, zkwg_zkey_apply_delta_size, zkwg_zkey_apply_delta, _stats.
// Both calls are one-shot like zkwg_zkey_new: they allocate the buffers of ONE piece (ZK_PHASE2_PIECE points: 280 bytes a G1 point, 488
// a G2 point), run every piece through  curve check -> zk_phase2_scale -> denominators -> batched inversion -> affine,  synchronise and
// free everything before they return.
#include <hip/hip_runtime.h>
#include <string.h>
#include <chrono>
#include <string>
#include <vector>
#include "../../include/zkwg.h"
#include "zkwg_phase2_core.h"

void zk_phase2_scale_launch(int group, const void* pts, void* acc, u32 n, const ZkPhase2Digits& D, hipStream_t st);      // zkwg_kernels_phase2.hip
void zk_setup_prepare_launch(int group, const void* in, void* out, u64 n, u32* bad, hipStream_t st);                     // zkwg_kernels_setup.hip
void zk_setup_to_affine_launch(int group, const void* acc, Fq29* den, Fq29* pref, const u32* seg_wire, void* out, u32 n, hipStream_t st);
extern "C" void zk_set_last_error(const char* m);                                                                          // zkwg_api.hip

namespace {
thread_local double g_seconds[5];
thread_local u64 g_ops[4];
int fail(const std::string& m) { zk_set_last_error(m.c_str()); return ZKWG_RC_BAD_CONFIG; }
double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
const char* const NOT_ON_CURVE = "a point is not on its curve (or not reduced)";

// the buffers of one piece
struct Piece {
  void *pts = nullptr, *acc = nullptr;
  Fq29 *den = nullptr, *pref = nullptr;
  u32* bad = nullptr;
  int alloc(int group, u64 n) {
    const u64 pt = group == 2 ? 128 : 64, xs = group == 2 ? 288 : 144;
    if (hipMalloc(&pts, n * pt) != hipSuccess || hipMalloc(&acc, n * xs) != hipSuccess || hipMalloc((void**)&den, n * sizeof(Fq29)) != hipSuccess ||
        hipMalloc((void**)&pref, n * sizeof(Fq29)) != hipSuccess || hipMalloc((void**)&bad, 4) != hipSuccess) {
      (void)hipGetLastError();
      return ZKWG_RC_OOM;
    }
    return hipMemset(bad, 0, 4) == hipSuccess ? ZKWG_RC_OK : ZKWG_RC_HIP_ERROR;
  }
  ~Piece() { hipFree(pts); hipFree(acc); hipFree(den); hipFree(pref); hipFree(bad); }
};
// out[i] = s in[i], n points; in / out: host memory (on_device = false: staged through the piece) or device memory.  seconds (may be
// null): {upload + curve check, scaling, conversion + download} are added to seconds[0 .. 2], a synchronisation after each stage.
int scale_points(int group, const void* in, u64 n, const ZkPhase2Digits& D, void* out, bool on_device, hipStream_t st, double* seconds) {
  if (!n) return ZKWG_RC_OK;
  const u64 pt = group == 2 ? 128 : 64;
  Piece B;
  int rc = B.alloc(group, std::min<u64>(n, ZK_PHASE2_PIECE));
  if (rc != ZKWG_RC_OK) return rc;
  auto stage = [&](int k, double& t) {
    if (!seconds) return true;
    if (hipStreamSynchronize(st) != hipSuccess) return false;
    seconds[k] += now() - t; t = now();
    return true;
  };
  for (u64 first = 0; first < n; first += ZK_PHASE2_PIECE) {
    const u32 m = (u32)std::min<u64>(ZK_PHASE2_PIECE, n - first);
    const u8* src = (const u8*)in + first * pt;
    u8* dst = (u8*)out + first * pt;
    double t = now();
    if (!on_device && hipMemcpyAsync(B.pts, src, m * pt, hipMemcpyHostToDevice, st) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    zk_setup_prepare_launch(group, on_device ? (const void*)src : B.pts, B.pts, m, B.bad, st);      // -> the tables' form, in B.pts
    if (!stage(0, t)) return ZKWG_RC_HIP_ERROR;
    zk_phase2_scale_launch(group, B.pts, B.acc, m, D, st);
    if (!stage(1, t)) return ZKWG_RC_HIP_ERROR;
    zk_setup_to_affine_launch(group, B.acc, B.den, B.pref, nullptr, on_device ? (void*)dst : B.pts, m, st);
    if (!on_device && hipMemcpyAsync(dst, B.pts, m * pt, hipMemcpyDeviceToHost, st) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    // (the piece's buffers are reused: the next upload must not overtake this download -- same stream, so it does not)
    if (!stage(2, t)) return ZKWG_RC_HIP_ERROR;
  }
  u32 bad = 0;
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&bad, B.bad, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  return bad ? fail(NOT_ON_CURVE) : ZKWG_RC_OK;
}
}  // namespace

extern "C" {

int zkwg_point_scale_device(int device, int group, const void* d_points, uint64_t n, const uint8_t* scalar, void* d_out, void* hip_stream) {
  if ((group != 1 && group != 2) || !scalar || (n && (!d_points || !d_out)) || ((uintptr_t)d_points & 15) || ((uintptr_t)d_out & 15)) return ZKWG_RC_BAD_ARG;
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
    for (double& s : g_seconds) s = 0;
    for (u64& o : g_ops) o = 0;
    double t = now();
    ZkPhase2Frame F;
    std::string err;
    if (zk_phase2_frame(zkey, len, section10_len, F, err) != ZKWG_RC_OK) return fail(err);
    if (cap < F.out_bytes) return ZKWG_RC_BAD_ARG;
    ZkPhase2Digits dk, dkinv;
    if (zk_phase2_scalars(k, dk, dkinv, err) != ZKWG_RC_OK) return fail(err);
    g_ops[0] = F.H.size[8] / 64 * zk_phase2_adds(dkinv); g_ops[1] = F.H.size[8] / 64 * zk_phase2_dbls(dkinv);
    g_ops[2] = F.H.size[9] / 64 * zk_phase2_adds(dkinv); g_ops[3] = F.H.size[9] / 64 * zk_phase2_dbls(dkinv);
    if (hipSetDevice(device) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    double host_copy = 0;
    const int rc = zk_phase2_apply(zkey, F, dk, dkinv, section10, section10_len, out, [&](int group, const u8* in, u64 n, const ZkPhase2Digits& D, u8* o, int what) {
      if (what == 0) host_copy = now() - t;          // (the first call comes after the copies of the unchanged sections)
      double s[3] = {0, 0, 0};
      const int r = scale_points(group, in, n, D, o, false, nullptr, s);
      g_seconds[1] += s[0]; g_seconds[what == 9 ? 3 : 2] += what == 0 ? 0 : s[1]; g_seconds[4] += s[2];
      return r;
    });
    g_seconds[0] = host_copy;
    if (rc == ZKWG_RC_OK && out_len) *out_len = F.out_bytes;
    return rc;
  } catch (const std::bad_alloc&) {
    return ZKWG_RC_OOM;
  }
}

void zkwg_zkey_apply_delta_stats(double seconds[5], uint64_t ops[4]) {
  if (seconds) for (int i = 0; i < 5; ++i) seconds[i] = g_seconds[i];
  if (ops) for (int i = 0; i < 4; ++i) ops[i] = g_ops[i];
}

}
