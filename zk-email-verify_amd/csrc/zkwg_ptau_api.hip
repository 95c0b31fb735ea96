// C-ABI of the powers-of-tau preparation (include/zkwg.h "prepare phase 2"): zkwg_group_ntt_device, zkwg_ptau_prepare_size,
// zkwg_ptau_prepare, _stats.  Both calls are one-shot like zkwg_zkey_new: they build the table of recoded twiddles on the host, allocate
// the buffers of the largest transform (312 bytes a G1 point, 520 a G2 point; the file operation: 64 / 128 more for the section in the
// tables' form), run every transform as the launch series
//   zk_phase2_scale (2^-L) -> affine -> permutation -> per stage: zk_ptau_stage -> denominators -> batched inversion -> affine -> tables' form
// synchronise and free everything before they return.
#include <hip/hip_runtime.h>
#include <string.h>
#include <chrono>
#include <string>
#include <vector>
#include "../../include/zkwg.h"
#include "zkwg_ptau_core.h"

void zk_ptau_stage_launch(int group, const void* pts, void* acc, const ZkPtauTw* tw, u32 L, u32 s, u32 table_L, hipStream_t st);      // zkwg_kernels_ptau.hip
void zk_ptau_permute_launch(int group, void* pts, u32 L, hipStream_t st);
void zk_phase2_scale_launch(int group, const void* pts, void* acc, u32 n, const ZkPhase2Digits& D, hipStream_t st);                    // zkwg_kernels_phase2.hip
void zk_setup_prepare_launch(int group, const void* in, void* out, u64 n, u32* bad, hipStream_t st);                                   // zkwg_kernels_setup.hip
void zk_setup_to_affine_launch(int group, const void* acc, Fq29* den, Fq29* pref, const u32* seg_wire, void* out, u32 n, hipStream_t st);
extern "C" void zk_set_last_error(const char* m);                                                                                        // zkwg_api.hip

namespace {
thread_local double g_seconds[12 + 4 * 32];       // per section three stages, then per section and level the transform's seconds
thread_local u64 g_ops[8];
int fail(const std::string& m) { zk_set_last_error(m.c_str()); return ZKWG_RC_BAD_CONFIG; }
double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
const char* const NOT_ON_CURVE = "a point is not on its curve (or not reduced)";

// the buffers of one transform of n points, and the table
struct Work {
  void *pts = nullptr, *acc = nullptr, *src = nullptr;
  Fq29 *den = nullptr, *pref = nullptr;
  u32* bad = nullptr;                   // [0]: an input point failed its check; [1]: an intermediate point did (never: an internal error)
  int alloc(int group, u64 n, bool with_src) {
    const u64 pt = group == 2 ? 128 : 64, xs = group == 2 ? 288 : 144;
    if (hipMalloc(&pts, n * pt) != hipSuccess || hipMalloc(&acc, n * xs) != hipSuccess || hipMalloc((void**)&den, n * sizeof(Fq29)) != hipSuccess ||
        hipMalloc((void**)&pref, n * sizeof(Fq29)) != hipSuccess || hipMalloc((void**)&bad, 8) != hipSuccess || (with_src && hipMalloc(&src, n * pt) != hipSuccess)) {
      (void)hipGetLastError();
      return ZKWG_RC_OOM;
    }
    return hipMemset(bad, 0, 8) == hipSuccess ? ZKWG_RC_OK : ZKWG_RC_HIP_ERROR;
  }
  ~Work() { hipFree(pts); hipFree(acc); hipFree(src); hipFree(den); hipFree(pref); hipFree(bad); }
};
struct DeviceTable {
  ZkPtauTw* d = nullptr;
  int upload(const ZkPtauTable& T) {
    if (hipMalloc((void**)&d, T.tw.size() * sizeof(ZkPtauTw)) != hipSuccess) { (void)hipGetLastError(); return ZKWG_RC_OOM; }
    return hipMemcpy(d, T.tw.data(), T.tw.size() * sizeof(ZkPtauTw), hipMemcpyHostToDevice) == hipSuccess ? ZKWG_RC_OK : ZKWG_RC_HIP_ERROR;
  }
  ~DeviceTable() { hipFree(d); }
};
// the launches of one 2^q-point transform up to its last stage's butterflies: table-form points at src (may be W.pts) -> accumulators
// at W.acc, which finish() turns into the zkey-form points at W.pts
void transform(int group, const void* src, u32 q, Work& W, const ZkPtauTable& T, const ZkPtauTw* d_tw, hipStream_t st) {
  const u32 n = 1u << q;
  u8 k[32] = {1};
  if (T.inverse) zk_ptau_ninv(q, k);
  zk_phase2_scale_launch(group, src, W.acc, n, zk_phase2_recode(k), st);
  for (u32 s = 0; s < q; ++s) {
    zk_setup_to_affine_launch(group, W.acc, W.den, W.pref, nullptr, W.pts, n, st);
    zk_setup_prepare_launch(group, W.pts, W.pts, n, W.bad + 1, st);
    if (s == 0) zk_ptau_permute_launch(group, W.pts, q, st);
    zk_ptau_stage_launch(group, W.pts, W.acc, d_tw, q, s, T.L, st);
  }
}
void finish(int group, u32 q, Work& W, hipStream_t st) { zk_setup_to_affine_launch(group, W.acc, W.den, W.pref, nullptr, W.pts, 1u << q, st); }
int check(Work& W, hipStream_t st) {
  u32 bad[2] = {0, 0};
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(bad, W.bad, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  if (bad[0]) return fail(NOT_ON_CURVE);
  if (bad[1]) { zk_set_last_error("internal: an intermediate point of the transform is not on its curve"); return ZKWG_RC_HIP_ERROR; }
  return ZKWG_RC_OK;
}
int refuse_size(int group, u32 log2_n) {
  if (log2_n <= (group == 2 ? ZK_PTAU_MAX_LOG2_G2 : ZK_PTAU_MAX_LOG2_G1)) return ZKWG_RC_OK;
  return fail(group == 2 ? "a transform of more than 2^28 G2 points is not accepted (520 bytes of device memory a point)"
                         : "a transform of more than 2^29 G1 points is not accepted (312 bytes of device memory a point)");
}
}  // namespace

extern "C" {

int zkwg_group_ntt_device(int device, int group, void* d_points, uint32_t log2_n, int inverse, void* hip_stream) {
  if ((group != 1 && group != 2) || !d_points || ((uintptr_t)d_points & 15) || log2_n > 31) return ZKWG_RC_BAD_ARG;
  if (device < 0) return ZKWG_RC_NO_DEVICE;
  if (refuse_size(group, log2_n) != ZKWG_RC_OK) return ZKWG_RC_BAD_CONFIG;
  try {
    if (hipSetDevice(device) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    hipStream_t st = (hipStream_t)hip_stream;
    const u64 n = 1ull << log2_n, pt = group == 2 ? 128 : 64;
    ZkPtauTable T;
    zk_ptau_table(log2_n, inverse != 0, T);
    DeviceTable dt;
    Work W;
    int rc = dt.upload(T);
    if (rc == ZKWG_RC_OK) rc = W.alloc(group, n, false);
    if (rc != ZKWG_RC_OK) return rc;
    zk_setup_prepare_launch(group, d_points, W.pts, n, W.bad, st);
    if ((rc = check(W, st)) != ZKWG_RC_OK) return rc;          // (refused before anything is computed from a bad point; d_points stay as they were)
    transform(group, W.pts, log2_n, W, T, dt.d, st);
    finish(group, log2_n, W, st);
    if ((rc = check(W, st)) != ZKWG_RC_OK) return rc;
    if (hipMemcpyAsync(d_points, W.pts, n * pt, hipMemcpyDeviceToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    return ZKWG_RC_OK;
  } catch (const std::bad_alloc&) {
    return ZKWG_RC_OOM;
  }
}

int zkwg_ptau_prepare_size(const uint8_t* ptau, uint64_t len, uint32_t power, uint64_t* out_bytes) {
  if (!ptau || !out_bytes) return ZKWG_RC_BAD_ARG;
  ZkPtauFrame F;
  std::string err;
  if (zk_ptau_frame(ptau, len, power, F, err) != ZKWG_RC_OK) return fail(err);
  *out_bytes = F.out_bytes;
  return ZKWG_RC_OK;
}

int zkwg_ptau_prepare(int device, const uint8_t* ptau, uint64_t len, uint32_t power, uint8_t* out, uint64_t cap, uint64_t* out_len) {
  if (!ptau || !out) return ZKWG_RC_BAD_ARG;
  if (device < 0) return ZKWG_RC_NO_DEVICE;
  try {
    for (double& s : g_seconds) s = 0;
    for (u64& o : g_ops) o = 0;
    ZkPtauFrame F;
    std::string err;
    if (zk_ptau_frame(ptau, len, power, F, err) != ZKWG_RC_OK) return fail(err);
    if (cap < F.out_bytes) return ZKWG_RC_BAD_ARG;
    if (refuse_size(1, F.power + 1) != ZKWG_RC_OK || refuse_size(2, F.power) != ZKWG_RC_OK) return ZKWG_RC_BAD_CONFIG;
    if (hipSetDevice(device) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    hipStream_t st = nullptr;
    ZkPtauTable T;
    zk_ptau_table(F.power + 1, true, T);
    DeviceTable dt;
    int rc = dt.upload(T);
    if (rc != ZKWG_RC_OK) return rc;
    int which = 0;
    rc = zk_ptau_prepare_apply(ptau, F, out, [&](int group, const u8* in, u64 count, u32 top, u8* o) {
      double* sec = g_seconds + 3 * which;
      u64* ops = g_ops + 2 * which;
      ++which;
      const u64 n = 1ull << top, pt = group == 2 ? 128 : 64;
      Work W;
      int r = W.alloc(group, n, true);
      if (r != ZKWG_RC_OK) return r;
      double t = now();
      if (hipMemcpyAsync(W.src, in, count * pt, hipMemcpyHostToDevice, st) != hipSuccess) return (int)ZKWG_RC_HIP_ERROR;
      if (count < n && hipMemsetAsync((u8*)W.src + count * pt, 0, (n - count) * pt, st) != hipSuccess) return (int)ZKWG_RC_HIP_ERROR;        // the padded level's point at infinity
      zk_setup_prepare_launch(group, W.src, W.src, n, W.bad, st);
      if ((r = check(W, st)) != ZKWG_RC_OK) return r;
      sec[0] += now() - t;
      for (u32 q = 0; q <= top; ++q) {
        t = now();
        transform(group, W.src, q, W, T, dt.d, st);
        if (hipStreamSynchronize(st) != hipSuccess) return (int)ZKWG_RC_HIP_ERROR;
        sec[1] += now() - t; g_seconds[12 + 32 * (which - 1) + q] = now() - t; t = now();
        finish(group, q, W, st);
        if (hipMemcpyAsync(o + ((1ull << q) - 1) * pt, W.pts, pt << q, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return (int)ZKWG_RC_HIP_ERROR;
        sec[2] += now() - t;
        zk_ptau_ops(T, q, true, ops[0], ops[1]);
      }
      return check(W, st);
    });
    if (rc == ZKWG_RC_OK && out_len) *out_len = F.out_bytes;
    return rc;
  } catch (const std::bad_alloc&) {
    return ZKWG_RC_OOM;
  }
}

void zkwg_ptau_prepare_stats(double seconds[140], uint64_t ops[8]) {
  if (seconds) for (int i = 0; i < 140; ++i) seconds[i] = g_seconds[i];
  if (ops) for (int i = 0; i < 8; ++i) ops[i] = g_ops[i];
}

}
