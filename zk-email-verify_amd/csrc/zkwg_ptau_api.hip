// C-ABI of the powers-of-tau preparation (include/zkwg.h "prepare phase 2"): zkwg_group_ntt_device, zkwg_ptau_prepare_size,
// zkwg_ptau_prepare, _stats.  Both calls are one-shot like zkwg_zkey_new: they build the table of recoded twiddles on the host, allocate
// the buffers of the largest transform (312 bytes a G1 point, 520 a G2 point; the file operation: 64 / 128 more for the section in the
// tables' form), run every transform as the launch series
//   zk_phase2_scale (2^-L) -> affine -> permutation -> per stage: zk_ptau_stage -> denominators -> batched inversion -> affine -> tables' form
// synchronise and free everything before they return.
#include <string.h>
#include "zkwg_ptau_core.h"
#include "zkwg_points_host.h"

namespace {
thread_local ZkStats<12 + 4 * 32, 8> g_stats;       // seconds: per section three stages, then per section and level the transform's seconds

// the buffers of one transform of n points (owned by B)
struct Work {
  void *pts, *acc, *src;
  Fq29 *den, *pref;
  u32* bad;                             // [0]: an input point failed its check; [1]: an intermediate point did (never: an internal error)
};
int alloc(DevBufs& B, Work& W, int group, u64 n, bool with_src) {
  const u64 pt = zk_pt_bytes(group);
  W.pts = B.get(n * pt); W.acc = B.get(n * zk_acc_bytes(group));
  W.den = (Fq29*)B.get(n * sizeof(Fq29)); W.pref = (Fq29*)B.get(n * sizeof(Fq29));
  W.bad = (u32*)B.get(8);
  W.src = with_src ? B.get(n * pt) : nullptr;
  if (B.oom) return ZKWG_RC_OOM;
  return hipMemset(W.bad, 0, 8) == hipSuccess ? ZKWG_RC_OK : ZKWG_RC_HIP_ERROR;
}
// the table of recoded twiddles on the device
int upload(DevBufs& B, const ZkPtauTable& T, ZkPtauTw*& d_tw) {
  d_tw = T.tw.empty() ? nullptr : (ZkPtauTw*)B.get(T.tw.size() * sizeof(ZkPtauTw));      // (a transform of one point has no table)
  if (B.oom) return ZKWG_RC_OOM;
  return hipMemcpy(d_tw, T.tw.data(), T.tw.size() * sizeof(ZkPtauTw), hipMemcpyHostToDevice) == hipSuccess ? ZKWG_RC_OK : ZKWG_RC_HIP_ERROR;
}
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
  if (zk_read_flags(st, W.bad, bad, 2) != ZKWG_RC_OK) return ZKWG_RC_HIP_ERROR;
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
  if (zk_bad_point_args(group, d_points, 1, d_points) || log2_n > 31) return ZKWG_RC_BAD_ARG;
  if (device < 0) return ZKWG_RC_NO_DEVICE;
  if (refuse_size(group, log2_n) != ZKWG_RC_OK) return ZKWG_RC_BAD_CONFIG;
  try {
    if (hipSetDevice(device) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    hipStream_t st = (hipStream_t)hip_stream;
    const u64 n = 1ull << log2_n, pt = zk_pt_bytes(group);
    ZkPtauTable T;
    zk_ptau_table(log2_n, inverse != 0, T);
    DevBufs B;
    ZkPtauTw* d_tw;
    Work W;
    int rc = upload(B, T, d_tw);
    if (rc == ZKWG_RC_OK) rc = alloc(B, W, group, n, false);
    if (rc != ZKWG_RC_OK) return rc;
    zk_setup_prepare_launch(group, d_points, W.pts, n, W.bad, st);
    if ((rc = check(W, st)) != ZKWG_RC_OK) return rc;          // (refused before anything is computed from a bad point; d_points stay as they were)
    transform(group, W.pts, log2_n, W, T, d_tw, st);
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
    g_stats.reset();
    ZkPtauFrame F;
    std::string err;
    if (zk_ptau_frame(ptau, len, power, F, err) != ZKWG_RC_OK) return fail(err);
    if (cap < F.out_bytes) return ZKWG_RC_BAD_ARG;
    if (refuse_size(1, F.power + 1) != ZKWG_RC_OK || refuse_size(2, F.power) != ZKWG_RC_OK) return ZKWG_RC_BAD_CONFIG;
    if (hipSetDevice(device) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    hipStream_t st = nullptr;
    ZkPtauTable T;
    zk_ptau_table(F.power + 1, true, T);
    DevBufs table;
    ZkPtauTw* d_tw;
    int rc = upload(table, T, d_tw);
    if (rc != ZKWG_RC_OK) return rc;
    int which = 0;
    rc = zk_ptau_prepare_apply(ptau, F, out, [&](int group, const u8* in, u64 count, u32 top, u8* o) {
      double* sec = g_stats.seconds + 3 * which;
      u64* ops = g_stats.ops + 2 * which;
      ++which;
      const u64 n = 1ull << top, pt = zk_pt_bytes(group);
      DevBufs B;
      Work W;
      int r = alloc(B, W, group, n, true);
      if (r != ZKWG_RC_OK) return r;
      ZkStageClock clock(st, sec);
      if (hipMemcpyAsync(W.src, in, count * pt, hipMemcpyHostToDevice, st) != hipSuccess) return (int)ZKWG_RC_HIP_ERROR;
      if (count < n && hipMemsetAsync((u8*)W.src + count * pt, 0, (n - count) * pt, st) != hipSuccess) return (int)ZKWG_RC_HIP_ERROR;        // the padded level's point at infinity
      zk_setup_prepare_launch(group, W.src, W.src, n, W.bad, st);
      if ((r = check(W, st)) != ZKWG_RC_OK) return r;
      sec[0] += now() - clock.t;                               // (check has synchronised)
      for (u32 q = 0; q <= top; ++q) {
        const double before = sec[1];
        clock.start();
        transform(group, W.src, q, W, T, d_tw, st);
        if (!clock.lap(1)) return (int)ZKWG_RC_HIP_ERROR;
        g_stats.seconds[12 + 32 * (which - 1) + q] = sec[1] - before;
        finish(group, q, W, st);
        if (hipMemcpyAsync(o + ((1ull << q) - 1) * pt, W.pts, pt << q, hipMemcpyDeviceToHost, st) != hipSuccess || !clock.lap(2)) return (int)ZKWG_RC_HIP_ERROR;
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
  g_stats.copy(seconds, ops);
}

}
