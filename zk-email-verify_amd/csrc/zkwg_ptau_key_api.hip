// C-ABI of "each point times its own scalar" and of a powers-of-tau contribution (include/zkwg.h "powers of tau: a contribution"):
// zkwg_point_mul_device, zkwg_point_powers_device, zkwg_ptau_apply_key_size, zkwg_ptau_apply_key, _stats.  One-shot calls like
// zkwg_point_scale_device: they allocate the buffers of ONE piece (2^20 G1 / 2^19 G2 points: 2,024 / 3,544 bytes a point), check EVERY
// point on its curve before anything is written, run every piece through
//   tables' form -> zk_ptau_key_table -> affine -> tables' form -> zk_ptau_key_walk -> affine
// synchronise and free everything before they return.
#include <string.h>
#include "zkwg_ptau_key_core.h"
#include "zkwg_points_host.h"

namespace {
thread_local ZkStats<18, 8> g_stats;

// out[i] = k_i in[i], n points; k_i = scalars[i] (device memory, 32 bytes each), or c t^(first + i) from T when scalars is null.
// in / out: device memory (on_device) or host memory, staged through the piece.  seconds (may be null): {upload + curve check, tables,
// walk, conversion + download} are added to seconds[0 .. 3], a synchronisation after each stage.
int mul_points(int group, const void* in, u64 n, const void* scalars, const ZkKeyPowers* T, u64 first, void* out, bool on_device, hipStream_t st, double* seconds) {
  if (!n) return ZKWG_RC_OK;
  const u64 pt = zk_pt_bytes(group), xs = zk_acc_bytes(group), piece = group == 2 ? ZK_KEY_PIECE_G2 : ZK_KEY_PIECE_G1;
  const u64 cap = std::min<u64>(n, piece), rows_n = (ZK_KEY_ROWS - 1) * cap;
  // the buffers of one piece: the table T[row][point]; the accumulators of rows 1 - 7; the host points of a piece
  DevBufs B;
  void *tab = B.get(ZK_KEY_ROWS * cap * pt), *acc = B.get(rows_n * xs);
  Fq29 *den = (Fq29*)B.get(rows_n * sizeof(Fq29)), *pref = (Fq29*)B.get(rows_n * sizeof(Fq29));
  ZkKeyPowers* powers = (ZkKeyPowers*)B.get(sizeof(ZkKeyPowers));
  u32* d_bad = (u32*)B.get(8);          // [0]: an input point failed its check; [1]: a row of a table did (never: an internal error)
  void* stage = on_device ? nullptr : B.get(cap * pt);
  if (B.oom) return ZKWG_RC_OOM;
  if (hipMemset(d_bad, 0, 8) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  if (T && hipMemcpyAsync(powers, T, sizeof(ZkKeyPowers), hipMemcpyHostToDevice, st) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  u32 bad[2] = {0, 0};
  ZkStageClock clock(st, seconds);
  // every point is checked before the first is written (out may be in: a refusal leaves the points as they were)
  for (u64 at = 0; at < n; at += piece) {
    const u64 m = std::min<u64>(piece, n - at);
    const u8* src = (const u8*)in + at * pt;
    if (!on_device && hipMemcpyAsync(stage, src, m * pt, hipMemcpyHostToDevice, st) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    zk_setup_prepare_launch(group, on_device ? (const void*)src : stage, tab, m, d_bad, st);
  }
  if (zk_read_flags(st, d_bad, bad, 2) != ZKWG_RC_OK) return ZKWG_RC_HIP_ERROR;
  if (bad[0]) return fail(NOT_ON_CURVE);
  if (!clock.lap(0)) return ZKWG_RC_HIP_ERROR;
  for (u64 at = 0; at < n; at += piece) {
    const u32 m = (u32)std::min<u64>(piece, n - at);
    const u8* src = (const u8*)in + at * pt;
    u8* dst = (u8*)out + at * pt;
    u8* rows = (u8*)tab + (u64)m * pt;                              // rows 1 - 7
    if (n > piece) {                                                // (a single piece is in row 0 since its check)
      if (!on_device && hipMemcpyAsync(stage, src, m * pt, hipMemcpyHostToDevice, st) != hipSuccess) return ZKWG_RC_HIP_ERROR;
      zk_setup_prepare_launch(group, on_device ? (const void*)src : stage, tab, m, d_bad, st);
    }
    if (!clock.lap(0)) return ZKWG_RC_HIP_ERROR;
    zk_ptau_key_table_launch(group, tab, acc, m, st);
    zk_setup_to_affine_launch(group, acc, den, pref, nullptr, rows, (ZK_KEY_ROWS - 1) * m, st);
    zk_setup_prepare_launch(group, rows, rows, (u64)(ZK_KEY_ROWS - 1) * m, d_bad + 1, st);
    if (!clock.lap(1)) return ZKWG_RC_HIP_ERROR;
    zk_ptau_key_walk_launch(group, tab, acc, m, scalars ? (const u8*)scalars + at * 32 : nullptr, powers, first + at, st);
    if (!clock.lap(2)) return ZKWG_RC_HIP_ERROR;
    zk_setup_to_affine_launch(group, acc, den, pref, nullptr, on_device ? (void*)dst : stage, m, st);
    if (!on_device && (hipMemcpyAsync(dst, stage, m * pt, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)) return ZKWG_RC_HIP_ERROR;
    if (!clock.lap(3)) return ZKWG_RC_HIP_ERROR;
  }
  if (zk_read_flags(st, d_bad, bad, 2) != ZKWG_RC_OK) return ZKWG_RC_HIP_ERROR;
  if (bad[1]) { zk_set_last_error("internal: a row of a point's table is not on its curve"); return ZKWG_RC_HIP_ERROR; }
  return ZKWG_RC_OK;
}
}  // namespace

extern "C" {

int zkwg_point_mul_device(int device, int group, const void* d_points, uint64_t n, const void* d_scalars, void* d_out, void* hip_stream) {
  if (zk_bad_point_args(group, d_points, n, d_out) || (n && !d_scalars) || ((uintptr_t)d_scalars & 15)) return ZKWG_RC_BAD_ARG;
  if (device < 0) return ZKWG_RC_NO_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  return mul_points(group, d_points, n, d_scalars, nullptr, 0, d_out, true, (hipStream_t)hip_stream, nullptr);
}

int zkwg_point_powers_device(int device, int group, const void* d_points, uint64_t n, const uint8_t* c, const uint8_t* t, uint64_t first, void* d_out, void* hip_stream) {
  if (zk_bad_point_args(group, d_points, n, d_out) || !c || !t || first + n < first) return ZKWG_RC_BAD_ARG;
  if (device < 0) return ZKWG_RC_NO_DEVICE;
  ZkKeyPowers T;
  if (!zk_key_powers_table(c, t, T)) return fail("the scalars c and t must not be 0 modulo the group order");
  if (hipSetDevice(device) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  return mul_points(group, d_points, n, nullptr, &T, first, d_out, true, (hipStream_t)hip_stream, nullptr);
}

int zkwg_ptau_apply_key_size(const uint8_t* ptau, uint64_t len, uint64_t section7_len, uint64_t* out_bytes) {
  if (!ptau || !out_bytes) return ZKWG_RC_BAD_ARG;
  ZkPtauKeyFrame F;
  std::string err;
  if (zk_ptau_key_frame(ptau, len, section7_len, F, err) != ZKWG_RC_OK) return fail(err);
  *out_bytes = F.out_bytes;
  return ZKWG_RC_OK;
}

int zkwg_ptau_apply_key(int device, const uint8_t* ptau, uint64_t len, const uint8_t* tau, const uint8_t* alpha, const uint8_t* beta,
                        const uint8_t* section7, uint64_t section7_len, uint8_t* out, uint64_t cap, uint64_t* out_len) {
  if (!ptau || !tau || !alpha || !beta || !out || (section7_len && !section7)) return ZKWG_RC_BAD_ARG;
  if (device < 0) return ZKWG_RC_NO_DEVICE;
  try {
    g_stats.reset();
    double t0 = now();
    ZkPtauKeyFrame F;
    std::string err;
    if (zk_ptau_key_frame(ptau, len, section7_len, F, err) != ZKWG_RC_OK) return fail(err);
    if (cap < F.out_bytes) return ZKWG_RC_BAD_ARG;
    ZkPtauKey K;
    if (zk_ptau_key_scalars(tau, alpha, beta, K, err) != ZKWG_RC_OK) return fail(err);
    if (hipSetDevice(device) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    const int rc = zk_ptau_key_apply(ptau, F, K, section7, out, [&](int group, const u8* in, u64 count, const u8* c, const u8* t, u8* o, int section) {
      if (section == 2) g_stats.seconds[16] = now() - t0;      // (the first call comes after the copies of sections 1 and 7)
      ZkKeyPowers T;
      zk_key_powers_table(c, t, T);                            // (neither is 0: zk_ptau_key_scalars)
      g_stats.ops[2 * (section - 2)] = count * ZK_KEY_ADDS_PER_POINT; g_stats.ops[2 * (section - 2) + 1] = count * ZK_KEY_DBLS_PER_POINT;
      return mul_points(group, in, count, nullptr, &T, 0, o, false, nullptr, g_stats.seconds + 4 * (section - 2));
    }, [&](const u8* in, const u8* k, u8* o) {
      const double t = now();
      int r;
      {
        DevBufs B;
        void* d = B.get(128);
        if (B.oom) return (int)ZKWG_RC_OOM;
        r = hipMemcpy(d, in, 128, hipMemcpyHostToDevice) == hipSuccess ? ZKWG_RC_OK : ZKWG_RC_HIP_ERROR;
        if (r == ZKWG_RC_OK) r = zkwg_point_scale_device(device, 2, d, 1, k, d, nullptr);
        if (r == ZKWG_RC_OK && hipMemcpy(o, d, 128, hipMemcpyDeviceToHost) != hipSuccess) r = ZKWG_RC_HIP_ERROR;
      }                                                          // (freed before the time is taken)
      g_stats.seconds[17] = now() - t;
      return r;
    });
    if (rc == ZKWG_RC_OK && out_len) *out_len = F.out_bytes;
    return rc;
  } catch (const std::bad_alloc&) {
    return ZKWG_RC_OOM;
  }
}

void zkwg_ptau_apply_key_stats(double seconds[18], uint64_t ops[8]) {
  g_stats.copy(seconds, ops);
}

}
