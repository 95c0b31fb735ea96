// C-ABI of the groth16 set-up (include/zkwg.h "the groth16 set-up"): zkwg_ptau_parse, zkwg_zkey_new_size, zkwg_zkey_new.
// zkwg_zkey_new is a one-shot call: it allocates its device buffers, synchronises after every stage (that is where its times come from)
// and frees everything before it returns -- a key is made once per circuit.
#include <string.h>
#include "zkwg_points_host.h"

namespace {
thread_local ZkStats<7, 8> g_stats;

// one sum: plan -> the n_vars points of a section, downloaded to `host_out` (point bytes: 64 / 128)
int run_plan(int group, const ZkSetupPlan& P, const ZkSetupMag* d_mag, const void* t0, const void* t1, const void* t2, u32 n_vars, u8* host_out) {
  DevBufs B;
  const u64 pt = zk_pt_bytes(group), xs = zk_acc_bytes(group), n_seg = P.seg_wire.size();
  ZkSetupRun r;
  r.T = ZkSetupDev{B.up(P.terms), d_mag};
  r.t0 = t0; r.t1 = t1; r.t2 = t2;
  r.shorts = B.up(P.shorts); r.chunks = B.up(P.chunks); r.joins = B.up(P.joins);
  r.n_short = (u32)P.shorts.size(); r.n_chunk = (u32)P.chunks.size(); r.n_join = (u32)P.joins.size(); r.n_seg = (u32)n_seg;
  r.seg_wire = B.up(P.seg_wire);
  r.acc = B.get(n_seg * xs); r.part = B.get((u64)P.n_part * xs);
  r.den = (Fq29*)B.get(n_seg * sizeof(Fq29)); r.pref = (Fq29*)B.get(n_seg * sizeof(Fq29));
  r.out = B.get((u64)n_vars * pt);
  if (B.oom) return ZKWG_RC_OOM;
  if (hipMemset(r.out, 0, (u64)n_vars * pt) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  zk_setup_run_launch(group, r, nullptr);
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return ZKWG_RC_HIP_ERROR;
  if (hipMemcpy(host_out, r.out, (u64)n_vars * pt, hipMemcpyDeviceToHost) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  return ZKWG_RC_OK;
}
}  // namespace

extern "C" {

int zkwg_ptau_parse(const uint8_t* ptau, uint64_t len, uint32_t power, zkwg_setup_slices* out) {
  if (!ptau || !out) return ZKWG_RC_BAD_ARG;
  std::string err;
  const int rc = zk_ptau_parse(ptau, len, power, *out, err);
  if (rc != ZKWG_RC_OK) zk_set_last_error(err.c_str());
  return rc;
}

int zkwg_zkey_new_size(const uint8_t* r1cs, uint64_t len, uint32_t* power, uint64_t* zkey_bytes) {
  if (!r1cs) return ZKWG_RC_BAD_ARG;
  try {
    ZkR1csHost R;
    if (!zk_r1cs_parse(r1cs, len, R)) return fail("the .r1cs file could not be parsed: " + R.err);
    ZkSetupShape S;
    std::string err;
    if (zk_setup_shape(R, S, err) != ZKWG_RC_OK) return fail(err);
    if (power) *power = S.power;
    if (zkey_bytes) *zkey_bytes = S.zkey_bytes;
    return ZKWG_RC_OK;
  } catch (const std::bad_alloc&) {
    return ZKWG_RC_OOM;
  }
}

int zkwg_zkey_new(int device, const uint8_t* r1cs, uint64_t len, const zkwg_setup_slices* sl, uint8_t* out_zkey, uint64_t cap, uint64_t* out_len) {
  if (!r1cs || !sl || !out_zkey || !sl->tau_g1 || !sl->tau_g2 || !sl->alpha_tau_g1 || !sl->beta_tau_g1 || !sl->tau_g1_next) return ZKWG_RC_BAD_ARG;
  if (device < 0) return ZKWG_RC_NO_DEVICE;
  try {
    g_stats.reset();
    double t = now();
    ZkR1csHost R;
    if (!zk_r1cs_parse(r1cs, len, R)) return fail("the .r1cs file could not be parsed: " + R.err);
    ZkSetupShape S;
    std::string err;
    if (zk_setup_shape(R, S, err) != ZKWG_RC_OK) return fail(err);
    if (sl->power < S.power) return fail("the powers of tau are too small for the circuit: power " + std::to_string(sl->power) + ", needed " + std::to_string(S.power));
    if (sl->power != S.power) return fail("the slices are of power " + std::to_string(sl->power) + ", the circuit's domain is 2^" + std::to_string(S.power));
    if (cap < S.zkey_bytes) return ZKWG_RC_BAD_ARG;
    ZkSetupMags M;
    ZkSetupPlan pa, pb, pk;
    if (zk_setup_plan(R, S, ZK_SETUP_SRC_A, 1, M, pa, err) != ZKWG_RC_OK || zk_setup_plan(R, S, ZK_SETUP_SRC_B, 1, M, pb, err) != ZKWG_RC_OK ||
        zk_setup_plan(R, S, ZK_SETUP_SRC_K, 3, M, pk, err) != ZKWG_RC_OK)
      return fail(err);
    ZkSetupLayout L;
    zk_setup_write_frame(R, S, *sl, out_zkey, L);
    const ZkSetupPlan* plans[4] = {&pa, &pb, &pb, &pk};
    for (int i = 0; i < 4; ++i) { g_stats.ops[2 * i] = plans[i]->n_add; g_stats.ops[2 * i + 1] = plans[i]->n_dbl; }
    g_stats.seconds[0] = now() - t; t = now();

    if (hipSetDevice(device) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    DevBufs B;
    const u64 n = S.domain;
    void *d_t1 = B.get(64 * n), *d_ta = B.get(64 * n), *d_tb = B.get(64 * n), *d_t2 = B.get(128 * n);
    void* d_stage = sl->on_device ? nullptr : B.get(128 * n);
    u32* d_bad = (u32*)B.get(4);
    if (B.oom) return ZKWG_RC_OOM;
    if (hipMemset(d_bad, 0, 4) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    // every slice: uploaded as it is, checked and brought to the tables' form on the device; level p + 1 last (it stays for section 9)
    struct Slice { const void* p; void* table; int group; u64 count; };
    const Slice slices[5] = {{sl->tau_g1, d_t1, 1, n}, {sl->alpha_tau_g1, d_ta, 1, n}, {sl->beta_tau_g1, d_tb, 1, n}, {sl->tau_g2, d_t2, 2, n}, {sl->tau_g1_next, nullptr, 1, 2 * n}};
    const void* d_next = sl->tau_g1_next;
    for (const Slice& s : slices) {
      const void* src = s.p;
      if (!sl->on_device) {
        if (hipMemcpy(d_stage, s.p, s.count * zk_pt_bytes(s.group), hipMemcpyHostToDevice) != hipSuccess) return ZKWG_RC_HIP_ERROR;
        src = d_stage;
        d_next = d_stage;
      }
      zk_setup_prepare_launch(s.group, src, s.table, s.count, d_bad, nullptr);
      if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return ZKWG_RC_HIP_ERROR;
    }
    u32 bad = 0;
    if (hipMemcpy(&bad, d_bad, 4, hipMemcpyDeviceToHost) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    if (bad) return fail("a point of the powers of tau is not on its curve (or not reduced)");
    const ZkSetupMag* d_mag = B.up(M.mag);
    if (B.oom) return ZKWG_RC_OOM;
    g_stats.seconds[1] = now() - t; t = now();

    std::vector<u8> sec((size_t)64 * S.n_vars);
    int rc = run_plan(1, pa, d_mag, d_t1, nullptr, nullptr, S.n_vars, out_zkey + L.off[5]);
    g_stats.seconds[2] = now() - t; t = now();
    if (rc == ZKWG_RC_OK) rc = run_plan(1, pb, d_mag, d_t1, nullptr, nullptr, S.n_vars, out_zkey + L.off[6]);
    g_stats.seconds[3] = now() - t; t = now();
    if (rc == ZKWG_RC_OK) rc = run_plan(2, pb, d_mag, d_t2, nullptr, nullptr, S.n_vars, out_zkey + L.off[7]);
    g_stats.seconds[4] = now() - t; t = now();
    if (rc == ZKWG_RC_OK) rc = run_plan(1, pk, d_mag, d_t1, d_tb, d_ta, S.n_vars, sec.data());
    g_stats.seconds[5] = now() - t; t = now();
    if (rc != ZKWG_RC_OK) return rc;
    memcpy(out_zkey + L.off[3], sec.data(), 64ull * (S.n_public + 1));
    memcpy(out_zkey + L.off[8], sec.data() + 64ull * (S.n_public + 1), 64ull * (S.n_vars - S.n_public - 1));
    // section 9: the odd entries of level p + 1 (d_t1 is free now)
    zk_setup_odd_copy_launch(d_next, d_t1, n, nullptr);
    if (hipGetLastError() != hipSuccess || hipMemcpy(out_zkey + L.off[9], d_t1, 64 * n, hipMemcpyDeviceToHost) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    g_stats.seconds[6] = now() - t;
    if (out_len) *out_len = S.zkey_bytes;
    return ZKWG_RC_OK;
  } catch (const std::bad_alloc&) {
    return ZKWG_RC_OOM;
  }
}

void zkwg_zkey_new_stats(double seconds[7], uint64_t ops[8]) {
  g_stats.copy(seconds, ops);
}

}
