// The host scaffold of the one-shot device calls -- the key ceremony, proof checking and DKIM verification: what
// zkwg_{setup,phase2,ptau,ptau_key,verify,pair,fexp,dkim}_api.hip (and nothing else) are written with.  Every one of those calls allocates its
// device buffers, synchronises and frees everything before it returns (zkwg_dkim_verify_batch may hand the batch's buffers to its caller) --
// so they share: the declarations of the launch wrappers, the sizes of a point, the refusal (fail), one owner of device
// buffers (DevBufs), the read of the fault flags (zk_read_flags), a stage clock, the per-thread statistics (ZkStats) and the check of
// the point arguments.  The piece loops themselves stay in their files.  Host only: no kernel includes this.
#pragma once
#include <hip/hip_runtime.h>
#include <chrono>
#include <string>
#include <vector>
#include "../../include/zkwg.h"
#include "zkwg_setup_core.h"

struct ZkPhase2Digits;      // zkwg_phase2_core.h
struct ZkPtauTw;            // zkwg_ptau_core.h
struct ZkKeyPowers;         // zkwg_ptau_key_core.h

// ---- the launch wrappers, each declared here once
// zkwg_kernels_setup.hip
void zk_setup_run_launch(int group, const ZkSetupRun& r, hipStream_t st);
void zk_setup_prepare_launch(int group, const void* in, void* out, u64 n, u32* bad, hipStream_t st);
void zk_setup_to_affine_launch(int group, const void* acc, Fq29* den, Fq29* pref, const u32* seg_wire, void* out, u32 n, hipStream_t st);
void zk_setup_odd_copy_launch(const void* in, void* out, u64 n, hipStream_t st);
// zkwg_kernels_phase2.hip
void zk_phase2_scale_launch(int group, const void* pts, void* acc, u32 n, const ZkPhase2Digits& D, hipStream_t st);
// zkwg_kernels_ptau.hip
void zk_ptau_stage_launch(int group, const void* pts, void* acc, const ZkPtauTw* tw, u32 L, u32 s, u32 table_L, hipStream_t st);
void zk_ptau_permute_launch(int group, void* pts, u32 L, hipStream_t st);
// zkwg_kernels_ptau_key.hip
void zk_ptau_key_table_launch(int group, const void* tab, void* acc, u32 n, hipStream_t st);
void zk_ptau_key_walk_launch(int group, const void* tab, void* acc, u32 n, const void* scalars, const ZkKeyPowers* powers, u64 first, hipStream_t st);
// zkwg_kernels_verify.hip
void zk_verify_g2_subgroup_launch(const void* pts, u32 n, const ZkPhase2Digits& Du, u32* res, hipStream_t st);
void zk_verify_widen_launch(const void* in, void* out, u64 n, hipStream_t st);
// zkwg_kernels_pair.hip
void zk_pair_miller_launch(const void* g1, const void* g2, u32 n, const ZkPhase2Digits& Du, void* f, u8* inside, hipStream_t st);
void zk_pair_product_launch(const void* f, const u8* use, u32 n, void* out, hipStream_t st);
// zkwg_kernels_fexp.hip
void zk_fexp_fold_launch(const void* f, u32 n, u32 k, void* out, hipStream_t st);
void zk_fexp_ninv_launch(const void* x, const void* y, u32 n, void* out, hipStream_t st);
void zk_fexp_pow_u_launch(const void* g, u32 n, void* out, hipStream_t st);
void zk_fexp_step_launch(const void* x, const void* y, u32 n, u32 pre_a, u32 pre_b, u32 post, void* out, hipStream_t st);
void zk_g16_vkx_launch(const void* ic0, const void* terms, u32 n_terms, u32 n, void* g1, hipStream_t st);
// zkwg_kernels_dkim.hip
void zk_dkim_body_launch(const void* recs, const void* raw, void* bodies, void* body_len, void* fits, u32 stride, u32 n, hipStream_t st);
void zk_dkim_hash_launch(const void* recs, const void* bodies, const void* body_len, const void* fits, u32 body_stride, const void* headers,
                         const void* header_len, u32 header_stride, void* body_digest, void* header_digest, u32 n, hipStream_t st);
void zk_dkim_verify_launch(const void* recs, const void* keys, const void* fits, const void* body_digest, const void* header_digest, const void* signature_be,
                           u32 flags, void* status, void* key_index, void* pubkey_be, u32 n, hipStream_t st);
// zkwg_api.hip
extern "C" void zk_set_last_error(const char* m);

namespace {
inline u64 zk_pt_bytes(int group) { return group == 2 ? 128 : 64; }       // an affine point in the zkey's form
inline u64 zk_acc_bytes(int group) { return group == 2 ? 288 : 144; }     // an accumulator of the point kernels

inline int fail(const std::string& m) { zk_set_last_error(m.c_str()); return ZKWG_RC_BAD_CONFIG; }
inline double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
const char* const NOT_ON_CURVE = "a point is not on its curve (or not reduced)";

// group 1 / 2, neither array null when there are points, both 16-byte aligned (a call with one array passes it twice)
inline bool zk_bad_point_args(int group, const void* a, u64 n, const void* b) {
  return (group != 1 && group != 2) || (n && (!a || !b)) || ((uintptr_t)a & 15) || ((uintptr_t)b & 15);
}

// the device buffers of a call: freed when it returns (a request of 0 bytes gets 16: every buffer has an address).  After a failed
// allocation (oom; the sticky HIP error is cleared) nothing more is allocated and every later get returns null: the caller asks for
// all its buffers, then checks oom once -> ZKWG_RC_OOM
struct DevBufs {
  std::vector<void*> p;
  bool oom = false;
  void* get(u64 bytes) {
    void* d = nullptr;
    if (oom) return nullptr;
    if (hipMalloc(&d, bytes ? bytes : 16) != hipSuccess) { (void)hipGetLastError(); oom = true; return nullptr; }
    p.push_back(d);
    return d;
  }
  template <class T> T* up(const std::vector<T>& v) {
    T* d = (T*)get(v.size() * sizeof(T));
    if (d && !v.empty() && hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) oom = true;
    return d;
  }
  void drop(void* d) { for (void*& q : p) if (q == d) { hipFree(d); q = nullptr; } }      // one buffer, before the others
  ~DevBufs() { for (void* d : p) hipFree(d); }
};

// what the kernels have flagged so far: pending launch errors, the copy of n_words flag words, the stream's synchronisation
inline int zk_read_flags(hipStream_t st, const u32* d_flags, u32* host, int n_words) {
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(host, d_flags, 4 * n_words, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return ZKWG_RC_HIP_ERROR;
  return ZKWG_RC_OK;
}

// the seconds of a call's stages.  Without `seconds` a lap does nothing -- no synchronisation: a call nobody times stays asynchronous
// up to its last read of the flags; with it, lap(k) synchronises the stream and adds the time since the last lap (or start) to seconds[k]
struct ZkStageClock {
  hipStream_t st;
  double* seconds;
  double t;
  ZkStageClock(hipStream_t st, double* seconds) : st(st), seconds(seconds), t(now()) {}
  void start() { t = now(); }
  bool lap(int k) {
    if (!seconds) return true;
    if (hipStreamSynchronize(st) != hipSuccess) return false;
    seconds[k] += now() - t; t = now();
    return true;
  }
};

// the statistics of a thread's last call (one thread_local instance per file): NS seconds, NO operation counts
template <int NS, int NO> struct ZkStats {
  double seconds[NS];
  u64 ops[NO];
  void reset() { for (double& s : seconds) s = 0; for (u64& o : ops) o = 0; }
  void copy(double* s, uint64_t* o) const {
    if (s) for (int i = 0; i < NS; ++i) s[i] = seconds[i];
    if (o) for (int i = 0; i < NO; ++i) o[i] = ops[i];
  }
};
}  // namespace
