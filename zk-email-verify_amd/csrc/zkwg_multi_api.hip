// C-ABI of libzkwg.so (see include/zkwg.h), the multi-device calls: one handle and one host thread per GPU, the result table
// gathered over RCCL (opened with dlopen).  Written against the public ABI and the three internal calls of zkwg_rows_calls.h; the handle's type stays opaque here.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <dlfcn.h>
#include <algorithm>
#include <string>
#include <thread>
#include <vector>
#include "../../include/zkwg.h"

#include "zkwg_rows_calls.h"
extern "C" void zk_set_last_error(const char* m);      // zkwg_api.hip

extern "C" {

// ------------------------------------------------------------------ multi-device
// One handle + one host thread per GPU, contiguous shards, no data-path collective.  The only exchange is
// the gather of the 100-byte/email result table {status, pubkeyHash, shaHi, shaLo} on devices[0] over
// RCCL (ncclGroupStart + ncclSend / ncclRecv over xGMI).  RCCL is opened with dlopen when n_dev > 1 (and its header
// is not included), so a single-GPU deployment carries no dependency on it.
// The few RCCL declarations the gather needs (the library is opened with dlopen, so a single-GPU deployment
// neither links nor includes RCCL): nccl.h's ncclComm_t, ncclResult_t (0 = ncclSuccess), ncclDataType_t (1 = ncclUint8).
typedef struct ncclComm* zk_nccl_comm_t;
enum { ZK_NCCL_SUCCESS = 0, ZK_NCCL_UINT8 = 1 };
struct zkwg_multi {
  std::vector<zkwg_circuit_t*> h;
  std::vector<int> dev;
  std::vector<zk_nccl_comm_t> comm;
  void* rccl = nullptr;
  int (*CommInitAll)(zk_nccl_comm_t*, int, const int*) = nullptr;
  int (*CommDestroy)(zk_nccl_comm_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*Send)(const void*, size_t, int, int, zk_nccl_comm_t, hipStream_t) = nullptr;
  int (*Recv)(void*, size_t, int, int, zk_nccl_comm_t, hipStream_t) = nullptr;
};

void zkwg_shard_range(uint64_t n, int n_shards, int i, uint64_t* first, uint64_t* count) {
  // contiguous ranges whose sizes differ by at most one (the first n % n_shards shards take the extra email)
  if (n_shards <= 0 || i < 0 || i >= n_shards) { if (first) *first = 0; if (count) *count = 0; return; }
  const uint64_t q = n / (uint64_t)n_shards, r = n % (uint64_t)n_shards;
  const uint64_t f = (uint64_t)i * q + std::min<uint64_t>((uint64_t)i, r);
  if (first) *first = f;
  if (count) *count = q + ((uint64_t)i < r ? 1 : 0);
}

void zkwg_multi_destroy(zkwg_multi_t* m) {
  if (!m) return;
  for (auto cm : m->comm) if (cm && m->CommDestroy) m->CommDestroy(cm);
  for (auto c : m->h) zkwg_circuit_destroy(c);
  if (m->rccl) dlclose(m->rccl);
  delete m;
}

int zkwg_multi_create(const zkwg_config* cfg, const int* devices, int n_dev, zkwg_multi_t** out) {
  if (!cfg || !devices || n_dev <= 0 || !out) return ZKWG_RC_BAD_ARG;
  zkwg_multi* m = new zkwg_multi();
  int rc = ZKWG_RC_OK;
  for (int i = 0; i < n_dev && rc == ZKWG_RC_OK; ++i) {
    zkwg_circuit_t* c = nullptr;
    rc = zkwg_circuit_create(cfg, devices[i], &c);
    if (rc == ZKWG_RC_OK) { m->h.push_back(c); m->dev.push_back(devices[i]); }
  }
  if (rc == ZKWG_RC_OK && n_dev > 1) {
    // ZKWG_RCCL_LIB names the library (a deployment's own build; the single-GPU test of this branch loads a
    // stand-in that implements the six calls with hipMemcpyAsync, tests/native/rccl_stub.cpp)
    const char* lib = getenv("ZKWG_RCCL_LIB");
    if (lib && *lib) m->rccl = dlopen(lib, RTLD_NOW | RTLD_LOCAL);
    else {
      m->rccl = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
      if (!m->rccl) m->rccl = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    }
    if (!m->rccl) { zk_set_last_error((std::string(lib && *lib ? lib : "librccl.so") + " could not be loaded (needed for the result-table gather with n_dev > 1)").c_str()); rc = ZKWG_RC_BAD_CONFIG; }
    else {
      m->CommInitAll = (decltype(m->CommInitAll))dlsym(m->rccl, "ncclCommInitAll");
      m->CommDestroy = (decltype(m->CommDestroy))dlsym(m->rccl, "ncclCommDestroy");
      m->GroupStart = (decltype(m->GroupStart))dlsym(m->rccl, "ncclGroupStart");
      m->GroupEnd = (decltype(m->GroupEnd))dlsym(m->rccl, "ncclGroupEnd");
      m->Send = (decltype(m->Send))dlsym(m->rccl, "ncclSend");
      m->Recv = (decltype(m->Recv))dlsym(m->rccl, "ncclRecv");
      if (!m->CommInitAll || !m->CommDestroy || !m->GroupStart || !m->GroupEnd || !m->Send || !m->Recv) {
        zk_set_last_error("librccl.so lacks a required symbol"); rc = ZKWG_RC_BAD_CONFIG;
      } else {
        m->comm.assign(n_dev, nullptr);
        if (m->CommInitAll(m->comm.data(), n_dev, devices) != ZK_NCCL_SUCCESS) { m->comm.clear(); zk_set_last_error("ncclCommInitAll failed"); rc = ZKWG_RC_HIP_ERROR; }
      }
    }
  }
  if (rc != ZKWG_RC_OK) { zkwg_multi_destroy(m); return rc; }
  *out = m;
  return ZKWG_RC_OK;
}
int zkwg_multi_devices(const zkwg_multi_t* m) { return m ? (int)m->h.size() : 0; }
zkwg_circuit_t* zkwg_multi_circuit(zkwg_multi_t* m, int i) { return (m && i >= 0 && i < (int)m->h.size()) ? m->h[i] : nullptr; }

int zkwg_calculate_batch_multi(zkwg_multi_t* m, const uint8_t* packed, uint64_t n, uint8_t* out_wtns,
                               uint64_t out_stride, int32_t* status, uint8_t* table, uint64_t max_tile) {
  if (!m || !packed || !status || m->h.empty()) return ZKWG_RC_BAD_ARG;
  if (n == 0) return ZKWG_RC_OK;
  const int nd = (int)m->h.size();
  const uint64_t in_stride = zkwg_input_stride(m->h[0]);
  std::vector<uint8_t*> d_rows(nd, nullptr), d_tab(nd, nullptr);
  std::vector<int32_t*> d_st(nd, nullptr);
  std::vector<int> rcs(nd, ZKWG_RC_OK);
  std::vector<uint64_t> first(nd), cnt(nd);
  for (int i = 0; i < nd; ++i) zkwg_shard_range(n, nd, i, &first[i], &cnt[i]);
  auto worker = [&](int i) {
    if (cnt[i] == 0) return;
    if (hipSetDevice(m->dev[i]) != hipSuccess) { rcs[i] = ZKWG_RC_HIP_ERROR; return; }
    if (table && hipMalloc((void**)&d_rows[i], cnt[i] * 96) != hipSuccess) { rcs[i] = ZKWG_RC_OOM; return; }
    // out_wtns = NULL: nothing but the result table leaves the GPUs -- the device-resident two-stream pipeline (witnesses into
    // each GPU's own placed ring); otherwise each shard's witnesses leave through that GPU's PCIe link
    if (!out_wtns) rcs[i] = zk_calculate_batch_resident_rows(m->h[i], packed + first[i] * in_stride, cnt[i], status + first[i], max_tile, 0, d_rows[i], nullptr, nullptr);
    else rcs[i] = zk_calculate_batch_rows(m->h[i], packed + first[i] * in_stride, cnt[i], out_wtns + first[i] * out_stride, out_stride, status + first[i],
                                       max_tile, d_rows[i]);
    if (rcs[i] != ZKWG_RC_OK || !table) return;
    // device-side table rows of this shard: {status i32, 96 bytes}
    if (hipMalloc((void**)&d_tab[i], cnt[i] * 100) != hipSuccess || hipMalloc((void**)&d_st[i], cnt[i] * 4) != hipSuccess) { rcs[i] = ZKWG_RC_OOM; return; }
    hipStream_t st = (hipStream_t)zk_circuit_stream(m->h[i]);
    bool ok = hipMemcpyAsync(d_st[i], status + first[i], cnt[i] * 4, hipMemcpyHostToDevice, st) == hipSuccess &&
              hipMemcpy2DAsync(d_tab[i], 100, d_st[i], 4, 4, cnt[i], hipMemcpyDeviceToDevice, st) == hipSuccess &&
              hipMemcpy2DAsync(d_tab[i] + 4, 100, d_rows[i], 96, 96, cnt[i], hipMemcpyDeviceToDevice, st) == hipSuccess &&
              hipStreamSynchronize(st) == hipSuccess;
    if (!ok) rcs[i] = ZKWG_RC_HIP_ERROR;
  };
  int caller_dev = -1;
  if (hipGetDevice(&caller_dev) != hipSuccess) caller_dev = -1;   // worker(0) and the gather change the calling thread's device
  {
    std::vector<std::thread> th;
    for (int i = 1; i < nd; ++i) th.emplace_back(worker, i);
    worker(0);
    for (auto& t : th) t.join();
  }
  int rc = ZKWG_RC_OK;
  for (int i = 0; i < nd; ++i) if (rcs[i] != ZKWG_RC_OK) rc = rcs[i];
  if (rc == ZKWG_RC_OK && table) {
    // gather on devices[0]: rank i sends its rows, rank 0 receives them at the shard's offset
    uint8_t* d_all = nullptr;
    if (hipSetDevice(m->dev[0]) != hipSuccess || hipMalloc((void**)&d_all, n * 100) != hipSuccess) rc = ZKWG_RC_OOM;
    if (rc == ZKWG_RC_OK) {
      hipStream_t s0 = (hipStream_t)zk_circuit_stream(m->h[0]);
      bool ok = cnt[0] == 0 || hipMemcpyAsync(d_all, d_tab[0], cnt[0] * 100, hipMemcpyDeviceToDevice, s0) == hipSuccess;
      if (nd > 1 && ok) {
        ok = m->GroupStart() == ZK_NCCL_SUCCESS;
        if (ok) {
          // once a group is open it is always closed, whatever the calls inside returned
          for (int i = 1; i < nd && ok; ++i) {
            if (cnt[i] == 0) continue;
            ok = m->Recv(d_all + first[i] * 100, cnt[i] * 100, ZK_NCCL_UINT8, i, m->comm[0], s0) == ZK_NCCL_SUCCESS &&
                 m->Send(d_tab[i], cnt[i] * 100, ZK_NCCL_UINT8, 0, m->comm[i], (hipStream_t)zk_circuit_stream(m->h[i])) == ZK_NCCL_SUCCESS;
          }
          ok = (m->GroupEnd() == ZK_NCCL_SUCCESS) && ok;
        }
        for (int i = 1; i < nd; ++i) { if (hipSetDevice(m->dev[i]) != hipSuccess || hipStreamSynchronize((hipStream_t)zk_circuit_stream(m->h[i])) != hipSuccess) ok = false; }
        if (hipSetDevice(m->dev[0]) != hipSuccess) ok = false;
      }
      ok = ok && hipMemcpyAsync(table, d_all, n * 100, hipMemcpyDeviceToHost, s0) == hipSuccess;
      if (hipStreamSynchronize(s0) != hipSuccess) ok = false;
      if (!ok) rc = ZKWG_RC_HIP_ERROR;
    }
    if (d_all) hipFree(d_all);
  }
  for (int i = 0; i < nd; ++i) {
    if (d_rows[i] || d_tab[i] || d_st[i]) { hipSetDevice(m->dev[i]); hipFree(d_rows[i]); hipFree(d_tab[i]); hipFree(d_st[i]); }
  }
  if (caller_dev >= 0) (void)hipSetDevice(caller_dev);
  return rc;
}

}  // extern "C"
