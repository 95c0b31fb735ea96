// The witness handle (struct zkwg_circuit) behind include/zkwg.h, shared by zkwg_api.hip (construction, queries, writers),
// zkwg_launch_api.hip (the launch sequence) and zkwg_hostpath_api.hip (host-buffer path, host expansion, resident pipeline).
// Every device allocation, pinned buffer, stream and event of a handle belongs to one of the small owners below and is released by
// that owner's destructor: `delete c` is the whole free list, on the failing exits of zkwg_circuit_create* as on zkwg_circuit_destroy.
// Host only: no kernel includes this, and it pulls in neither the circom front end nor the layout walkers.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/zkwg.h"
#include "zkwg_sched.h"
#include "zkwg_net_core.h"
#include "zkwg_o0.h"

#define ZK_MAX_KERNELS 9   // (EmailReveal: the five EmailVerifier roles + zk_substr + zk_app_tail + zk_expand = 8; CleanEmailAddress: 5 + 2 + 1)
#define ZK_RS_SLOTS 16
#define ZK_EV_RING 512     // launches whose HIP events are kept for zkwg_timing_summary

namespace zkc { struct Net; }   // zkwg_circom.h

// ---- owners: each destroys exactly what it created
// device buffers that live and die together (the shape of DevBufs in zkwg_points_host.h, plus clear() for a group that is rebuilt).
// A request of 0 bytes gets 16: every buffer has an address.  After a failure every later get returns null: ask for all, check `failed` once
// (copy_failed: it was an upload, not an allocation).
struct ZkDevMem {
  std::vector<void*> p;
  bool failed = false, copy_failed = false;
  ZkDevMem() = default;
  ZkDevMem(const ZkDevMem&) = delete;
  ZkDevMem& operator=(const ZkDevMem&) = delete;
  void* get(u64 bytes) {
    void* d = nullptr;
    if (failed) return nullptr;
    if (hipMalloc(&d, bytes < 16 ? 16 : bytes) != hipSuccess) { (void)hipGetLastError(); failed = true; return nullptr; }
    p.push_back(d);
    return d;
  }
  void* up(const void* src, u64 bytes, u64 slack = 0) {      // `slack` bytes behind the copy, for kernels that read past the end
    void* d = get(bytes + slack);
    if (d && bytes && hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) != hipSuccess) failed = copy_failed = true;
    return d;
  }
  template <class T> T* up(const std::vector<T>& v, u64 slack = 0) { return (T*)up(v.data(), v.size() * sizeof(T), slack); }
  void drop(void* d) { for (size_t i = 0; i < p.size(); ++i) if (p[i] == d) { hipFree(d); p.erase(p.begin() + i); return; } }      // one buffer, before the others
  void clear() { for (void* d : p) hipFree(d); p.clear(); failed = copy_failed = false; }
  ~ZkDevMem() { clear(); }
};
struct ZkPinned {
  u8* p = nullptr;
  ZkPinned() = default;
  ZkPinned(const ZkPinned&) = delete;
  ZkPinned& operator=(const ZkPinned&) = delete;
  bool alloc(u64 bytes) { reset(); return hipHostMalloc((void**)&p, bytes, hipHostMallocDefault) == hipSuccess; }
  void reset() { if (p) hipHostFree(p); p = nullptr; }
  ~ZkPinned() { reset(); }
};
struct ZkStream {
  hipStream_t s = nullptr;
  ZkStream() = default;
  ZkStream(const ZkStream&) = delete;
  ZkStream& operator=(const ZkStream&) = delete;
  bool create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess; }
  bool create(int priority) { return hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority) == hipSuccess; }
  operator hipStream_t() const { return s; }
  ~ZkStream() { if (s) hipStreamDestroy(s); }
};
struct ZkEvent {
  hipEvent_t e = nullptr;
  ZkEvent() = default;
  ZkEvent(const ZkEvent&) = delete;
  ZkEvent& operator=(const ZkEvent&) = delete;
  bool create(unsigned flags = hipEventDisableTiming) { return e || hipEventCreateWithFlags(&e, flags) == hipSuccess; }      // (once)
  operator hipEvent_t() const { return e; }
  ~ZkEvent() { if (e) hipEventDestroy(e); }
};
// the resident pipeline's two-tile output ring: chunk-mapped (zkwg_vmm.hip) or plain
struct ZkRing {
  u8* out[2] = {nullptr, nullptr};
  u64 tile_bytes = 0;
  bool chunked = false;      // the tiles come from zkwg_device_alloc_chunked
  ZkRing() = default;
  ZkRing(const ZkRing&) = delete;
  ZkRing& operator=(const ZkRing&) = delete;
  void clear() {
    for (u8*& o : out) { if (o) { if (chunked) zkwg_device_free_chunked(o); else hipFree(o); } o = nullptr; }
    tile_bytes = 0;
  }
  ~ZkRing() { clear(); }
};

// ---- the handle's parts
// circuit and layout: what the schedule builder and the `.sym` / `.r1cs` readers leave (host memory only)
struct ZkLayoutPart {
  zkwg_config cfg{};
  zkwg_app_config app{};           // ZKWG_MAIN_EMAIL_REVEAL (zkwg_circuit_create_app)
  ZkSched s{};
  std::vector<ZkSeg> segs;
  std::vector<std::string> sym_names;  // layout SYM: witness index -> name
  std::vector<u32> kept_dst;       // `.sym` layouts: kept-v1 slot -> witness index (0xffffffff = dropped by the file)
  // fully numbered circuits (`--O0` / `--O1`): zk_expand_o0 writes every wire of the file straight from the image (zkwg_o0.h)
  u64 full_W = 0;                  // wires of the `.sym` / `.r1cs` (0: not a fully numbered circuit)
  u64 lin_rows = 0;                // rows of its linear completion plan (zkwg_full.h)
  ZkLinPlan lin_host;              // the plan, kept for layout-only handles (tests evaluate it on the host)
  std::vector<u32> o0_short; u64 n_o0_short = 0;
  std::vector<u32> o0_desc, o0_src, o0_long;   // host evaluation (layout-only handles): wire -> kept-v1 slot | 0xfffffffe (row);  row terms as kept-v1 slots;  the rows
  std::vector<Fr> invtab_host;     // entry (d + half) holds d^{-1} mod r in standard form (zkwg_expand_host; uploaded as d_invtab)
};
// device tables built once per handle
struct ZkTablesPart {
  ZkDevMem mem;
  Fr* d_invtab = nullptr;
  ZkSeg* d_segs = nullptr;
  ZkPortionEntry* d_ent = nullptr;   // zk_expand: one entry per piece of 256 K slots (zkwg_build.h zk_build_entries)
  u32 n_ent = 0;
  Fr* d_pos = nullptr;      // Poseidon(9): sparse-round table (zk_build_poseidon_sparse(10, 60)), dense tables, Montgomery constants, Poseidon(1)
  u32 pos_dense_off = 0, pos1_off = 0;
  Fr* d_pos_rs = nullptr;   // removeSoftLineBreaks / CleanEmailAddress (PoseidonModular): Poseidon(16) then Poseidon(2) sparse-round tables
  u32 pos2_off = 0;
  u32* d_pos_l29 = nullptr; // the same two tables in 29-bit limb form (zkwg_poseidon29.h): zk_rslb_chunks / _merge1, zk_cea_chunks / _tail
  u32 pos2_l29_off = 0;
  Fr* d_rs_zero = nullptr;  // removeSoftLineBreaks: signals + digest of the all-zero chunk (constant chunks, zkwg_kernels_rslb.hip); null: off
  // fused Montgomery output, built on first use and published as a pair: v * R mod r for v < 65536 | the inverse table in Montgomery form
  ZkDevMem mont;
  Fr* d_rtab = nullptr;
  Fr* d_invtab_m = nullptr;
};
// BodyHashRegex loaded from a circom template (zkwg_circuit_create_regex): the net (owned; only zkwg_api.hip sees its type) and its device copies
struct ZkRegexPart {
  zkc::Net* net = nullptr;
  ZkNetDec h_netd{};             // how zk_expand decodes the region, with host pointers (host expansion); d_netd: the device copy
  ZkDevMem mem;
  u32 *d_net_records = nullptr, *d_net_counts = nullptr, *d_net_mask_tab = nullptr, *d_net_pd = nullptr, *d_net_tabs = nullptr;
  ZkNetDec* d_netd = nullptr;
  u8 *d_net_cclass = nullptr, *d_net_cdelta = nullptr, *d_net_bclass = nullptr, *d_net_bdelta = nullptr;
  u32 *d_net_cmask = nullptr, *d_net_bmask = nullptr;
  ZkRegexPart() = default;
  ZkRegexPart(const ZkRegexPart&) = delete;
  ZkRegexPart& operator=(const ZkRegexPart&) = delete;
  ~ZkRegexPart();                // zkwg_api.hip
};
// descriptor + row tables over the image (zkwg_o0.h): a numbered circuit's wires (o0), an attached system's A.w | B.w | C.w (abc)
struct ZkO0Part {
  ZkO0Tables t;                  // host copy (a device handle of a numbered circuit keeps its counters only)
  ZkO0Dev d{};                   // device pointers of the same, into mem
  ZkDevMem mem;
  u64 m = 0;                     // abc: constraints of the attached system (0: none)
  void clear() { mem.clear(); memset(&d, 0, sizeof(d)); }
};
// removeSoftLineBreaks: the serial merge chain (zk_rslb_chain, ~16 waves per 1024 emails, latency-bound) runs on a side stream so that
// the caller's stream can go on with the next batch; the expansion waits for the chain of the scratch buffer it reads (zk_wait_chain)
struct ZkRslbPart {
  ZkStream side[ZK_RS_SLOTS];    // one per scratch buffer in flight: chains of different batches overlap
  ZkEvent dep[ZK_RS_SLOTS], done[ZK_RS_SLOTS];
  const void* scr[ZK_RS_SLOTS] = {};
  int next = 0, sync = 0, nside = 0;
};
// EmailReveal: zk_substr and zk_app_tail read the record only, so they run on two streams of their own beside EmailVerifier's
// roles; the caller's stream waits for both at the end of zkwg_prepare_device (a timed prepare runs them in line instead)
struct ZkRevealPart {
  ZkStream stream[2];
  ZkEvent dep, done[2];
};
// host-buffer path (under hb_mutex): the handle's own streams, cached device staging (double-buffered witnesses), pinned images of host expansion
struct ZkHostBufPart {
  ZkStream own_stream, copy_stream;
  ZkEvent done[2], copied[2];
  ZkDevMem mem;
  u8 *in = nullptr, *out[2] = {nullptr, nullptr}, *scr = nullptr;
  int* status[2] = {nullptr, nullptr};
  u64 tile = 0;
  int host_expand_threads = 0;   // > 0: zkwg_calculate_batch expands on the host (zkwg_set_host_expand)
  ZkPinned hx_img[2]; u64 hx_bytes = 0;   // pinned staging of downloaded images (host expansion)
  void clear() {
    mem.clear(); in = out[0] = out[1] = scr = nullptr; status[0] = status[1] = nullptr; tile = 0;
    hx_img[0].reset(); hx_img[1].reset(); hx_bytes = 0;
  }
};
// device-resident pipeline (zkwg_calculate_batch_resident): buffers cached in the handle, under hb_mutex
struct ZkResidentPart {
  ZkDevMem mem;
  u8* in = nullptr; u64 in_cap = 0;
  u8* scr[2] = {nullptr, nullptr}; u64 scr_bytes = 0;
  int* status = nullptr; u64 n_cap = 0;
  ZkRing ring;
  ZkStream exp;
  ZkEvent prep_done[2], exp_done[2];
  float place_ms[8] = {0}; int place_n = 0, place_kept[2] = {-1, -1};   // (zkwg_resident_placement: unused since the ring is chunked)
  void clear_scratch() { mem.drop(scr[0]); mem.drop(scr[1]); scr[0] = scr[1] = nullptr; scr_bytes = 0; }
  void clear() { mem.clear(); in = nullptr; in_cap = 0; scr[0] = scr[1] = nullptr; scr_bytes = 0; status = nullptr; n_cap = 0; ring.clear(); }
};
// launch bookkeeping of zkwg_set_timing (under dev_mutex)
struct ZkTimingPart {
  int timing = 0;
  int n_kernels = 0;
  const char* kname[ZK_MAX_KERNELS] = {};
  u64 kslots[ZK_MAX_KERNELS] = {};
  ZkEvent ev[ZK_EV_RING][2];                    // zk_expand launches: start, stop
  ZkEvent pev[ZK_EV_RING][ZK_MAX_KERNELS + 1];  // prepare launches: boundaries between kernels
  u64 launches = 0, prep_launches = 0;          // launches recorded since timing was enabled
  bool ev_valid = false, prep_valid = false;
};
// tuning knobs, read from the environment at creation or set through the ABI
struct ZkKnobs {
  int rs_merge_lanes = 1;        // zk_rslb_merge1 (one lane per email, limb form) | 4: zk_rslb_merge (ZKWG_RSLB_MERGE_LANES)
  int o0_emails_per_wg = 16;     // emails per workgroup of zk_expand3_o0 (ZKWG_O0_EMAILS_PER_WG)
  u32 xcd_remap = 1;             // zk_expand workgroup -> portion mapping (ZKWG_XCD_REMAP)
  int rsa_wgs_per_cu = 0;        // ZKWG_RSA_WGS_PER_CU, zkwg_set_prepare_throttle
  int pos_lane = 0;              // 1: the lane-per-email zk_poseidon9 instead of zk_poseidon9_g16 (ZKWG_POS_LANE=1)
  int pos_wave_below = 1024;     // batches below this many emails use the wavefront-per-email kernel (ZKWG_POS_WAVE_BELOW)
  u32 prep_mask = 0xffffffffu;   // zkwg_set_prepare_mask (measurement aid)
};

struct zkwg_circuit {
  int device = -1;               // < 0: layout-only handle
  ZkLayoutPart lay;
  ZkKnobs knob;
  std::mutex hb_mutex;           // one host-path call at a time; lock order: hb_mutex, then dev_mutex
  std::mutex dev_mutex;          // launch bookkeeping (event rings, merge-chain slots, counters) of the device entry points
  ZkTablesPart tab;
  ZkRegexPart rx;
  ZkO0Part o0, abc;
  ZkRslbPart rs;
  ZkRevealPart rv;
  ZkHostBufPart hb;
  ZkResidentPart rp;
  ZkTimingPart tm;
};

// Device entry points may be called from a thread whose current HIP device is not the handle's.
struct ZkDeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit ZkDeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = hipSetDevice(dev) == hipSuccess; else prev = -1;
  }
  ~ZkDeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

extern "C" void zk_set_last_error(const char* m);      // zkwg_api.hip: the thread's last-error string

static inline u64 out_W(const zkwg_circuit* c) { return c->lay.full_W ? c->lay.full_W : c->lay.s.W; }   // witness length the caller sees
static inline u64 align256(u64 x) { return (x + 255) & ~255ull; }

// scratch buffer of an n-email batch: [SHA chaining states | bits | small | fr (+256) | removeSoftLineBreaks / CleanEmailAddress: the chunk
// kernel's dense-mix staging, 153 words per 16-element chunk, word-major (zkwg_poseidon29.h) | removeSoftLineBreaks: its two unit lists +
// counters | Montgomery copies (fr + limbs)].
// The Montgomery copies come LAST (round 6): a caller that never asks this buffer for a Montgomery-form output allocates
// zkwg_scratch_bytes_standard -- half the bytes where the image is mostly field elements (removeSoftLineBreaks: 22 instead of 45 GB per
// 4,096 emails, i.e. twice as many prepared batches in flight in the same HBM).
struct ZkScratchLayout { u64 off_hst, off_bits, off_small, off_fr, off_img_end, off_frm, off_rs_stage, off_rs_list, rs_units, total_std, total; };
static inline ZkScratchLayout scratch_layout(const ZkSched& s, u64 n) {
  ZkScratchLayout L;
  u64 off = 0;
  L.off_hst = off; off += align256(n * (u64)s.hstates_per_email * 32);
  L.off_bits = off; off += align256(n * (u64)s.img_bits * 8);
  L.off_small = off; off += align256(n * (u64)s.img_small * 4);
  L.off_fr = off; off += align256(n * (u64)s.img_fr * 32) + 256;
  L.off_img_end = off;
  // (sized by the larger PoseidonModular of the circuit: chunk kernels follow each other on the caller's stream and may share the words)
  const u64 nch = std::max(s.rslb ? s.rs_nch : 0u, s.cea.present ? s.cea.nch : 0u);
  L.rs_units = (n * nch + 63) / 64 * 64;
  L.off_rs_stage = off; off += align256(L.rs_units * 153 * 4);
  L.off_rs_list = off; off += s.rslb ? align256(L.rs_units * 2 * 4) + 256 : 0;      // constant chunks: two unit lists | their two counters
  L.total_std = off;
  L.off_frm = off; off += align256(n * (u64)(s.img_fr + ZK_MONT_LIMBS) * 32);
  L.total = off;
  return L;
}

// removeSoftLineBreaks: a merge chain may still be running on a side stream over this scratch buffer; `st` waits for it
static inline void zk_wait_chain(const zkwg_circuit* c, const void* d_scratch, hipStream_t st) {
  if (!c->lay.s.rslb || c->rs.sync) return;
  for (int i = 0; i < ZK_RS_SLOTS; ++i)
    if (c->rs.scr[i] == d_scratch) hipStreamWaitEvent(st, c->rs.done[i], 0);
}
