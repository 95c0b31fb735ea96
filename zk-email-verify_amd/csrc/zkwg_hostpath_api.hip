// C-ABI of libzkwg.so (see include/zkwg.h), the host paths of the witness handle: the host-buffer path (zkwg_calculate_batch), host
// expansion of a downloaded image, the device-resident pipeline, pinned memory and CU-masked streams.  The kernels are reached through
// zkwg_prepare_device / zkwg_expand_device (zkwg_launch_api.hip) only.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>
#include <emmintrin.h>
#include "zkwg_handle.h"
#include "zkwg_rows_calls.h"
#include "zkwg_o0_dec.h"
#include "zkwg_expand_dec.h"

extern "C" int zk_rows_copy_launch(const u8* src, u64 stride, u8* dst, u32 count, hipStream_t st);   // zkwg_kernels_handoff.hip
// host expansion helpers (zkwg_expand_host below)
static inline void zk_host_put(u8* dst, u32 code, const ZkRefSrc& R) {
  uint4 lo, hi;
  if (!(code >> 31)) { lo = make_uint4(code, 0, 0, 0); hi = make_uint4(0, 0, 0, 0); }
  else { lo = zk_ref_half(code, 0u, R); hi = zk_ref_half(code, 1u, R); }
  _mm_stream_si128((__m128i*)dst, _mm_set_epi32((int)lo.w, (int)lo.z, (int)lo.y, (int)lo.x));
  _mm_stream_si128((__m128i*)(dst + 16), _mm_set_epi32((int)hi.w, (int)hi.z, (int)hi.y, (int)hi.x));
}
template <class DEC>
static void zk_host_segment(const ZkSeg& sg, const ZkCtx& cx, const ZkRefSrc& R, u32 r0, u32 n, u8* dst) {
  const DEC dec(sg, cx);
  for (u32 i = 0; i < n; ++i) zk_host_put(dst + 32ull * i, dec(r0 + i), R);
}

extern "C" {

// The same values written by the host from a host copy of the scratch buffer (standard form): with `rows_on_host` = 0 the image
// comes from zkwg_prepare_device of a handle that already had the system attached (its row results are in the image; only
// the 4.4 MB image crosses PCIe instead of 72 MB of evaluations); with 1 the row tables are evaluated here as well -- the
// whole path of a layout-only handle, which is how the CPU tests check zk_o0_build's tables without a GPU.
static int tables_host(const zkwg_circuit* c, const ZkO0Tables& T, u64 W3, const uint8_t* records, uint64_t n, uint8_t* scratch_host,
                       uint64_t first, uint64_t count, int rows_on_host, uint8_t* out, uint64_t out_stride) {
  if (!c || !records || !scratch_host || !out) return ZKWG_RC_BAD_ARG;
  if (!W3 || T.desc.size() != 2 * W3) return ZKWG_RC_BAD_CONFIG;   // (a device handle of a numbered circuit keeps its tables on the device only)
  const ZkSched& s = c->lay.s;
  if (first + count > n || out_stride < W3 * 32 || (out_stride & 15) || ((uintptr_t)out & 15)) return ZKWG_RC_BAD_ARG;
  const ZkScratchLayout L = scratch_layout(s, n);
  for (u64 el = 0; el < count; ++el) {
    const u64 e = first + el;
    u32* small_w = (u32*)(scratch_host + L.off_small) + e * s.img_small;
    Fr* frv_w = (Fr*)(scratch_host + L.off_fr) + e * s.img_fr;
    ZkCtx cx;
    cx.rec = records + e * s.in_stride; cx.bits = (const u64*)(scratch_host + L.off_bits) + e * s.img_bits; cx.small = small_w;
    cx.half = (int)s.inv_half; cx.m_dfa_cm = s.m_dfa_cm; cx.m_dfa_pm = s.m_dfa_pm; cx.m_dfa_st = s.m_dfa_st;
    cx.nd = c->rx.net ? &c->rx.h_netd : nullptr;
    ZkRefSrc R;
    R.frv = (const uint4*)frv_w; R.invtab = (const uint4*)c->lay.invtab_host.data(); R.rec = cx.rec; R.small = cx.small;
    if (rows_on_host) {
      // zk_o0_generic, zk_o0_rows_small / _long / zk_o0_chains_small, zk_o0_rows_fr of zkwg_kernels_expand3.hip, one row at a time
      for (size_t g = 0; g < T.gen_seg.size(); ++g) small_w[T.gen_base + g] = zk_decode_any(c->lay.segs[T.gen_seg[g]], T.gen_r[g], cx);
      long long prev = 0;
      for (u64 j = 0; j < T.n_small(); ++j) {
        long long acc = T.s_chain[j] ? prev : 0;
        for (u64 t = T.s_ptr[j]; t < T.s_ptr[j + 1]; ++t)
          acc += (long long)T.s_coef[t] * zk_code_int(zk_desc_decode(T.s_term[2 * t], T.s_term[2 * t + 1], cx), cx);
        prev = acc;
        const u32 where = T.s_out[j];
        small_w[where & 0x7fffffffu] = (u32)(u64)acc;
        if (where >> 31) small_w[(where & 0x7fffffffu) + 1] = (u32)((u64)acc >> 32);
      }
      for (u64 j = 0; j < T.n_fr(); ++j) {
        Fr acc = fr_zero();
        for (u64 t = T.f_ptr[j]; t < T.f_ptr[j + 1]; ++t) {
          const Fr x = zk_code_value(zk_desc_decode(T.f_term[2 * t], T.f_term[2 * t + 1], cx), R);
          if (T.f_kind[t] == ZK_COEF_ONE) acc = fr_add(acc, x);
          else if (T.f_kind[t] == ZK_COEF_MINUS_ONE) acc = fr_sub(acc, x);
          else acc = fr_add(acc, fr_mont_mul(x, T.f_coefm[t]));
        }
        frv_w[T.fr_base + j] = acc;
      }
    }
    u8* w = out + el * out_stride;
    for (u64 i = 0; i < W3; ++i) zk_host_put(w + 32 * i, zk_wire_code(T.desc[2 * i], T.desc[2 * i + 1], T.aff.data(), cx), R);
  }
  _mm_sfence();
  return ZKWG_RC_OK;
}
int zkwg_expand_abc_host(const zkwg_circuit_t* c, const uint8_t* records, uint64_t n, uint8_t* scratch_host, uint64_t first,
                         uint64_t count, int rows_on_host, uint8_t* out, uint64_t out_stride) {
  if (!c) return ZKWG_RC_BAD_ARG;
  return tables_host(c, c->abc.t, 3 * c->abc.m, records, n, scratch_host, first, count, rows_on_host, out, out_stride);
}
// layout-only handles of a numbered circuit (zkwg_circuit_create_full): the complete witness from one image, through the very
// descriptor / row tables the device kernels read (tests)
int zkwg_expand_full_host(const zkwg_circuit_t* c, const uint8_t* records, uint64_t n, uint8_t* scratch_host, uint64_t first,
                          uint64_t count, uint8_t* out, uint64_t out_stride) {
  if (!c) return ZKWG_RC_BAD_ARG;
  return tables_host(c, c->o0.t, c->lay.full_W, records, n, scratch_host, first, count, 1, out, out_stride);
}

// Device staging buffers of the host-buffer path, cached in the handle (grow-only).
static int ensure_host_path_buffers(zkwg_circuit* c, u64 tile) {
  if (c->hb.tile >= tile) return ZKWG_RC_OK;
  ZkHostBufPart& H = c->hb;
  H.mem.clear(); H.tile = 0;      // (the pinned images of host expansion stay)
  const u64 wbytes = out_W(c) * 32;
  H.in = (u8*)H.mem.get(tile * c->lay.s.in_stride);
  for (int i = 0; i < 2; ++i) H.out[i] = (u8*)H.mem.get(tile * wbytes);
  H.scr = (u8*)H.mem.get(zkwg_scratch_bytes(c, tile));
  for (int i = 0; i < 2; ++i) H.status[i] = (int*)H.mem.get(tile * sizeof(int));
  if (H.mem.failed) { H.mem.clear(); return ZKWG_RC_OOM; }
  H.tile = tile;
  return ZKWG_RC_OK;
}

// d_rows (optional, device memory of the handle's GPU): n x 96 bytes, w[1..3] of every email
// (pubkeyHash, shaHi, shaLo for the EmailVerifier main) captured tile by tile for the result table.
int zk_calculate_batch_rows(zkwg_circuit_t* c, const uint8_t* packed, uint64_t n, uint8_t* out_wtns,
                            uint64_t out_stride, int32_t* status, uint64_t max_tile, uint8_t* d_rows) {
  if (!c || !packed || !status) return ZKWG_RC_BAD_ARG;
  if (c->device < 0) return ZKWG_RC_NO_DEVICE;
  if (n == 0) return ZKWG_RC_OK;
  const u64 wbytes = out_W(c) * 32;
  if (out_wtns && out_stride < wbytes) return ZKWG_RC_BAD_ARG;
  std::lock_guard<std::mutex> lock(c->hb_mutex);   // one host-path call at a time per handle
  if (hipSetDevice(c->device) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  // tile: two witness buffers must fit; default 256 emails (the D2H of one tile overlaps the kernels of the next)
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  const u64 have = (u64)free_b + c->hb.tile * (2 * wbytes);
  const u64 per_email = 2 * wbytes + c->lay.s.in_stride + zkwg_scratch_bytes(c, 64) / 64 + 64;
  u64 tile = max_tile ? max_tile : 256;
  tile = std::min<u64>(tile, std::max<u64>(1, (u64)(have * 0.8) / per_email));
  tile = std::min<u64>(tile, n);
  int rc = ensure_host_path_buffers(c, tile);
  if (rc != ZKWG_RC_OK) return rc;
  hipStream_t st = c->hb.own_stream, cs = c->hb.copy_stream;
  u64 t = 0;
  for (u64 base = 0; rc == ZKWG_RC_OK && base < n; base += tile, ++t) {
    const u64 cnt = std::min<u64>(tile, n - base);
    const int b = (int)(t & 1);
    if (t >= 2 && hipStreamWaitEvent(st, c->hb.copied[b], 0) != hipSuccess) { rc = ZKWG_RC_HIP_ERROR; break; }
    if (hipMemcpyAsync(c->hb.in, packed + base * c->lay.s.in_stride, cnt * c->lay.s.in_stride, hipMemcpyHostToDevice, st) != hipSuccess) { rc = ZKWG_RC_HIP_ERROR; break; }
    rc = zkwg_calculate_batch_device(c, c->hb.in, cnt, c->hb.out[b], wbytes, c->hb.status[b], c->hb.scr, st);
    if (rc != ZKWG_RC_OK) break;
    if (d_rows && hipMemcpy2DAsync(d_rows + base * 96, 96, c->hb.out[b] + 32, wbytes, 96, cnt, hipMemcpyDeviceToDevice, st) != hipSuccess) { rc = ZKWG_RC_HIP_ERROR; break; }
    if (hipEventRecord(c->hb.done[b], st) != hipSuccess || hipStreamWaitEvent(cs, c->hb.done[b], 0) != hipSuccess) { rc = ZKWG_RC_HIP_ERROR; break; }
    if (out_wtns) {
      hipError_t e = (out_stride == wbytes)
          ? hipMemcpyAsync(out_wtns + base * out_stride, c->hb.out[b], cnt * wbytes, hipMemcpyDeviceToHost, cs)
          : hipMemcpy2DAsync(out_wtns + base * out_stride, out_stride, c->hb.out[b], wbytes, wbytes, cnt, hipMemcpyDeviceToHost, cs);
      if (e != hipSuccess) { rc = ZKWG_RC_HIP_ERROR; break; }
    }
    if (hipMemcpyAsync(status + base, c->hb.status[b], cnt * sizeof(int), hipMemcpyDeviceToHost, cs) != hipSuccess) { rc = ZKWG_RC_HIP_ERROR; break; }
    if (hipEventRecord(c->hb.copied[b], cs) != hipSuccess) { rc = ZKWG_RC_HIP_ERROR; break; }
  }
  if (hipStreamSynchronize(st) != hipSuccess) rc = rc == ZKWG_RC_OK ? ZKWG_RC_HIP_ERROR : rc;
  if (hipStreamSynchronize(cs) != hipSuccess) rc = rc == ZKWG_RC_OK ? ZKWG_RC_HIP_ERROR : rc;
  return rc;
}


// ------------------------------------------------------------------ host expansion (the delivered rate)
// A witness delivered to HOST memory crosses PCIe at 32 bytes per signal (56.9 MB per email, ~55 GB/s: 963 witnesses/s).
// Its information is the 0.45 MB image.  zkwg_expand_host runs the same segment decoders (zkwg_expand_dec.h, compiled
// for the host) over a downloaded image and writes the witness straight into the caller's buffer with non-temporal
// stores, on `threads` host threads -- the expansion then costs host memory bandwidth instead of PCIe.  Bit-identical
// to zk_expand by construction (same decoders), checked in tests/test_host_expand.py.
int zkwg_expand_host(const zkwg_circuit_t* c, const uint8_t* records, uint64_t n, const uint8_t* scratch_host, uint64_t first,
                     uint64_t count, uint8_t* out, uint64_t out_stride, int threads) {
  if (!c || !records || !scratch_host || !out) return ZKWG_RC_BAD_ARG;
  if (c->lay.full_W) return ZKWG_RC_BAD_CONFIG;      // numbered circuits: their row results are computed on the device
  const ZkSched& s = c->lay.s;
  if (first + count > n || out_stride < s.W * 32 || (out_stride & 15) || ((uintptr_t)out & 15)) return ZKWG_RC_BAD_ARG;
  const ZkScratchLayout L = scratch_layout(s, n);
  const u64* bits = (const u64*)(scratch_host + L.off_bits);
  const u32* small = (const u32*)(scratch_host + L.off_small);
  const Fr* frv = (const Fr*)(scratch_host + L.off_fr);
  const u64 CH = 1u << 16;                                   // slots per work item
  const u64 per = (s.W + CH - 1) / CH, items = count * per;
  std::atomic<u64> next(0);
  auto work = [&]() {
    for (;;) {
      const u64 it = next.fetch_add(1);
      if (it >= items) break;
      const u64 el = it / per, slot0 = (it % per) * CH, slot1 = std::min<u64>(s.W, slot0 + CH), e = first + el;
      ZkCtx cx;
      cx.rec = records + e * s.in_stride; cx.bits = bits + e * s.img_bits; cx.small = small + e * s.img_small;
      cx.half = (int)s.inv_half; cx.m_dfa_cm = s.m_dfa_cm; cx.m_dfa_pm = s.m_dfa_pm; cx.m_dfa_st = s.m_dfa_st;
      cx.nd = c->rx.net ? &c->rx.h_netd : nullptr;
        ZkRefSrc R;
      R.frv = (const uint4*)(frv + e * s.img_fr); R.invtab = (const uint4*)c->lay.invtab_host.data(); R.rec = cx.rec; R.small = cx.small;
      u8* w = out + el * out_stride;
      size_t lo = 0, hi = c->lay.segs.size();
      while (hi - lo > 1) { const size_t mid = (lo + hi) / 2; if (c->lay.segs[mid].slot <= slot0) lo = mid; else hi = mid; }
      for (size_t si = lo; si < c->lay.segs.size() && c->lay.segs[si].slot < slot1; ++si) {
        const ZkSeg& sg = c->lay.segs[si];
        const u64 a = std::max<u64>(sg.slot, slot0), b = std::min<u64>(sg.slot + sg.nslots, slot1);
        const u32 r0 = (u32)(a - sg.slot) + sg.r0, cnt = (u32)(b - a);
        u8* dst = w + 32 * a;
        switch (sg.type) {
#define ZK_X(T, D) case T: zk_host_segment<D>(sg, cx, R, r0, cnt, dst); break;
          ZK_FOR_SEG_TYPES_ALL(ZK_X)
#undef ZK_X
          default: memset(dst, 0, 32ull * cnt); break;
        }
      }
    }
    _mm_sfence();
  };
  const int T = std::max(1, threads);
  std::vector<std::thread> th;
  for (int i = 1; i < T; ++i) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
  return ZKWG_RC_OK;
}
int zkwg_set_host_expand(zkwg_circuit_t* c, int threads) {
  if (!c || threads < 0) return ZKWG_RC_BAD_ARG;
  std::lock_guard<std::mutex> lock(c->hb_mutex);
  c->hb.host_expand_threads = threads;
  return ZKWG_RC_OK;
}

// zkwg_calculate_batch with the expansion on the host: per tile H2D records -> prepare kernels -> D2H of the image
// (0.45 MB per email instead of 56.9 MB of witness) into pinned staging; the host threads expand tile t into the
// caller's buffer while the device prepares tile t + 1.
static int calculate_batch_hostexpand(zkwg_circuit_t* c, const uint8_t* packed, uint64_t n, uint8_t* out_wtns,
                                      uint64_t out_stride, int32_t* status, uint64_t max_tile) {
  const ZkSched& s = c->lay.s;
  if (hipSetDevice(c->device) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  const u64 tile = std::min<u64>(max_tile ? max_tile : 256, n);
  const u64 scr_bytes = zkwg_scratch_bytes(c, tile);
  // device: records + scratch + status for two tiles in flight
  u8 *d_in[2], *d_scr[2];
  int* d_st[2];
  int rc = ZKWG_RC_OK;
  if (c->hb.hx_bytes < scr_bytes) {
    c->hb.hx_bytes = 0;
    for (int i = 0; i < 2; ++i) if (!c->hb.hx_img[i].alloc(scr_bytes)) rc = ZKWG_RC_OOM;
    if (rc == ZKWG_RC_OK) c->hb.hx_bytes = scr_bytes;
  }
  if (rc != ZKWG_RC_OK) return rc;
  ZkDevMem call;      // this call's buffers
  for (int i = 0; i < 2; ++i) { d_in[i] = (u8*)call.get(tile * s.in_stride); d_scr[i] = (u8*)call.get(scr_bytes); d_st[i] = (int*)call.get(tile * sizeof(int)); }
  if (call.failed) return ZKWG_RC_OOM;
  hipStream_t st = c->hb.own_stream;
  const ZkScratchLayout L = scratch_layout(s, tile);
  const u64 img_lo = L.off_bits, img_hi = L.off_img_end;      // the image arrays (not the SHA chaining states / staging / Montgomery copies)
  auto submit = [&](u64 t) -> int {
    const u64 base = t * tile, cnt = std::min<u64>(tile, n - base);
    const int b = (int)(t & 1);
    if (hipMemcpyAsync(d_in[b], packed + base * s.in_stride, cnt * s.in_stride, hipMemcpyHostToDevice, st) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    // NB the scratch layout depends on the batch size: every tile is prepared as a batch of `tile` emails; the records beyond
    // cnt of a partial last tile are zeroed (their images are never expanded, but the kernels must not chew on
    // uninitialised device memory: ADVICE r3)
    if (cnt < tile && hipMemsetAsync(d_in[b] + cnt * s.in_stride, 0, (tile - cnt) * s.in_stride, st) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    int r = zkwg_prepare_device(c, d_in[b], tile, d_st[b], d_scr[b], st);
    if (r != ZKWG_RC_OK) return r;
    zk_wait_chain(c, d_scr[b], st);
    if (hipMemcpyAsync(c->hb.hx_img[b].p + img_lo, d_scr[b] + img_lo, img_hi - img_lo, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(status + base, d_st[b], cnt * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipEventRecord(c->hb.done[b], st) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    return ZKWG_RC_OK;
  };
  const u64 ntiles = (n + tile - 1) / tile;
  if (rc == ZKWG_RC_OK) rc = submit(0);
  for (u64 t = 0; rc == ZKWG_RC_OK && t < ntiles; ++t) {
    if (t + 1 < ntiles) rc = submit(t + 1);                     // the device works on tile t + 1 ...
    if (rc != ZKWG_RC_OK) break;
    const int b = (int)(t & 1);
    if (hipEventSynchronize(c->hb.done[b]) != hipSuccess) { rc = ZKWG_RC_HIP_ERROR; break; }
    const u64 base = t * tile, cnt = std::min<u64>(tile, n - base);
    // ... while the host expands tile t (records: the caller's own buffer, indexed from the tile's first email)
    // (the image was laid out for a batch of `tile` emails: zkwg_expand_host derives the same layout from its n argument;
    //  only the records of the cnt emails it expands are read)
    rc = zkwg_expand_host(c, packed + base * s.in_stride, tile, c->hb.hx_img[b].p, 0, cnt, out_wtns + base * out_stride, out_stride,
                          c->hb.host_expand_threads);
  }
  if (hipStreamSynchronize(st) != hipSuccess && rc == ZKWG_RC_OK) rc = ZKWG_RC_HIP_ERROR;
  return rc;
}

int zkwg_calculate_batch(zkwg_circuit_t* c, const uint8_t* packed, uint64_t n, uint8_t* out_wtns,
                         uint64_t out_stride, int32_t* status, uint64_t max_tile) {
  if (c && c->device >= 0 && c->hb.host_expand_threads > 0 && out_wtns && packed && status && n && !c->lay.full_W && out_stride >= out_W(c) * 32 && !(out_stride & 15) && !((uintptr_t)out_wtns & 15)) {
    std::lock_guard<std::mutex> lock(c->hb_mutex);
    return calculate_batch_hostexpand(c, packed, n, out_wtns, out_stride, status, max_tile);
  }
  return zk_calculate_batch_rows(c, packed, n, out_wtns, out_stride, status, max_tile, nullptr);
}

// ------------------------------------------------------------------ device-resident pipeline below the boundary
// What bench.py's Pipeline does, for hosts without torch (the Node host of BASELINE.json's north_star): records go to the
// device once, the prepare kernels of sub-batch i + 1 run on one stream while sub-batch i is expanded tile by tile on another,
// witnesses are written into a two-tile ring in HBM -- placed where HBM takes the stores fastest (the
// real expansion is timed into spare candidate tiles once per handle) -- and handed to `consumer` (a device-side prover)
// stream-ordered; only the statuses and the three public outputs per email come back.  d_rows: optional device buffer,
// n x 96 bytes (the multi-device path gathers them over RCCL).
int zk_calculate_batch_resident_rows(zkwg_circuit_t* c, const uint8_t* packed, uint64_t n, int32_t* status, uint64_t tile_req,
                                     uint64_t prep_req, uint8_t* d_rows, zkwg_tile_fn consumer, void* user) {
  if (!c || !packed || !status) return ZKWG_RC_BAD_ARG;
  if (c->device < 0) return ZKWG_RC_NO_DEVICE;
  if (n == 0) return ZKWG_RC_OK;
  std::lock_guard<std::mutex> lock(c->hb_mutex);
  if (hipSetDevice(c->device) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  const u64 wbytes = out_W(c) * 32, in_stride = c->lay.s.in_stride;
  u64 tile = std::min<u64>(tile_req ? tile_req : 512, n);
  u64 prep = std::max<u64>(tile, std::min<u64>(prep_req ? prep_req : 1024, n));
  prep = prep / tile * tile;
  // fit: two output tiles, two scratch buffers, the records
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  const u64 held = 2 * c->rp.ring.tile_bytes + 2 * c->rp.scr_bytes + c->rp.in_cap * in_stride;
  while (tile > 1 && 2 * tile * wbytes + 2 * zkwg_scratch_bytes(c, prep) + n * in_stride > (u64)((free_b + held) * 0.9)) { tile = (tile + 1) / 2; prep = std::max(tile, prep / 2 / tile * tile); }
  ZkDevMem& RM = c->rp.mem;
  RM.failed = false;      // (a cache that outlives the call: an earlier call's failed allocation does not refuse this one)
  auto ensure = [&](void** p, u64& have, u64 want) -> bool {
    if (have >= want) return true;
    RM.drop(*p); have = 0;
    *p = RM.get(want);
    if (!*p) return false;
    have = want;
    return true;
  };
  if (!c->rp.exp) {
    int lo = 0, hi = 0;
    hipDeviceGetStreamPriorityRange(&lo, &hi);
    bool ok = true;      // (the stream last: it stands for the four events)
    for (int i = 0; i < 2; ++i) ok = ok && c->rp.prep_done[i].create() && c->rp.exp_done[i].create();
    if (!ok || !c->rp.exp.create(hi)) return ZKWG_RC_HIP_ERROR;
  }
  {
    // (the capacities are written back on failure too: a buffer that is gone has capacity 0)
    u64 cap = c->rp.in_cap * in_stride;
    const bool in_ok = ensure((void**)&c->rp.in, cap, n * in_stride);
    c->rp.in_cap = cap / in_stride;
    if (!in_ok) return ZKWG_RC_OOM;
    u64 sc = c->rp.n_cap * sizeof(int);
    const bool st_ok = ensure((void**)&c->rp.status, sc, n * sizeof(int));
    c->rp.n_cap = sc / sizeof(int);
    if (!st_ok) return ZKWG_RC_OOM;
    const u64 scr_b = zkwg_scratch_bytes(c, prep);
    if (c->rp.scr_bytes < scr_b) {
      c->rp.clear_scratch();
      for (int i = 0; i < 2; ++i) c->rp.scr[i] = (u8*)RM.get(scr_b);
      if (RM.failed) { c->rp.clear_scratch(); return ZKWG_RC_OOM; }
      c->rp.scr_bytes = scr_b;
    }
  }
  hipStream_t P = c->hb.own_stream, E = c->rp.exp;
  if (hipMemcpyAsync(c->rp.in, packed, n * in_stride, hipMemcpyHostToDevice, P) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  const u64 tile_bytes = tile * wbytes;
  bool place = c->rp.ring.tile_bytes < tile_bytes;      // (a larger tile: the ring is allocated again, and placed again)
  if (place) c->rp.ring.clear();
  int rc = ZKWG_RC_OK;
  u64 ring = 0;
  const u64 nsub = (n + prep - 1) / prep;
  for (u64 sb = 0; sb < nsub && rc == ZKWG_RC_OK; ++sb) {
    const u64 lo = sb * prep, cnt = std::min<u64>(prep, n - lo);
    const int b = (int)(sb & 1);
    if (sb >= 2) hipStreamWaitEvent(P, c->rp.exp_done[b], 0);      // scratch buffer b is free again
    rc = zkwg_prepare_device(c, c->rp.in + lo * in_stride, cnt, c->rp.status + lo, c->rp.scr[b], P);
    if (rc != ZKWG_RC_OK) break;
    hipEventRecord(c->rp.prep_done[b], P);
    hipStreamWaitEvent(E, c->rp.prep_done[b], 0);
    if (place) {
      // once per handle (and tile size): the two tiles of the output ring, mapped from 1 GiB physical chunks (zkwg_vmm.hip) -- every such
      // buffer takes zk_expand's stores at the rate only the best of round 4's hipMalloc candidates reached (profiles/r05/r05_f_*), with no
      // spare candidates and no transient memory.  ZKWG_PLACE_RING=0: two plain hipMalloc buffers.
      place = false;
      const bool chunked = !(getenv("ZKWG_PLACE_RING") && atoi(getenv("ZKWG_PLACE_RING")) == 0);
      c->rp.ring.chunked = chunked;
      for (int k = 0; k < 2 && rc == ZKWG_RC_OK; ++k) {
        void* p = nullptr;
        if (chunked) {
          // spare candidate chunks (half as many again, at most 16 GiB per tile): each takes a probe fill, the fastest are kept
          const u32 nch = (u32)((tile_bytes + (1ull << 30) - 1) >> 30);
          rc = zkwg_device_alloc_chunked_ex(c->device, tile_bytes, 0, std::min<u32>(nch / 2, 16u), &p, nullptr, 0, nullptr);
          if (rc != ZKWG_RC_OK) rc = zkwg_device_alloc_chunked(c->device, tile_bytes, 0, &p);
        }
        else if (hipMalloc(&p, tile_bytes) != hipSuccess) rc = ZKWG_RC_OOM;
        c->rp.ring.out[k] = (u8*)p;
      }
      c->rp.place_n = 0;
      if (rc != ZKWG_RC_OK) break;
      c->rp.ring.tile_bytes = tile_bytes;
    }
    for (u64 first = 0; first < cnt && rc == ZKWG_RC_OK; first += tile, ++ring) {
      const u64 count = std::min<u64>(tile, cnt - first);
      u8* o = c->rp.ring.out[ring & 1];
      rc = zkwg_expand_device(c, c->rp.in + lo * in_stride, cnt, c->rp.scr[b], first, count, o, wbytes, E);
      if (rc != ZKWG_RC_OK) break;
      if (d_rows && zk_rows_copy_launch(o, wbytes, d_rows + (lo + first) * 96, (u32)count, E) != 0) { rc = ZKWG_RC_HIP_ERROR; break; }
      if (consumer) consumer(user, c->device, o, wbytes, lo + first, count, (void*)E);
    }
    hipEventRecord(c->rp.exp_done[b], E);
  }
  if (rc == ZKWG_RC_OK && hipMemcpyAsync(status, c->rp.status, n * sizeof(int), hipMemcpyDeviceToHost, E) != hipSuccess) rc = ZKWG_RC_HIP_ERROR;
  if (hipStreamSynchronize(P) != hipSuccess && rc == ZKWG_RC_OK) rc = ZKWG_RC_HIP_ERROR;
  if (hipStreamSynchronize(E) != hipSuccess && rc == ZKWG_RC_OK) rc = ZKWG_RC_HIP_ERROR;
  return rc;
}

int zkwg_calculate_batch_resident(zkwg_circuit_t* c, const uint8_t* packed, uint64_t n, int32_t* status, uint8_t* table,
                                  uint64_t tile, uint64_t prep, zkwg_tile_fn consumer, void* user) {
  if (!c || !packed || !status) return ZKWG_RC_BAD_ARG;
  if (c->device < 0) return ZKWG_RC_NO_DEVICE;
  if (n == 0) return ZKWG_RC_OK;
  ZkDeviceGuard dg(c->device);
  if (!dg.ok) return ZKWG_RC_HIP_ERROR;
  ZkDevMem call;
  u8* d_rows = table ? (u8*)call.get(n * 96) : nullptr;
  if (call.failed) return ZKWG_RC_OOM;
  int rc = zk_calculate_batch_resident_rows(c, packed, n, status, tile, prep, d_rows, consumer, user);
  if (rc == ZKWG_RC_OK && table) {
    std::vector<u8> rows(n * 96);
    if (hipMemcpy(rows.data(), d_rows, n * 96, hipMemcpyDeviceToHost) != hipSuccess) rc = ZKWG_RC_HIP_ERROR;
    else for (u64 i = 0; i < n; ++i) { memcpy(table + 100 * i, status + i, 4); memcpy(table + 100 * i + 4, rows.data() + 96 * i, 96); }
  }
  return rc;
}
void* zk_circuit_stream(zkwg_circuit_t* c) { return (void*)(hipStream_t)c->hb.own_stream; }
// The buffers zkwg_calculate_batch_resident keeps in the handle between calls -- records, two scratch buffers, the two-tile witness ring
// (2 x 29 GB at the headline circuit's tile of 512), statuses -- go back to the device; the next call allocates and places them again.
int zkwg_resident_release(zkwg_circuit_t* c) {
  if (!c) return ZKWG_RC_BAD_ARG;
  if (c->device < 0) return ZKWG_RC_OK;
  std::lock_guard<std::mutex> lock(c->hb_mutex);
  if (hipSetDevice(c->device) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  if (c->rp.exp) hipStreamSynchronize(c->rp.exp);
  if (c->hb.own_stream) hipStreamSynchronize(c->hb.own_stream);
  c->rp.clear();
  return ZKWG_RC_OK;
}
// candidate tiles the ring was chosen from (average milliseconds of one tile's expansion into each; kept[2] = the chosen)
int zkwg_resident_placement(const zkwg_circuit_t* c, float* ms, int cap, int kept[2]) {
  if (!c) return 0;
  std::lock_guard<std::mutex> lock(const_cast<zkwg_circuit_t*>(c)->hb_mutex);   // (written by zkwg_calculate_batch_resident under the same lock)
  for (int i = 0; i < c->rp.place_n && i < cap; ++i) if (ms) ms[i] = c->rp.place_ms[i];
  if (kept) { kept[0] = c->rp.place_kept[0]; kept[1] = c->rp.place_kept[1]; }
  return c->rp.place_n;
}

// Page-locked host memory for witness output buffers: lets the D2H copy of one tile overlap the
// kernels of the next (pageable destinations work too, the copy is then staged by the runtime).
void* zkwg_alloc_pinned(uint64_t bytes) {
  void* p = nullptr;
  return hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess ? p : nullptr;
}
void zkwg_free_pinned(void* p) { if (p) hipHostFree(p); }


// A stream restricted to a subset of the compute units (hipExtStreamCreateWithCUMask): bit i of `mask` enables CU i.
// bench.py uses it to keep the latency-bound prepare kernels off the CUs zk_expand streams from.
void* zkwg_stream_create_masked(int device, const uint32_t* mask, int words) {
  if (!mask || words <= 0) return nullptr;
  ZkDeviceGuard dg(device);
  if (!dg.ok) return nullptr;
  hipStream_t st = nullptr;
  if (hipExtStreamCreateWithCUMask(&st, (uint32_t)words, mask) != hipSuccess) return nullptr;
  return (void*)st;
}
void zkwg_stream_destroy(void* stream) { if (stream) hipStreamDestroy((hipStream_t)stream); }

}  // extern "C"
