// C-ABI of libzkwg.so (see include/zkwg.h), the launch sequence of the witness path: zkwg_prepare_device, the three expansions,
// zkwg_calculate_batch_device, zkwg_generate_inputs_device, and the timing and knob setters.  The only API file that sees the witness kernels.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>
#include "zkwg_handle.h"
#include "zkwg_kernels.h"
#include "zkwg_bh_dfa.h"   // ZK_DFA_STATES

extern "C" {

int zkwg_set_prepare_throttle(zkwg_circuit_t* c, int rsa_wavefronts_per_cu) {
  if (!c || rsa_wavefronts_per_cu < 0) return ZKWG_RC_BAD_ARG;
  c->knob.rsa_wgs_per_cu = rsa_wavefronts_per_cu;
  return ZKWG_RC_OK;
}
int zkwg_set_prepare_mask(zkwg_circuit_t* c, uint32_t kernel_mask) {
  if (!c) return ZKWG_RC_BAD_ARG;
  std::lock_guard<std::mutex> lock(c->dev_mutex);
  c->knob.prep_mask = kernel_mask;
  return ZKWG_RC_OK;
}
int zkwg_set_timing(zkwg_circuit_t* c, int enable) {
  if (!c) return ZKWG_RC_BAD_ARG;
  std::lock_guard<std::mutex> lock(c->dev_mutex);
  c->tm.timing = enable;
  c->tm.ev_valid = false;
  c->tm.prep_valid = false;
  c->tm.launches = 0;
  c->tm.prep_launches = 0;
  return ZKWG_RC_OK;
}
int zkwg_num_kernels(const zkwg_circuit_t* c) { return c->tm.n_kernels; }
const char* zkwg_kernel_name(const zkwg_circuit_t* c, int which) {
  return (which >= 0 && which < c->tm.n_kernels) ? c->tm.kname[which] : "";
}
uint64_t zkwg_kernel_slots(const zkwg_circuit_t* c, int which) {
  return (which >= 0 && which < c->tm.n_kernels) ? c->tm.kslots[which] : 0;
}
// events of kernel `which` in the k-th most recent recorded launch (k = 0: last); false if none
static bool timing_events(zkwg_circuit* c, int which, u64 k, hipEvent_t& a, hipEvent_t& b) {
  if (which == c->tm.n_kernels - 1) {
    if (!c->tm.ev_valid || k >= c->tm.launches || k >= ZK_EV_RING) return false;
    const ZkEvent* ev = c->tm.ev[(c->tm.launches - 1 - k) % ZK_EV_RING];
    a = ev[0]; b = ev[1];
  } else {
    if (!c->tm.prep_valid || k >= c->tm.prep_launches || k >= ZK_EV_RING) return false;
    const ZkEvent* ev = c->tm.pev[(c->tm.prep_launches - 1 - k) % ZK_EV_RING];
    a = ev[which]; b = ev[which + 1];
  }
  return true;
}
int zkwg_last_kernel_ms(zkwg_circuit_t* c, int which, float* ms) {
  if (!c || !ms || which < 0 || which >= c->tm.n_kernels || !c->tm.timing) return ZKWG_RC_BAD_ARG;
  hipEvent_t a, b;
  if (!timing_events(c, which, 0, a, b)) return ZKWG_RC_BAD_ARG;
  if (hipEventSynchronize(b) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  if (hipEventElapsedTime(ms, a, b) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  return ZKWG_RC_OK;
}
int zkwg_timing_summary(zkwg_circuit_t* c, int which, float* total_ms, uint32_t* launches) {
  if (!c || !total_ms || !launches || which < 0 || which >= c->tm.n_kernels || !c->tm.timing) return ZKWG_RC_BAD_ARG;
  float tot = 0.f;
  u64 k = 0;
  hipEvent_t a, b;
  for (; timing_events(c, which, k, a, b); ++k) {
    float ms = 0.f;
    if (hipEventSynchronize(b) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    tot += ms;
  }
  *total_ms = tot;
  *launches = (uint32_t)k;
  return ZKWG_RC_OK;
}

static void fill_bufs(const zkwg_circuit* c, ZkBufs& B, const void* d_in, u64 n, void* d_scratch) {
  const ZkSched& s = c->lay.s;
  u8* scr = (u8*)d_scratch;
  const ZkScratchLayout L = scratch_layout(s, n);
  B.in = (const u8*)d_in;
  B.hst = (u32*)(scr + L.off_hst);
  B.bits = (u64*)(scr + L.off_bits);
  B.small = (u32*)(scr + L.off_small);
  B.frv = (Fr*)(scr + L.off_fr);
  B.frm = (Fr*)(scr + L.off_frm);
  B.invtab = c->tab.d_invtab;
  B.pos_c = c->tab.d_pos;
  B.pos_m = c->tab.d_pos ? c->tab.d_pos + c->tab.pos_dense_off : nullptr;
  B.rtab = c->tab.d_rtab;
  B.invtab_m = c->tab.d_invtab_m;
  B.net_records = c->rx.d_net_records;
  B.net_counts = c->rx.d_net_counts;
  B.net_mask_tab = c->rx.d_net_mask_tab;
  B.net_cclass = c->rx.d_net_cclass; B.net_cdelta = c->rx.d_net_cdelta; B.net_cmask = c->rx.d_net_cmask;
  B.net_bclass = c->rx.d_net_bclass; B.net_bdelta = c->rx.d_net_bdelta; B.net_bmask = c->rx.d_net_bmask;
  B.pos16 = c->tab.d_pos_rs;
  B.pos16_l29 = c->tab.d_pos_l29;
  B.pos2_l29 = c->tab.d_pos_l29 ? c->tab.d_pos_l29 + c->tab.pos2_l29_off : nullptr;
  { static const u32 prio = getenv("ZKWG_RSLB_MERGE_PRIO") ? (u32)atoi(getenv("ZKWG_RSLB_MERGE_PRIO")) : 1u; B.rs_prio = prio; }
  B.rs_stage = (u32*)(scr + L.off_rs_stage);
  B.rs_units = L.rs_units;
  B.rs_zero = c->tab.d_rs_zero;
  B.rs_list = c->tab.d_rs_zero ? (u32*)(scr + L.off_rs_list) : nullptr;
  B.rs_cnt = c->tab.d_rs_zero ? (u32*)(scr + L.off_rs_list + align256(L.rs_units * 2 * 4)) : nullptr;
  B.pos2 = c->tab.d_pos_rs ? c->tab.d_pos_rs + c->tab.pos2_off : nullptr;
  B.pos1 = c->tab.pos1_off ? c->tab.d_pos + c->tab.pos1_off : nullptr;
  B.segs = c->tab.d_segs;
  B.wit = nullptr;
  B.wit_stride16 = 0;
  B.status = nullptr;
  B.n_emails = (u32)n;
  B.e_first = 0;
  B.xcd_remap = c->knob.xcd_remap;
}

static void fill_x3(const zkwg_circuit* c, const ZkBufs& B, ZkX3& A) {
  const ZkSched& s = c->lay.s;
  A.in = B.in; A.bits = B.bits; A.small = B.small; A.frv = B.frv; A.invtab = B.invtab;
  A.ent = c->tab.d_ent; A.segs = c->tab.d_segs; A.wit = B.wit;
  A.frm = B.frm; A.invtab_m = B.invtab_m; A.rtab = B.rtab;
  A.frm_w = B.frm; A.small_w = B.small; A.frv_w = B.frv;
  A.wit_stride16 = B.wit_stride16; A.W = s.W;
  A.in_stride = s.in_stride; A.img_bits = s.img_bits; A.img_small = s.img_small; A.img_fr = s.img_fr; A.inv_half = s.inv_half;
  A.m_dfa_cm = s.m_dfa_cm; A.m_dfa_pm = s.m_dfa_pm; A.m_dfa_st = s.m_dfa_st;
  A.netd = c->rx.d_netd;
  A.nportions = c->tab.n_ent; A.nsegs = s.nsegs; A.e_first = B.e_first; A.n_count = B.n_emails - B.e_first;
  A.xcd_remap = c->knob.xcd_remap; A.limb_off = s.in_off[ZKWG_IN_PUBKEY];
}

// the linear rows of a numbered (`--O0`) circuit that are real sums, for emails [B.e_first, B.n_emails): results go into the image
// extensions (zkwg_o0.h).  Launched at the end of zkwg_prepare_device -- so that in a two-stream pipeline they overlap the
// previous sub-batch's expansion -- on the caller's stream, or behind the removeSoftLineBreaks chain on its side stream (the
// chain writes field elements the rows read; the expansion waits for that stream anyway).
static void launch_o0_rows(const zkwg_circuit* c, const ZkO0Dev& O, const ZkBufs& B, hipStream_t st) {
  ZkX3 A;
  fill_x3(c, B, A);
  const u32 total = B.n_emails - B.e_first;
  for (u32 off = 0; off < total; off += 32768u) {   // the kernels index emails with blockIdx.y
    const u32 cnt = std::min(32768u, total - off);
    A.e_first = B.e_first + off; A.n_count = cnt;
    // zk_o0_generic first: the rows read the codes it leaves
    if (O.n_gen) hipLaunchKernelGGL(zk_o0_generic, dim3((O.n_gen + 255) / 256, cnt), dim3(256), 0, st, A, O);
    if (O.n_small_single) hipLaunchKernelGGL(zk_o0_rows_small, dim3((O.n_small_single + 255) / 256, (cnt + ZK_ROW_EMAILS - 1) / ZK_ROW_EMAILS), dim3(256), 0, st, A, O);
    if (O.n_small_long) hipLaunchKernelGGL(zk_o0_rows_small_long, dim3((O.n_small_long + 3) / 4, (cnt + ZK_ROW_EMAILS - 1) / ZK_ROW_EMAILS), dim3(256), 0, st, A, O);
    if (O.n_small_chains) hipLaunchKernelGGL(zk_o0_chains_small, dim3(O.n_small_chains, cnt), dim3(64), 0, st, A, O);
    if (O.n_fr_groups) hipLaunchKernelGGL(zk_o0_rows_fr, dim3(O.n_fr_groups, (cnt + 63u) / 64u), dim3(64), 0, st, A, O);   // a wavefront = one row x 64 emails
  }
}

int zkwg_prepare_device(zkwg_circuit_t* c, const void* d_in, uint64_t n, void* d_status, void* d_scratch,
                        void* hip_stream) {
  if (!c || !d_in || !d_status || !d_scratch) return ZKWG_RC_BAD_ARG;
  if (c->device < 0) return ZKWG_RC_NO_DEVICE;
  if (n == 0) return ZKWG_RC_OK;
  const ZkSched& s = c->lay.s;
  if (n > 0x3fffffffull) return ZKWG_RC_BAD_ARG;
  if (((uintptr_t)d_scratch & 255) || ((uintptr_t)d_in & 15)) return ZKWG_RC_BAD_ARG;
  std::lock_guard<std::mutex> lock(c->dev_mutex);
  ZkDeviceGuard dg(c->device);
  if (!dg.ok) return ZKWG_RC_HIP_ERROR;
  hipStream_t st = (hipStream_t)hip_stream;
  const u32 ne = (u32)n;
  ZkBufs B;
  fill_bufs(c, B, d_in, n, d_scratch);
  B.status = (int*)d_status;
  const bool tm = c->tm.timing != 0;
  zk_wait_chain(c, d_scratch, st);   // a merge chain of an earlier batch may still be reading this scratch buffer
  if (hipMemsetAsync(B.status, 0, n * sizeof(int), st) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  int ki = 0;
  const ZkEvent* evs = c->tm.pev[c->tm.prep_launches % ZK_EV_RING];
  const u32 pm = c->knob.prep_mask;
  const bool pos9 = s.rsa.present && (s.main_kind == ZKWG_MAIN_EMAIL_VERIFIER || s.app.present) && (pm & 32u);
  // EmailReveal: zk_substr (the RevealSubstring component) and zk_app_tail (packed bytes, nullifier) beside the roles below
  const u32 sub_lds = s.sub.present ? zk_sub_lds_bytes(s.sub.L, s.sub.S) : 0u;
  auto launch_substr = [&](hipStream_t q) {   // one wavefront per email, in[] and the substring in LDS
    if (sub_lds > 48u * 1024u) hipFuncSetAttribute((const void*)zk_substr, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sub_lds);
    hipLaunchKernelGGL(zk_substr, dim3(ne), dim3(64), sub_lds, q, s, B);
  };
  const bool app_side = s.app.present && !tm;
  if (app_side) {
    hipEventRecord(c->rv.dep, st);   // (behind the status memset and whatever wrote the records on this stream)
    for (int i = 0; i < 2; ++i) hipStreamWaitEvent(c->rv.stream[i], c->rv.dep, 0);
    if (pm & 16u) launch_substr(c->rv.stream[0]);
    if (pm & 512u) hipLaunchKernelGGL(zk_app_tail, dim3((ne + 63) / 64), dim3(64), 0, c->rv.stream[1], s, B);
    for (int i = 0; i < 2; ++i) hipEventRecord(c->rv.done[i], c->rv.stream[i]);
  }
  if (tm) hipEventRecord(evs[ki], st);
  if (s.nframes && (pm & 1u)) {
    u32 threads = ne * s.nframes;
    hipLaunchKernelGGL(zk_sha_chain, dim3((threads + 63) / 64), dim3(64), 0, st, s, B);
  }
  if (tm) hipEventRecord(evs[++ki], st);
  if (s.nframes && (pm & 2u)) {
    u64 units = (u64)ne * s.total_blocks;
    // EmailVerifier: round records; the trace only for the readers that address its words (descriptor tables)
    const dim3 g((u32)((units + 63) / 64));
    if (s.fr[0].m_rounds == ~0u) hipLaunchKernelGGL((zk_sha_trace<false, true>), g, dim3(64), 0, st, s, B);
    else if (c->lay.full_W || c->abc.m) hipLaunchKernelGGL((zk_sha_trace<true, true>), g, dim3(64), 0, st, s, B);
    else hipLaunchKernelGGL((zk_sha_trace<true, false>), g, dim3(64), 0, st, s, B);
  }
  if (tm) hipEventRecord(evs[++ki], st);
  if (s.net_mode) {
    // the regex circuit of a loaded template: gate list, one wavefront per email (LDS: value cache + message bytes)
    const u32 ew = 64u / std::max(16u, s.net_lanes);   // emails per wavefront
    if (4u * s.net_lds_words * ew + 16 > 48u * 1024u)   // (gfx950: 160 KB of LDS per CU; the default per-workgroup cap is lower)
      hipFuncSetAttribute((const void*)zk_net_eval, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(4u * s.net_lds_words * ew + 16));
    if (pm & 4u) {
      if (s.net_chain_end) hipLaunchKernelGGL(zk_net_scan, dim3((ne + 63) / 64), dim3(64), 0, st, s, B);   // chain states first: the list's mask words need them
      hipLaunchKernelGGL(zk_net_eval, dim3((ne + ew - 1) / ew), dim3(64), 4u * s.net_lds_words * ew + 16, st, s, B);
    }
    if (tm) hipEventRecord(evs[++ki], st);
  }
  if (s.body && (pm & 8u)) hipLaunchKernelGGL(zk_misc_ev, dim3(ne), dim3(64), 7 * s.fr[0].max_bytes + 64 + ZK_DFA_STATES * 256 + 16, st, s, B);
  if (tm) hipEventRecord(evs[++ki], st);
  if (s.rsa.present && (pm & 16u)) {
    // optional throttle: pad the workgroup's LDS claim so that only `rsa_wgs_per_cu` RSA wavefronts
    // (164 VGPRs each) are resident per CU, leaving registers/slots to a concurrently running zk_expand
    u32 dyn = 0;
    if (c->knob.rsa_wgs_per_cu > 0) {
      const u32 per = (160u * 1024u) / (u32)c->knob.rsa_wgs_per_cu;
      dyn = per > 14u * 1024u ? std::min(per - 14u * 1024u, 50u * 1024u) : 0u;
    }
    hipLaunchKernelGGL(zk_rsa, dim3(ne), dim3(64), dyn, st, s, B);
  }
  if (s.fpg.present && (pm & 16u)) hipLaunchKernelGGL(zk_fpmul_small, dim3((ne + 63) / 64), dim3(64), 0, st, s, B);   // (timed in zk_rsa's slot)
  if (s.sub.present && !s.app.present && (pm & 16u)) launch_substr(st);   // substring mains (timed in zk_rsa's slot)
  if (tm) hipEventRecord(evs[++ki], st);
  if (pos9) {
    // one lane per email once the batch supplies >= 16 wavefronts of them; one wavefront per email below
    if ((int)ne < c->knob.pos_wave_below) hipLaunchKernelGGL(zk_poseidon9_wave, dim3(ne), dim3(64), 0, st, s, B);
    else if (c->knob.pos_lane) hipLaunchKernelGGL(zk_poseidon9, dim3((ne + 63) / 64), dim3(64), 0, st, s, B);
    else hipLaunchKernelGGL(zk_poseidon9_g16, dim3((ne + 3) / 4), dim3(64), 0, st, s, B);
  }
  if (s.app.present) {
    if (app_side) for (int i = 0; i < 2; ++i) hipStreamWaitEvent(st, c->rv.done[i], 0);
    else {   // timed: in line, a slot each
      hipEventRecord(evs[++ki], st);
      if (pm & 16u) launch_substr(st);
      hipEventRecord(evs[++ki], st);
      if (pm & 512u) hipLaunchKernelGGL(zk_app_tail, dim3((ne + 63) / 64), dim3(64), 0, st, s, B);
    }
  }
  if (s.rslb) {
    // removeSoftLineBreaks: chunk hashes (one lane per 16-byte chunk), then the serial merge chain + scans
    if (tm) hipEventRecord(evs[++ki], st);
    const u64 units = (u64)ne * s.rs_nch;
    if (pm & 64u) {
      const dim3 g((u32)((units + 63) / 64));
      if (B.rs_list) {     // constant chunks: split the units, copy the constant ones' signals, hash the others (the grid covers the worst case)
        hipMemsetAsync(B.rs_cnt, 0, 8, st);
        hipLaunchKernelGGL(zk_rslb_classify, dim3((u32)((units + 255) / 256)), dim3(256), 0, st, s, B);
        hipLaunchKernelGGL(zk_rslb_fill_const, dim3(8192), dim3(64), 0, st, s, B);
      }
      hipLaunchKernelGGL(zk_rslb_chunks, g, dim3(64), 0, st, s, B);
    }
    if (tm) hipEventRecord(evs[++ki], st);
    auto launch_chain = [&](hipStream_t q) {   // the serial merge chain, then the scans
      if (c->knob.rs_merge_lanes == 1) hipLaunchKernelGGL(zk_rslb_merge1, dim3((ne + 63u) / 64u), dim3(64), 0, q, s, B);
      else hipLaunchKernelGGL(zk_rslb_merge, dim3((ne + 64u / ZK_RS_MERGE_LANES - 1u) / (64u / ZK_RS_MERGE_LANES)), dim3(64), 0, q, s, B);
      hipLaunchKernelGGL(zk_rslb_scan, dim3((ne + 63) / 64), dim3(64), 0, q, s, B);
    };
    if (c->rs.sync) {
      if (pm & 128u) launch_chain(st);
    } else {
      int slot = -1;
      for (int i = 0; i < ZK_RS_SLOTS; ++i) if (c->rs.scr[i] == d_scratch) slot = i;
      if (slot < 0) { slot = c->rs.next; c->rs.next = (c->rs.next + 1) % ZK_RS_SLOTS; c->rs.scr[slot] = d_scratch; }
      hipEventRecord(c->rs.dep[slot], st);
      // four side streams by default (ZKWG_RSLB_SIDE_STREAMS): a batch's chain then starts when its chunk hashes are done instead of
      // behind the chain of the batch before last (round 6, same box: 53.3 k witnesses/s against 51.9 k with two,
      // profiles/r06/r06_n_rslb_variants.json).  They are lowest-priority streams: their hardware queues come from a pool of their own.
      hipStream_t ss = c->rs.side[slot % c->rs.nside];
      hipStreamWaitEvent(ss, c->rs.dep[slot], 0);
      if (pm & 128u) launch_chain(ss);
      if (pm & 256u) {   // the rows read the chain's field elements: they follow it on the side stream
        if (c->lay.full_W) launch_o0_rows(c, c->o0.d, B, ss);
        if (c->abc.m) launch_o0_rows(c, c->abc.d, B, ss);
      }
      hipEventRecord(c->rs.done[slot], ss);
      if (tm) { hipEventRecord(evs[++ki], ss); c->tm.prep_valid = true; c->tm.prep_launches++; }
      if (hipGetLastError() != hipSuccess) return ZKWG_RC_HIP_ERROR;
      return ZKWG_RC_OK;
    }
  }
  if (s.cea.present) {
    // CleanEmailAddress: chunk hashes (one lane per 16 elements of encoded || decoded), then per email the merges, chains and inversion
    if (tm) hipEventRecord(evs[++ki], st);
    if (pm & 64u) hipLaunchKernelGGL(zk_cea_chunks, dim3((u32)(((u64)ne * s.cea.nch + 63) / 64)), dim3(64), 0, st, s, B);
    if (tm) hipEventRecord(evs[++ki], st);
    if (pm & 128u) hipLaunchKernelGGL(zk_cea_tail, dim3((ne + 63) / 64), dim3(64), 0, st, s, B);
  }
  if (!(s.rslb && !c->rs.sync) && (pm & 256u)) {   // (timed with the last prepare kernel)
    if (c->lay.full_W) launch_o0_rows(c, c->o0.d, B, st);
    if (c->abc.m) launch_o0_rows(c, c->abc.d, B, st);
  }
  if (tm) { hipEventRecord(evs[++ki], st); c->tm.prep_valid = true; c->tm.prep_launches++; }
  if (hipGetLastError() != hipSuccess) return ZKWG_RC_HIP_ERROR;
  return ZKWG_RC_OK;
}

static int expand_impl(zkwg_circuit_t* c, const void* d_in, uint64_t n, const void* d_scratch, uint64_t first,
                       uint64_t count, void* d_out, uint64_t out_stride, void* hip_stream, bool mont, bool abc = false) {
  if (!c || !d_in || !d_out || !d_scratch) return ZKWG_RC_BAD_ARG;
  if (c->device < 0) return ZKWG_RC_NO_DEVICE;
  if (count == 0) return ZKWG_RC_OK;
  const ZkSched& s = c->lay.s;
  if (abc && !c->abc.m) return ZKWG_RC_BAD_CONFIG;
  if (mont && (s.sub.present || s.cea.present)) return ZKWG_RC_BAD_CONFIG;   // substring mains, EmailReveal, CleanEmailAddress: no Montgomery-form output
  // the descriptor table written from: the attached system's A.w | B.w | C.w, a numbered circuit's wires, or none (kept-v1 pieces)
  const ZkO0Dev* OD = abc ? &c->abc.d : (c->lay.full_W ? &c->o0.d : nullptr);
  if (first + count > n || out_stride < (abc ? 3 * c->abc.m : out_W(c)) * 32 || (out_stride & 15)) return ZKWG_RC_BAD_ARG;
  if (((uintptr_t)d_scratch & 255) || ((uintptr_t)d_out & 15)) return ZKWG_RC_BAD_ARG;
  std::lock_guard<std::mutex> lock(c->dev_mutex);
  ZkDeviceGuard dg(c->device);
  if (!dg.ok) return ZKWG_RC_HIP_ERROR;
  hipStream_t st = (hipStream_t)hip_stream;
  if (mont) {
    if (!c->tab.d_rtab || !c->tab.d_invtab_m) {
      // v * R mod r for v < 65536 (2 MiB) and the inverse table in Montgomery form, built once per handle and
      // published together (a half-built pair must never be seen by a later call)
      std::vector<Fr> tab(65536);
      Fr acc = fr_zero();
      const Fr Rm = fr_R();
      for (u32 v = 0; v < 65536; ++v) { tab[v] = acc; acc = fr_add(acc, Rm); }
      std::vector<Fr> inv(c->lay.invtab_host);      // (the standard-form table of s.inv_half, built with the handle)
      for (Fr& x : inv) x = fr_to_mont(x);
      ZkDevMem& M = c->tab.mont;
      M.clear();
      Fr* d_r = M.up(tab);
      Fr* d_i = M.up(inv);
      if (M.failed) { const int rc = M.copy_failed ? ZKWG_RC_HIP_ERROR : ZKWG_RC_OOM; M.clear(); return rc; }
      c->tab.d_rtab = d_r; c->tab.d_invtab_m = d_i;
    }
  }
  // sub-launches: the O0 row kernels index emails with blockIdx.y; zk_expand3's grid is pieces x emails
  u64 sub = OD ? std::min<u64>(count, 32768) : count;
  { const u64 per = OD ? OD->nportions : c->tab.n_ent; if (per) sub = std::min<u64>(sub, std::max<u64>(1, 0x7fffffffull / per)); }
  ZkBufs B;
  fill_bufs(c, B, d_in, n, (void*)d_scratch);
  zk_wait_chain(c, d_scratch, st);   // the merge chain of this scratch buffer may still be running on the side stream
  const bool tm = c->tm.timing != 0;
  const ZkEvent* evs = c->tm.ev[c->tm.launches % ZK_EV_RING];
  if (tm) hipEventRecord(evs[0], st);
  for (u64 off = 0; off < count; off += sub) {
    const u64 cnt = std::min(sub, count - off);
    u8* out_sub = (u8*)d_out + off * out_stride;
    B.wit = (uint4*)out_sub;
    B.wit_stride16 = out_stride / 16;
    B.e_first = (u32)(first + off);
    B.n_emails = (u32)(first + off + cnt);
    ZkX3 A;
    fill_x3(c, B, A);
    const u64 conv = cnt * (u64)(s.img_fr + ZK_MONT_LIMBS);
    if (OD) {
      // numbered circuit (`--O0` / `--O1`), one pass: the rows that are real sums go into the image extensions of these
      // emails, then every wire is written from its descriptor (zkwg_o0.h) -- no staging buffer, no gather
      const ZkO0Dev& O = *OD;
      const u64 units = ((cnt + O.emails_per_wg - 1) / O.emails_per_wg) * (u64)O.nportions;
      if (units > 0x7fffffffull) return ZKWG_RC_BAD_ARG;
      if (mont) hipLaunchKernelGGL(zk_image_to_mont, dim3((u32)((conv + 255) / 256)), dim3(256), 0, st, A);
      const dim3 g3((u32)units), b3(256);
      hipLaunchKernelGGL(mont ? zk_expand3_o0_mont : zk_expand3_o0, g3, b3, 0, st, A, O);
      continue;
    }
    {
      // one piece of 256 K slots per workgroup (zkwg_kernels_expand3.hip)
      const u64 units3 = cnt * (u64)c->tab.n_ent;
      if (units3 > 0x7fffffffull) return ZKWG_RC_BAD_ARG;
      if (mont) hipLaunchKernelGGL(zk_image_to_mont, dim3((u32)((conv + 255) / 256)), dim3(256), 0, st, A);
      const dim3 g3((u32)units3), b3(256);
      // (mont was refused above) EmailReveal without the uniqueness check has no match matrix: the plain kernel serves
      if (s.app.present ? s.sub.uniq != 0 : s.sub.present != 0) hipLaunchKernelGGL(zk_expand3_subm, g3, b3, 0, st, A);
      else if (s.cea.present) hipLaunchKernelGGL(zk_expand3_cea, g3, b3, 0, st, A);
      else hipLaunchKernelGGL(mont ? zk_expand3_mont : zk_expand3, g3, b3, 0, st, A);
    }
  }
  if (tm) { hipEventRecord(evs[1], st); c->tm.ev_valid = true; c->tm.launches++; }
  if (hipGetLastError() != hipSuccess) return ZKWG_RC_HIP_ERROR;
  return ZKWG_RC_OK;
}

int zkwg_expand_device(zkwg_circuit_t* c, const void* d_in, uint64_t n, const void* d_scratch, uint64_t first,
                       uint64_t count, void* d_out, uint64_t out_stride, void* hip_stream) {
  return expand_impl(c, d_in, n, d_scratch, first, count, d_out, out_stride, hip_stream, false);
}
int zkwg_expand_montgomery_device(zkwg_circuit_t* c, const void* d_in, uint64_t n, const void* d_scratch, uint64_t first,
                                  uint64_t count, void* d_out, uint64_t out_stride, void* hip_stream) {
  return expand_impl(c, d_in, n, d_scratch, first, count, d_out, out_stride, hip_stream, true);
}
int zkwg_expand_abc_device(zkwg_circuit_t* c, const void* d_in, uint64_t n, const void* d_scratch, uint64_t first, uint64_t count,
                           int montgomery, void* d_abc, uint64_t abc_stride, void* hip_stream) {
  return expand_impl(c, d_in, n, d_scratch, first, count, d_abc, abc_stride, hip_stream, montgomery != 0, true);
}

int zkwg_calculate_batch_device(zkwg_circuit_t* c, const void* d_in, uint64_t n, void* d_out,
                                uint64_t out_stride, void* d_status, void* d_scratch, void* hip_stream) {
  if (!c || !d_in || !d_out || !d_status || !d_scratch) return ZKWG_RC_BAD_ARG;
  if (n == 0) return ZKWG_RC_OK;
  int rc = zkwg_prepare_device(c, d_in, n, d_status, d_scratch, hip_stream);
  if (rc != ZKWG_RC_OK) return rc;
  return zkwg_expand_device(c, d_in, n, d_scratch, 0, n, d_out, out_stride, hip_stream);
}

// what both input generators check of a batch, and its device-side copy
static int gen_batch(const zkwg_circuit_t* c, const zkwg_dkim_batch* b, ZkDkimBatch& D) {
  if (!b->headers || !b->header_len || !b->pubkey_be || !b->signature_be) return ZKWG_RC_BAD_ARG;
  if (c->lay.s.body && (!b->bodies || !b->body_len || !b->body_hash_b64)) return ZKWG_RC_BAD_ARG;
  if (b->selector_len && !b->selector) return ZKWG_RC_BAD_ARG;
  D.headers = b->headers; D.header_len = b->header_len; D.bodies = b->bodies; D.body_len = b->body_len;
  D.body_hash_b64 = b->body_hash_b64; D.pubkey_be = b->pubkey_be; D.signature_be = b->signature_be;
  D.selector = b->selector; D.header_stride = b->header_stride; D.body_stride = b->body_stride;
  D.selector_len = b->selector_len;
  return ZKWG_RC_OK;
}

int zkwg_generate_inputs_device(zkwg_circuit_t* c, const zkwg_dkim_batch* b, uint64_t n, void* d_records,
                                void* d_gen_status, void* hip_stream) {
  if (!c || !b || !d_records || !d_gen_status) return ZKWG_RC_BAD_ARG;
  if (c->device < 0) return ZKWG_RC_NO_DEVICE;
  // (EmailReveal: its two indices are the caller's here; zkwg_generate_reveal_inputs_device finds them)
  if (c->lay.s.main_kind != ZKWG_MAIN_EMAIL_VERIFIER && !c->lay.s.app.present) return ZKWG_RC_BAD_CONFIG;
  if (n == 0) return ZKWG_RC_OK;
  ZkDkimBatch D;
  const int rc = gen_batch(c, b, D);
  if (rc != ZKWG_RC_OK) return rc;
  ZkDeviceGuard dg(c->device);
  if (!dg.ok) return ZKWG_RC_HIP_ERROR;
  hipLaunchKernelGGL(zk_gen_inputs, dim3((u32)n), dim3(64), 0, (hipStream_t)hip_stream, c->lay.s, D, (u8*)d_records,
                     (int*)d_gen_status, (u32)n);
  return hipGetLastError() == hipSuccess ? ZKWG_RC_OK : ZKWG_RC_HIP_ERROR;
}

int zkwg_generate_reveal_inputs_device(zkwg_circuit_t* c, const zkwg_dkim_batch* b, const zkwg_needles* nd, uint64_t n,
                                       void* d_records, void* d_gen_status, void* hip_stream) {
  if (!c || !b || !nd || !d_records || !d_gen_status) return ZKWG_RC_BAD_ARG;
  if (c->device < 0) return ZKWG_RC_NO_DEVICE;
  if (!c->lay.s.app.present) return ZKWG_RC_BAD_CONFIG;
  if (n == 0) return ZKWG_RC_OK;
  if (n > 0xffffffffull || !nd->bytes || !nd->first) return ZKWG_RC_BAD_ARG;
  if (c->lay.s.app.from_body && b->selector_len) return ZKWG_RC_BAD_ARG;      // the needle cuts the body: a selector beside it is refused
  ZkDkimBatch D;
  const int rc = gen_batch(c, b, D);
  if (rc != ZKWG_RC_OK) return rc;
  ZkNeedles Q;
  Q.bytes = nd->bytes; Q.first = nd->first;
  ZkDeviceGuard dg(c->device);
  if (!dg.ok) return ZKWG_RC_HIP_ERROR;
  hipLaunchKernelGGL(zk_gen_reveal_inputs, dim3((u32)n), dim3(64), 0, (hipStream_t)hip_stream, c->lay.s, D, Q, (u8*)d_records,
                     (int*)d_gen_status, (u32)n);
  return hipGetLastError() == hipSuccess ? ZKWG_RC_OK : ZKWG_RC_HIP_ERROR;
}

}  // extern "C"
