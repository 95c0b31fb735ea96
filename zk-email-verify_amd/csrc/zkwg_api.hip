// C-ABI of libzkwg.so (see include/zkwg.h), the witness handle: construction from a configuration, a `.sym` / `.r1cs` pair or a
// regex template, destruction, layout and size queries, record packing, attach_r1cs, the .wtns / .sym writers.  The launch
// sequence is in zkwg_launch_api.hip, the host paths in zkwg_hostpath_api.hip; this is the only file of the three that sees the
// circom front end and the layout walkers.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <memory>
#include <map>
#include <thread>
#include <algorithm>
#include <chrono>
#include "zkwg_handle.h"
#include "zkwg_layout.h"
#include "zkwg_build.h"
#include "zkwg_poseidon_sparse.h"
#include "zkwg_poseidon29.h"
#include "zkwg_net_host.h"
#include "zkwg_full.h"

#define ZK_O0_SHORT_ROW 8   // host evaluation of the plan (tests): rows up to this many terms are listed first

ZkRegexPart::~ZkRegexPart() { delete net; }
namespace { struct ZkHandleDelete { void operator()(zkwg_circuit* c) const { delete c; } }; }   // (a type of this file: create_impl's unique_ptr adds no exported symbol)

// inverse table: entry (d + half) holds d^{-1} mod r in standard form, d in [-half, half]
static void build_inv_table(u32 inv_half, std::vector<Fr>& tab) {
  const long long half = (long long)inv_half;
  tab.assign(2 * (u64)inv_half + 1, fr_zero());
  std::vector<Fr> inv(half + 1, fr_zero());  // Montgomery form
  if (half >= 1) inv[1] = fr_R();
  // inv[i] = -(r / i) * inv[r mod i]  (mod r); r / i and r % i by long division on 4 limbs
  for (long long i = 2; i <= half; ++i) {
    const u64 p[4] = {ZK_P0, ZK_P1, ZK_P2, ZK_P3};
    u64 q[4];
    unsigned __int128 rem = 0;
    for (int j = 3; j >= 0; --j) {
      unsigned __int128 cur = (rem << 64) | p[j];
      q[j] = (u64)(cur / (u64)i);
      rem = cur % (u64)i;
    }
    Fr qf{{q[0], q[1], q[2], q[3]}};
    Fr t = fr_mont_mul(fr_to_mont(qf), inv[(u64)rem]);
    inv[i] = fr_neg(t);
  }
  for (long long d = 1; d <= half; ++d) {
    Fr v = fr_from_mont(inv[d]);
    tab[(u64)(half + d)] = v;
    tab[(u64)(half - d)] = fr_neg(v);
  }
}
extern "C" int zk_misc_init_tables(void);

// descriptor + row tables of a numbered layout (zkwg_o0.h) onto the device; the host copy keeps its counters only
static bool upload_o0(const zkwg_circuit* c, ZkO0Part& P, ZkO0Tables& T, u64 W, bool keep_host = false) {
  P.clear();
  ZkO0Dev& O = P.d;
  ZkDevMem& M = P.mem;
  O.desc = (const uint2*)M.up(T.desc); O.aff = (const uint4*)M.up(T.aff);
  O.s_ptr = M.up(T.s_ptr); O.s_term = (const uint2*)M.up(T.s_term); O.s_coef = M.up(T.s_coef); O.s_out = M.up(T.s_out);
  {
    // small rows: the groups of one row (a thread each, a wavefront for the long ones) and the chains (a wavefront each)
    std::vector<u32> single, lng, chains;
    for (size_t g = 0; g + 1 < T.s_group.size(); ++g) {
      const u32 a = T.s_group[g], b = T.s_group[g + 1];
      if (b - a == 1) (T.s_ptr[a + 1] - T.s_ptr[a] > ZK_ROW_LONG ? lng : single).push_back(a); else { chains.push_back(a); chains.push_back(b - a); }
    }
    O.s_single = M.up(single); O.s_long = M.up(lng); O.s_chains = (const uint2*)M.up(chains);
    O.n_small_single = (u32)single.size(); O.n_small_long = (u32)lng.size(); O.n_small_chains = (u32)(chains.size() / 2);
  }
  O.f_ptr = M.up(T.f_ptr); O.f_term = (const uint2*)M.up(T.f_term); O.f_coef = M.up(T.f_coef); O.f_coefm = M.up(T.f_coefm); O.f_kind = M.up(T.f_kind);
  O.gen_seg = M.up(T.gen_seg); O.gen_r = M.up(T.gen_r);
  O.n_gen = (u32)T.gen_seg.size(); O.gen_base = T.gen_base;
  O.W = W; O.nportions = (u32)((W + 256u * ZK_X3_SLOTS_O0 - 1) / (256u * ZK_X3_SLOTS_O0)); O.small_base = T.small_base; O.fr_base = T.fr_base;
  O.emails_per_wg = (u32)c->knob.o0_emails_per_wg;
  O.n_fr_groups = (u32)T.n_fr();   // (field rows are never chained: one group each)
  if (M.failed) { P.clear(); return false; }
  if (!keep_host) { ZkO0Tables keep; keep.small_base = T.small_base; keep.fr_base = T.fr_base; keep.gen_base = T.gen_base; keep.n_alias = T.n_alias; keep.n_const = T.n_const; std::swap(T, keep); }
  return true;
}
extern "C" {

int zkwg_abi_version(void) { return ZKWG_ABI_VERSION; }

const char* zkwg_strerror(int rc) {
  switch (rc) {
    case ZKWG_RC_OK: return "ok";
    case ZKWG_ERR_ASSERT_FAILED: return "Error: Assert Failed.";
    case 1: return "Signal not found";
    case 2: return "Too many signals set";
    case 3: return "Signal already set";
    case 5: return "Not enough memory";
    case 6: return "Input signal array access exceeds the size";
    case ZKWG_ERR_WITNESS_NOT_REDUCED: return "zkwg: a witness value is not below the field order";
    case ZKWG_DKIM_NOT_FOUND: return "DKIM signature not found for domain";
    case ZKWG_DKIM_MULTIPLE_FROM: return "Multiple From header in email and domain for verification not specified";
    case ZKWG_DKIM_NO_KEY: return "no key";
    case ZKWG_DKIM_BODY_HASH: return "body hash did not verify";
    case ZKWG_DKIM_BAD_SIGNATURE: return "bad signature";
    case ZKWG_DKIM_UNSUPPORTED: return "unsupported";
    case ZKWG_DKIM_BODY_DOES_NOT_FIT: return "body does not fit";
    case ZKWG_RC_BAD_CONFIG: return "zkwg: unsupported circuit configuration";
    case ZKWG_RC_BAD_ARG: return "zkwg: bad argument";
    case ZKWG_RC_NO_DEVICE: return "zkwg: no HIP device (layout-only handle or HIP unavailable)";
    case ZKWG_RC_HIP_ERROR: return "zkwg: HIP runtime error";
    case ZKWG_RC_OOM: return "zkwg: out of device memory";
    default: return "zkwg: unknown code";
  }
}

static thread_local std::string g_last_error;
const char* zkwg_last_error(void) { return g_last_error.c_str(); }
void zk_set_last_error(const char* m) { g_last_error = m; }      // for the C-ABI files beside this one (zkwg_setup_api.hip)

static int create_impl(const zkwg_config* cfg_in, int device, const char* sym_text, uint64_t sym_len,
                       const char* alias_text, uint64_t alias_len, zkwg_circuit_t** out,
                       const uint8_t* r1cs = nullptr, uint64_t r1cs_len = 0, const zkwg_regex_source* regex = nullptr,
                       const zkwg_app_config* app = nullptr) {
  if (!cfg_in || !out) return ZKWG_RC_BAD_ARG;
  if (cfg_in->main_kind == ZKWG_MAIN_EMAIL_REVEAL && !app) {
    g_last_error = "ZKWG_MAIN_EMAIL_REVEAL takes its parameters from zkwg_app_config: create the handle with zkwg_circuit_create_app";
    return ZKWG_RC_BAD_CONFIG;
  }
  if (app && cfg_in->main_kind != ZKWG_MAIN_EMAIL_REVEAL) { g_last_error = "zkwg_circuit_create_app builds ZKWG_MAIN_EMAIL_REVEAL only"; return ZKWG_RC_BAD_CONFIG; }
  zkwg_config cfg_copy = *cfg_in;
  cfg_copy.layout = ZKWG_LAYOUT_KEPT_V1;
  const zkwg_config* cfg = &cfg_copy;
  std::unique_ptr<zkwg_circuit, ZkHandleDelete> owner(new zkwg_circuit());   // every exit below is a plain return: the handle's owners release what it holds
  zkwg_circuit* c = owner.get();
  c->lay.cfg = *cfg;
  if (app) c->lay.app = *app;
  // tuning knobs
  { const char* v = getenv("ZKWG_RSLB_MERGE_LANES"); c->knob.rs_merge_lanes = v && atoi(v) == 4 ? 4 : 1; }
  c->knob.o0_emails_per_wg = getenv("ZKWG_O0_EMAILS_PER_WG") ? std::max(1, atoi(getenv("ZKWG_O0_EMAILS_PER_WG"))) : 16;
  c->knob.xcd_remap = getenv("ZKWG_XCD_REMAP") ? (u32)atoi(getenv("ZKWG_XCD_REMAP")) : 1u;
  if (const char* v = getenv("ZKWG_RSA_WGS_PER_CU")) c->knob.rsa_wgs_per_cu = atoi(v);
  if (regex) {
    // the regex circuit is compiled from the supplied template text (zkwg_circom.h)
    if (!regex->circom_path || cfg->main_kind != ZKWG_MAIN_EMAIL_VERIFIER || cfg->ignore_body_hash_check) {
      g_last_error = "a regex template needs an EmailVerifier configuration with the body-hash check";
      return ZKWG_RC_BAD_CONFIG;
    }
    std::string err;
    c->rx.net = new zkc::Net();
    if (!zkc::load(regex->circom_path, regex->include_dirs ? regex->include_dirs : "",
                   regex->template_name ? regex->template_name : "BodyHashRegex", {(zkc::i64)cfg->max_header}, *c->rx.net, err)) {
      g_last_error = "regex template: " + err;
      return ZKWG_RC_BAD_CONFIG;
    }
    // the scan tables against the plain gate list on a few messages, once per handle (zkwg_net_host.h; ZKWG_NET_SELFCHECK=0 skips it)
    if (!getenv("ZKWG_NET_SELFCHECK") || atoi(getenv("ZKWG_NET_SELFCHECK"))) {
      if (!zkc::self_check(regex->circom_path, regex->include_dirs ? regex->include_dirs : "",
                           regex->template_name ? regex->template_name : "BodyHashRegex", {(zkc::i64)cfg->max_header}, *c->rx.net, err)) {
        g_last_error = "regex template: " + err;
        return ZKWG_RC_BAD_CONFIG;
      }
    }
  }
  const zkc::Net* net = c->rx.net;
  const bool dbg_t = getenv("ZKWG_DEBUG_TIMING") != nullptr;
  auto t_last = std::chrono::steady_clock::now();
  auto phase = [&](const char* what) {
    if (!dbg_t) return;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[zkwg] create: %-28s %7.2f s\n", what, std::chrono::duration<double>(now - t_last).count());
    t_last = now;
  };
  if (!build_sched(*cfg, c->lay.s, c->lay.segs, net, app)) {
    g_last_error = "unsupported circuit configuration";
    if (cfg->main_kind == ZKWG_MAIN_CLEAN_EMAIL_ADDRESS)
      g_last_error = !zk_cea_length_ok(cfg->max_header) ? "CleanEmailAddress: maxLength must be a multiple of 8 with 8 <= maxLength <= 1024"
                     : cfg->max_body != cfg->max_header ? "CleanEmailAddress: max_body must equal max_header (both are maxLength)"
                                                        : "CleanEmailAddress: n, k and every flag must be 0";
    return ZKWG_RC_BAD_CONFIG;
  }
  if (c->rx.net) {   // how a slot of the template's region is decoded, with host pointers (host expansion, layout-only handles); the device copy follows
    ZkNetDec& D = c->rx.h_netd;
    D.pd = c->rx.net->pd.data(); D.tab = c->rx.net->tabs.data();
    D.offF = c->rx.net->offF; D.offB = c->rx.net->offB; D.nL = c->rx.net->nL; D.nF = c->rx.net->nF; D.nB = c->rx.net->nB; D.b_fdim = c->rx.net->bchain.fdim;
    D.m_net = c->lay.s.m_net; D.m_net_pw = c->lay.s.m_net_pw; D.n_in = c->rx.net->n_in;
  }
  if (getenv("ZKWG_DEBUG_SKIP_INV") && atoi(getenv("ZKWG_DEBUG_SKIP_INV")) && c->lay.s.rsa.present) c->lay.s.rsa.present = 2;  // profiling only
  if (c->lay.s.sub.present && (sym_text || r1cs)) { g_last_error = "the substring mains have no .sym / numbered layout"; return ZKWG_RC_BAD_CONFIG; }
  if (c->lay.s.cea.present && (sym_text || r1cs)) { g_last_error = "CleanEmailAddress has no .sym / numbered layout"; return ZKWG_RC_BAD_CONFIG; }
  if (sym_text) {
    ZkSymLayout L;
    L.allow_holes = r1cs != nullptr;
    // a compact `.sym` (no .r1cs): zk_expand writes the file's order directly (segments remapped).  A fully numbered
    // circuit (.r1cs given): every wire of the file gets a descriptor over the compact image or a linear row over
    // kept-v1 slots (zkwg_full.h -> zkwg_o0.h); zk_expand3_o0 writes the file's witness in one pass
    phase("schedule");
    // the two files are independent until the linear plan: the .r1cs is parsed on its own thread(s) while the .sym is laid out
    // (both are threaded inside; their serial stretches hide behind each other)
    ZkR1csHost R;
    bool r1cs_ok = true;
    std::thread r1cs_thread;
    std::exception_ptr r1cs_err, sym_err;      // neither thread may leave an exception unjoined: both are rethrown below, joined
    if (r1cs) r1cs_thread = std::thread([&] { try { r1cs_ok = zk_r1cs_parse(r1cs, r1cs_len, R); } catch (...) { r1cs_err = std::current_exception(); } });
    bool sym_ok = false;
    try { sym_ok = zk_sym_layout(c->lay.s, sym_text, sym_len, alias_text, alias_len, L, net); } catch (...) { sym_err = std::current_exception(); }
    if (r1cs_thread.joinable()) r1cs_thread.join();
    if (sym_err || r1cs_err) { std::rethrow_exception(sym_err ? sym_err : r1cs_err); }      // -> create_guarded's catch (ZKWG_RC_OOM / BAD_CONFIG)
    if (!sym_ok || (!r1cs && !zk_remap_segments(c->lay.s, c->lay.segs, L))) {
      g_last_error = L.err.empty() ? std::string(".sym layout does not tile the witness") : L.err;
      return ZKWG_RC_BAD_CONFIG;
    }
    if (r1cs) {
      // every signal the schedule does not produce must follow from the circuit's own linear constraints
      std::string err;
      std::vector<u8> produced(L.W, 0);
      for (u64 i = 0; i < L.W; ++i) produced[i] = L.hole[i] ? 0 : 1;
      phase(".sym layout | .r1cs parse");
      if (!r1cs_ok) err = "the .r1cs file could not be parsed";
      else if (R.n_wires != L.W) err = "the .r1cs has " + std::to_string(R.n_wires) + " wires, the .sym file numbers " + std::to_string(L.W);
      else zk_linear_plan(R, produced, c->lay.lin_host, err);
      phase("linear plan");
      if (err.empty()) {
        // wire -> where its value comes from: a kept-v1 slot (bit 31 clear) or a linear row over kept-v1 slots
        const ZkLinPlan& Pn = c->lay.lin_host;
        std::vector<u32> inv(L.W, 0xffffffffu);
        for (u64 slot = 0; slot < L.dst.size(); ++slot) if (L.dst[slot] != 0xffffffffu) inv[L.dst[slot]] = (u32)slot;
        c->lay.o0_desc.assign(L.W, 0xffffffffu);
        for (u64 w = 0; w < L.W; ++w) if (!L.hole[w]) c->lay.o0_desc[w] = inv[w];
        c->lay.o0_src.resize(Pn.src.size());
        for (size_t t = 0; t < Pn.src.size() && err.empty(); ++t) {
          c->lay.o0_src[t] = inv[Pn.src[t]];
          if (c->lay.o0_src[t] == 0xffffffffu) err = "internal: a linear row reads a wire the schedule does not produce";
        }
        for (u64 r = 0; r < Pn.n_rows(); ++r) {
          const u64 a = Pn.row_ptr[r], b = Pn.row_ptr[r + 1];
          if (b - a == 1 && Pn.kind[a] == ZK_COEF_ONE) c->lay.o0_desc[Pn.dst[r]] = c->lay.o0_src[a];   // alias: the wire copies its source's descriptor
          else { c->lay.o0_desc[Pn.dst[r]] = 0xfffffffeu; (b - a > ZK_O0_SHORT_ROW ? c->lay.o0_long : c->lay.o0_short).push_back((u32)r); }   // zk_o0_rows
        }
        c->lay.n_o0_short = c->lay.o0_short.size();
        c->lay.o0_long.insert(c->lay.o0_long.begin(), c->lay.o0_short.begin(), c->lay.o0_short.end());   // [short rows | long rows]
        std::vector<u32>().swap(c->lay.o0_short);
        for (u64 w = 0; w < L.W && err.empty(); ++w)
          if (c->lay.o0_desc[w] == 0xffffffffu || (!(c->lay.o0_desc[w] >> 31) && c->lay.o0_desc[w] >= c->lay.s.W)) err = "internal: wire " + std::to_string(w) + " has no source";
        if (Pn.n_rows() >= 0x7fffffffull || c->lay.s.W >= 0x7fffffffull) err = "circuit too large for the O0 gather table";
        c->lay.full_W = L.W;
        c->lay.lin_rows = Pn.n_rows();
        phase("wire table");
        if (err.empty()) zk_o0_build(c->lay.s, c->lay.segs, Pn, c->lay.o0_desc, c->lay.o0_src, c->o0.t, err);
        phase("descriptor / row tables");
        if (getenv("ZKWG_DEBUG_PLAN"))
          fprintf(stderr, "[zkwg] O0 tables: %llu wires, %llu alias rows, %llu constant rows, %llu small rows (%llu terms in %llu groups), %llu field rows (%llu terms in %llu groups); %llu terms before chaining\n",
                  (unsigned long long)L.W, (unsigned long long)c->o0.t.n_alias, (unsigned long long)c->o0.t.n_const, (unsigned long long)c->o0.t.n_small(),
                  (unsigned long long)c->o0.t.s_coef.size(), (unsigned long long)(c->o0.t.s_group.size() - 1), (unsigned long long)c->o0.t.n_fr(),
                  (unsigned long long)c->o0.t.f_kind.size(), (unsigned long long)(c->o0.t.f_group.size() - 1), (unsigned long long)c->o0.t.terms_before_chaining);
        if (getenv("ZKWG_DEBUG_PLAN")) {
          u64 hist[8] = {0}, terms = 0, longest = 0;
          for (u64 r = 0; r < Pn.n_rows(); ++r) {
            const u64 n = Pn.row_ptr[r + 1] - Pn.row_ptr[r];
            terms += n; longest = std::max(longest, n);
            ++hist[n == 0 ? 0 : n == 1 ? 1 : n == 2 ? 2 : n <= 4 ? 3 : n <= 16 ? 4 : n <= 64 ? 5 : n <= 256 ? 6 : 7];
          }
          std::map<std::string, std::pair<u64, u64>> by;   // template-ish key -> (rows, terms) of the long rows
          for (u64 r = 0; r < Pn.n_rows(); ++r) {
            const u64 n = Pn.row_ptr[r + 1] - Pn.row_ptr[r];
            if (n <= 8) continue;
            std::string nm = L.names[Pn.dst[r]], key;
            for (char ch : nm) if (!isdigit((unsigned char)ch)) key += ch;
            by[key].first++; by[key].second += n;
          }
          std::vector<std::pair<u64, std::string>> top;
          for (auto& kv : by) top.emplace_back(kv.second.second, kv.first + " rows=" + std::to_string(kv.second.first));
          std::sort(top.rbegin(), top.rend());
          for (size_t i = 0; i < top.size() && i < 14; ++i) fprintf(stderr, "[zkwg]   %llu terms: %s\n", (unsigned long long)top[i].first, top[i].second.c_str());
          fprintf(stderr, "[zkwg] O0 plan: %llu rows, %llu terms, longest %llu; rows with 0/1/2/3-4/5-16/17-64/65-256/>256 terms: %llu %llu %llu %llu %llu %llu %llu %llu\n",
                  (unsigned long long)Pn.n_rows(), (unsigned long long)terms, (unsigned long long)longest, (unsigned long long)hist[0], (unsigned long long)hist[1],
                  (unsigned long long)hist[2], (unsigned long long)hist[3], (unsigned long long)hist[4], (unsigned long long)hist[5], (unsigned long long)hist[6], (unsigned long long)hist[7]);
        }
      }
      if (!err.empty()) { g_last_error = err; return ZKWG_RC_BAD_CONFIG; }
    }
    c->lay.sym_names.swap(L.names);
    c->lay.kept_dst.swap(L.dst);
    c->lay.cfg.layout = ZKWG_LAYOUT_SYM;
  }
  // kernel table (launch order)
  {
    int k = 0;
    c->tm.kname[k++] = "zk_sha_chain";
    c->tm.kname[k++] = "zk_sha_trace";
    if (c->lay.s.net_mode) c->tm.kname[k++] = "zk_net_eval";
    c->tm.kname[k++] = "zk_misc_ev";
    c->tm.kname[k++] = "zk_rsa";
    c->tm.kname[k++] = "zk_poseidon9";
    if (c->lay.s.app.present) { c->tm.kname[k++] = "zk_substr"; c->tm.kname[k++] = "zk_app_tail"; }
    if (c->lay.s.rslb) { c->tm.kname[k++] = "zk_rslb_chunks"; c->tm.kname[k++] = "zk_rslb_chain"; }
    if (c->lay.s.cea.present) { c->tm.kname[k++] = "zk_cea_chunks"; c->tm.kname[k++] = "zk_cea_tail"; }
    c->tm.n_kernels = k + 1;
    for (int i = 0; i < k; ++i) c->tm.kslots[i] = 0;
  }
  build_inv_table(c->lay.s.inv_half, c->lay.invtab_host);   // (also the host expansion's table)
  c->tm.kname[c->tm.n_kernels - 1] = "zk_expand"; c->tm.kslots[c->tm.n_kernels - 1] = c->lay.full_W ? c->lay.full_W : c->lay.s.W;   // (zk_expand3_o0 for a fully numbered circuit)
  if (device >= 0) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) { return ZKWG_RC_NO_DEVICE; }
    if (hipSetDevice(device) != hipSuccess) { return ZKWG_RC_HIP_ERROR; }
    c->device = device;
    if (zk_misc_init_tables() != 0) { return ZKWG_RC_HIP_ERROR; }
    ZkDevMem& TM = c->tab.mem;
    c->tab.d_invtab = TM.up(c->lay.invtab_host);
    c->tab.d_segs = TM.up(c->lay.segs);
    {
      std::vector<ZkPortionEntry> ent;
      zk_build_entries(c->lay.s.W, c->lay.segs, ent, 256u * ZK_X3_SLOTS);
      c->tab.n_ent = (u32)ent.size();
      c->tab.d_ent = TM.up(ent);
    }
    bool ok = !TM.failed;
    if (ok && c->rx.net) {
      zkc::Net& N = *c->rx.net;
      ZkDevMem& RM = c->rx.mem;
      c->rx.d_net_records = RM.up(N.records);
      c->rx.d_net_counts = RM.up(N.step_count, 64);
      c->rx.d_net_mask_tab = RM.up(N.mask_tab); c->rx.d_net_pd = RM.up(N.pd); c->rx.d_net_tabs = RM.up(N.tabs);
      c->rx.d_net_cmask = RM.up(N.chain.mask);
      c->rx.d_net_bmask = RM.up(N.bchain.mask);
      {
        ZkNetDec D = c->rx.h_netd;
        D.pd = c->rx.d_net_pd; D.tab = c->rx.d_net_tabs;
        c->rx.d_netd = (ZkNetDec*)RM.up(&D, sizeof(D));
      }
      c->rx.d_net_cclass = RM.up(N.chain.cls); c->rx.d_net_cdelta = RM.up(N.chain.delta);
      c->rx.d_net_bclass = RM.up(N.bchain.cls); c->rx.d_net_bdelta = RM.up(N.bchain.delta);
      ok = !RM.failed;
      if (ok) for (zkc::ChainTab* t : {&N.chain, &N.bchain}) { std::vector<u32>().swap(t->tab); std::vector<u32>().swap(t->mask); }
      if (ok) std::vector<u32>().swap(N.fn_tab);
      if (ok) std::vector<u32>().swap(N.records);
    }
    if (ok && c->lay.full_W) {
      // numbered circuit: descriptors + row tables on the device (the host copies of the plan are dropped)
      ok = upload_o0(c, c->o0, c->o0.t, c->lay.full_W);
      if (ok) {
        ZkLinPlan empty; std::swap(c->lay.lin_host, empty);
        std::vector<u32>().swap(c->lay.o0_desc); std::vector<u32>().swap(c->lay.o0_src); std::vector<u32>().swap(c->lay.o0_long);
      }
    }
    if (ok && (c->lay.s.main_kind == ZKWG_MAIN_EMAIL_VERIFIER || c->lay.s.app.present)) {
      std::vector<Fr> C, M, t10;
      build_poseidon_constants(10, 8, 60, C, M);
      ok = zk_build_poseidon_sparse(10, 60, C, M, t10);
      c->tab.pos_dense_off = (u32)t10.size();
      t10.insert(t10.end(), C.begin(), C.end());     // dense tables for zk_poseidon9_wave
      t10.insert(t10.end(), M.begin(), M.end());
      {
        // additive constants of the sparse rounds in Montgomery form (zk_poseidon9_g16 keeps its state in Montgomery form)
        const u32 T = 10, RP = 60;
        const size_t c_part = 4 * T + T * T, c_last = c_part + RP * T + RP * (2 * T - 1) + T * T;
        std::vector<Fr> cm;
        for (u32 i = 0; i < 4 * T; ++i) cm.push_back(fr_to_mont(t10[i]));
        for (u32 i = 0; i < RP * T; ++i) cm.push_back(fr_to_mont(t10[c_part + i]));
        for (u32 i = 0; i < 4 * T; ++i) cm.push_back(fr_to_mont(t10[c_last + i]));
        t10.insert(t10.end(), cm.begin(), cm.end());
      }
      if (ok && c->lay.s.app.nullifier) {   // EmailNullifier's outer Poseidon(1): t = 2, R_P = 56
        std::vector<Fr> C1, M1, t2;
        build_poseidon_constants(2, 8, 56, C1, M1);
        ok = zk_build_poseidon_sparse(2, 56, C1, M1, t2);
        c->tab.pos1_off = (u32)t10.size();
        t10.insert(t10.end(), t2.begin(), t2.end());
      }
      if (ok) c->tab.d_pos = TM.up(t10);
    }
    if (ok && (c->lay.s.rslb || c->lay.s.cea.present)) {   // PoseidonModular: Poseidon(16) chunks, Poseidon(2) merges
      std::vector<Fr> C, M, t16, t2;
      build_poseidon_constants(17, 8, 68, C, M);
      ok = zk_build_poseidon_sparse(17, 68, C, M, t16);
      build_poseidon_constants(3, 8, 57, C, M);
      ok = ok && zk_build_poseidon_sparse(3, 57, C, M, t2);
      std::vector<u32> l29, l29_2;
      if (ok) { zk_build_poseidon29(17, 68, t16, l29); zk_build_poseidon29(3, 57, t2, l29_2); }
      const size_t n16 = l29.size();
      c->tab.pos2_l29_off = (u32)n16;
      l29.insert(l29.end(), l29_2.begin(), l29_2.end());
      if (ok) c->tab.d_pos_l29 = TM.up(l29);
      { const char* v = getenv("ZKWG_RSLB_CONST_CHUNKS");
        if (ok && c->lay.s.rslb && !(v && atoi(v) == 0)) {
          // Poseidon(16)(0, ..., 0): the same evaluator on the host (element j, limb l at st[l * 17 + j])
          std::vector<u32> st0(9 * 17, 0u);
          std::vector<Fr> z(ZK_P16_KEPT + 1);
          z[ZK_P16_KEPT] = zk_poseidon29<17, 0>(st0.data(), 1, 17, l29.data(), 68, z.data());
          c->tab.d_rs_zero = TM.up(z);
        } }
      c->tab.pos2_off = (u32)t16.size();
      t16.insert(t16.end(), t2.begin(), t2.end());
      if (ok) c->tab.d_pos_rs = TM.up(t16);
    }
    if (!ok || TM.failed) return ZKWG_RC_OOM;
    // streams and events: each owner destroys what it created, so a failure part-way is a plain return as well
    ok = c->hb.own_stream.create() && c->hb.copy_stream.create();
    if (c->lay.s.rslb) {
      // lowest priority: ROCm keeps separate hardware-queue pools per stream priority, so the side streams
      // never share a queue with the caller's (normal / high priority) prepare and expand streams -- a shared
      // queue would put the next batch's kernels behind a 0.2 s chain.  The chain has 1 wave per 64 emails;
      // dispatch priority does not slow it down once resident.
      int prio_lo = 0, prio_hi = 0;
      ok = ok && hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) == hipSuccess;
      for (int i = 0; i < ZK_RS_SLOTS; ++i) ok = ok && c->rs.side[i].create(prio_lo) && c->rs.dep[i].create() && c->rs.done[i].create();
      c->rs.sync = getenv("ZKWG_RSLB_SYNC") ? atoi(getenv("ZKWG_RSLB_SYNC")) : 0;
      c->rs.nside = getenv("ZKWG_RSLB_SIDE_STREAMS") ? std::min(ZK_RS_SLOTS, std::max(1, atoi(getenv("ZKWG_RSLB_SIDE_STREAMS")))) : 4;
    }
    if (c->lay.s.app.present) {
      ok = ok && c->rv.dep.create();
      for (int i = 0; i < 2; ++i) ok = ok && c->rv.stream[i].create() && c->rv.done[i].create();
    }
    c->knob.pos_lane = getenv("ZKWG_POS_LANE") ? atoi(getenv("ZKWG_POS_LANE")) : 0;
    c->knob.pos_wave_below = getenv("ZKWG_POS_WAVE_BELOW") ? atoi(getenv("ZKWG_POS_WAVE_BELOW")) : 1024;
    for (int i = 0; i < 2; ++i) ok = ok && c->hb.done[i].create() && c->hb.copied[i].create();
    for (int r = 0; r < ZK_EV_RING; ++r) {
      for (int i = 0; i < 2; ++i) ok = ok && c->tm.ev[r][i].create(hipEventDefault);
      for (int i = 0; i <= ZK_MAX_KERNELS; ++i) ok = ok && c->tm.pev[r][i].create(hipEventDefault);
    }
    if (!ok) return ZKWG_RC_HIP_ERROR;
  }
  *out = owner.release();
  return ZKWG_RC_OK;
}

// no C++ exception may cross the C ABI (ctypes / N-API callers would abort)
static int create_guarded(const zkwg_config* cfg, int device, const char* sym_text, uint64_t sym_len,
                          const char* alias_text, uint64_t alias_len, zkwg_circuit_t** out,
                          const uint8_t* r1cs = nullptr, uint64_t r1cs_len = 0, const zkwg_regex_source* regex = nullptr,
                          const zkwg_app_config* app = nullptr) {
  try {
    return create_impl(cfg, device, sym_text, sym_len, alias_text, alias_len, out, r1cs, r1cs_len, regex, app);
  } catch (const std::bad_alloc&) {
    g_last_error = "out of host memory while building the circuit";
    return ZKWG_RC_OOM;
  } catch (const std::exception& e) {
    g_last_error = std::string("circuit construction failed: ") + e.what();
    return ZKWG_RC_BAD_CONFIG;
  }
}
int zkwg_circuit_create(const zkwg_config* cfg, int device, zkwg_circuit_t** out) {
  if (cfg && cfg->layout != ZKWG_LAYOUT_KEPT_V1) { g_last_error = "layout SYM needs zkwg_circuit_create_sym"; return ZKWG_RC_BAD_CONFIG; }
  return create_guarded(cfg, device, nullptr, 0, nullptr, 0, out);
}
int zkwg_circuit_create_sym(const zkwg_config* cfg, int device, const char* sym_text, uint64_t sym_len,
                            const char* alias_text, uint64_t alias_len, zkwg_circuit_t** out) {
  if (!sym_text) return ZKWG_RC_BAD_ARG;
  return create_guarded(cfg, device, sym_text, sym_len, alias_text, alias_len, out);
}

int zkwg_circuit_create_full(const zkwg_config* cfg, int device, const char* sym_text, uint64_t sym_len,
                             const char* alias_text, uint64_t alias_len, const uint8_t* r1cs, uint64_t r1cs_len,
                             zkwg_circuit_t** out) {
  if (!sym_text || !r1cs) return ZKWG_RC_BAD_ARG;
  return create_guarded(cfg, device, sym_text, sym_len, alias_text, alias_len, out, r1cs, r1cs_len);
}
int zkwg_circuit_create_regex(const zkwg_config* cfg, int device, const zkwg_regex_source* regex,
                              const char* sym_text, uint64_t sym_len, const char* alias_text, uint64_t alias_len,
                              const uint8_t* r1cs, uint64_t r1cs_len, zkwg_circuit_t** out) {
  if (!regex || !regex->circom_path) return ZKWG_RC_BAD_ARG;
  if (r1cs && !sym_text) return ZKWG_RC_BAD_ARG;
  return create_guarded(cfg, device, sym_text, sym_len, alias_text, alias_len, out, r1cs, r1cs_len, regex);
}
int zkwg_circuit_create_app(const zkwg_config* cfg, const zkwg_app_config* app, int device, zkwg_circuit_t** out) {
  if (!app) return ZKWG_RC_BAD_ARG;
  return create_guarded(cfg, device, nullptr, 0, nullptr, 0, out, nullptr, 0, nullptr, app);
}
int zkwg_regex_info(const zkwg_circuit_t* c, uint64_t out[8]) {
  if (!c || !out) return ZKWG_RC_BAD_ARG;
  if (!c->rx.net) return ZKWG_RC_BAD_CONFIG;
  const zkc::Net& n = *c->rx.net;
  out[0] = n.n_kept; out[1] = n.n_temp; out[2] = n.n_gates; out[3] = n.n_asserts;
  out[4] = n.n_chunks; out[5] = n.n_steps; out[6] = n.n_pins; out[7] = n.n_general;
  return ZKWG_RC_OK;
}
// layout-only handles (device < 0): evaluate the linear completion of one host witness in place (tests)
int zkwg_linear_complete_host(const zkwg_circuit_t* c, uint8_t* witness) {
  if (!c || !witness) return ZKWG_RC_BAD_ARG;
  const ZkLinPlan& Pn = c->lay.lin_host;
  if (c->lay.lin_rows && !Pn.n_rows()) return ZKWG_RC_BAD_CONFIG;   // a device handle keeps its plan on the device only
  for (u64 r = 0; r < Pn.n_rows(); ++r)
    ((Fr*)witness)[Pn.dst[r]] = zk_linear_row(Pn.row_ptr.data(), Pn.src.data(), Pn.coef.data(), Pn.kind.data(), r, (const Fr*)witness);
  return ZKWG_RC_OK;
}
// layout-only handles: the linear plan of a fully numbered circuit (copies + rows over the kept-v1 witness) on the host -- every
// wire of the file from one compact kept-v1 witness through the wire table (tests)
int zkwg_o0_gather_host(const zkwg_circuit_t* c, const uint8_t* kept_witness, uint8_t* out) {
  if (!c || !kept_witness || !out) return ZKWG_RC_BAD_ARG;
  if (!c->lay.full_W || c->lay.o0_desc.size() != c->lay.full_W) return ZKWG_RC_BAD_CONFIG;
  const ZkLinPlan& Pn = c->lay.lin_host;
  const Fr* kw = (const Fr*)kept_witness;
  Fr* o = (Fr*)out;
  for (u64 w = 0; w < c->lay.full_W; ++w) {
    const u32 d = c->lay.o0_desc[w];
    if (d != 0xfffffffeu) o[w] = kw[d];
  }
  for (u32 r : c->lay.o0_long)   // [short rows | long rows]
    o[Pn.dst[r]] = zk_linear_row(Pn.row_ptr.data(), c->lay.o0_src.data(), Pn.coef.data(), Pn.kind.data(), r, kw);
  return ZKWG_RC_OK;
}
int zkwg_image_layout(const zkwg_circuit_t* c, uint64_t n, zkwg_image_layout_t* o) {
  if (!c || !o) return ZKWG_RC_BAD_ARG;
  const ZkSched& s = c->lay.s;
  o->hstate_words = (u64)s.hstates_per_email * 8; o->bits_words = s.img_bits; o->small_words = s.img_small; o->fr_elems = s.img_fr;
  const ZkScratchLayout L = scratch_layout(s, n);
  o->off_hstates = L.off_hst; o->off_bits = L.off_bits; o->off_small = L.off_small; o->off_fr = L.off_fr;
  o->total_bytes = L.total;
  return ZKWG_RC_OK;
}
uint64_t zkwg_segment_table(const zkwg_circuit_t* c, zkwg_segment* out, uint64_t cap) {
  if (!c) return 0;
  static_assert(sizeof(zkwg_segment) == sizeof(ZkSeg), "public segment struct must mirror ZkSeg");
  const u64 n = std::min<u64>(cap, c->lay.segs.size());
  if (out) memcpy(out, c->lay.segs.data(), n * sizeof(ZkSeg));
  // the record-decoded SHA types are reported as the documented trace-decoded ones (same src, a, b; c = the round record)
  for (u64 i = 0; out && i < n; ++i)
    switch (out[i].type) {
      case ZSEG_SHAR_SP: out[i].type = ZSEG_SHA_SP; break;
      case ZSEG_SHAR_T1: out[i].type = ZSEG_SHA_T1; break;
      case ZSEG_SHAR_T2: out[i].type = ZSEG_SHA_T2; break;
      case ZSEG_SHAR_SUM: out[i].type = ZSEG_BITS; break;
      default: break;
    }
  return c->lay.segs.size();
}
uint32_t zkwg_inverse_table_half(const zkwg_circuit_t* c) { return c ? c->lay.s.inv_half : 0; }
uint64_t zkwg_layout_map(const zkwg_circuit_t* c, uint32_t* out, uint64_t cap) {
  if (!c) return 0;
  if (out) for (u64 i = 0; i < c->lay.kept_dst.size() && i < cap; ++i) out[i] = c->lay.kept_dst[i];
  return c->lay.kept_dst.size();
}
uint64_t zkwg_linear_rows(const zkwg_circuit_t* c) { return c ? (c->lay.lin_rows ? c->lay.lin_rows : c->lay.lin_host.n_rows()) : 0; }

void zkwg_circuit_destroy(zkwg_circuit_t* c) {
  if (!c) return;
  if (c->device < 0) { delete c; return; }
  ZkDeviceGuard dg(c->device);
  // the side streams may still be running a batch's tail over the handle's tables; everything else is the owners' (zkwg_handle.h)
  for (const ZkStream& q : c->rv.stream) if (q) hipStreamSynchronize(q);
  for (const ZkStream& q : c->rs.side) if (q) hipStreamSynchronize(q);
  delete c;
}

uint64_t zkwg_witness_len(const zkwg_circuit_t* c) { return out_W(c); }
uint64_t zkwg_witness_bytes(const zkwg_circuit_t* c) { return out_W(c) * 32; }
uint32_t zkwg_num_public(const zkwg_circuit_t* c) { return c->lay.s.n_public; }
uint64_t zkwg_input_stride(const zkwg_circuit_t* c) { return c->lay.s.in_stride; }
uint64_t zkwg_input_offset(const zkwg_circuit_t* c, int field) {
  if (field < 0 || field >= ZKWG_IN_NFIELDS) return (uint64_t)-1;
  return c->lay.s.in_off[field];
}
uint64_t zkwg_scratch_bytes(const zkwg_circuit_t* c, uint64_t n) { return scratch_layout(c->lay.s, n).total; }
uint64_t zkwg_scratch_bytes_standard(const zkwg_circuit_t* c, uint64_t n) { return scratch_layout(c->lay.s, n).total_std; }

int zkwg_pack_input(const zkwg_circuit_t* c, uint8_t* rec, const uint8_t* header, uint32_t header_len,
                    const uint8_t* body, uint32_t body_len, const uint8_t* pre, const uint8_t* pubkey,
                    const uint8_t* sig, const uint8_t* msg, uint32_t bh_index) {
  if (!c || !rec) return ZKWG_RC_BAD_ARG;
  const ZkSched& s = c->lay.s;
  memset(rec, 0, s.in_stride);
  if (header) memcpy(rec + s.in_off[ZKWG_IN_HEADER], header, c->lay.cfg.max_header);
  if (body) memcpy(rec + s.in_off[ZKWG_IN_BODY], body, c->lay.cfg.max_body);
  if (pre) memcpy(rec + s.in_off[ZKWG_IN_PRECOMPUTED_SHA], pre, 32);
  if (pubkey) memcpy(rec + s.in_off[ZKWG_IN_PUBKEY], pubkey, 17 * 16);
  if (sig) memcpy(rec + s.in_off[ZKWG_IN_SIGNATURE], sig, 17 * 16);
  if (msg) memcpy(rec + s.in_off[ZKWG_IN_MESSAGE], msg, 17 * 16);
  memcpy(rec + s.in_off[ZKWG_IN_HEADER_LEN], &header_len, 4);
  memcpy(rec + s.in_off[ZKWG_IN_BODY_LEN], &body_len, 4);
  memcpy(rec + s.in_off[ZKWG_IN_BODY_HASH_INDEX], &bh_index, 4);
  return ZKWG_RC_OK;
}

int zkwg_pack_field(const zkwg_circuit_t* c, uint8_t* rec, int field, uint64_t first, const uint8_t* values32,
                    uint64_t count) {
  if (!c || !rec || !values32 || field < 0 || field >= ZKWG_IN_NFIELDS || field == ZKWG_IN_RANGE_FLAGS) return ZKWG_RC_BAD_ARG;
  const ZkSched& s = c->lay.s;
  u64 cap = 0;
  u32 width = 1;   // bytes per packed element
  switch (field) {
    case ZKWG_IN_HEADER: cap = c->lay.cfg.max_header; break;
    case ZKWG_IN_BODY: cap = c->lay.cfg.max_body; break;
    case ZKWG_IN_PRECOMPUTED_SHA: cap = 32; break;
    case ZKWG_IN_PUBKEY: case ZKWG_IN_SIGNATURE: case ZKWG_IN_MESSAGE: cap = 17; width = 16; break;
    case ZKWG_IN_HEADER_LEN: case ZKWG_IN_BODY_LEN: case ZKWG_IN_BODY_HASH_INDEX: cap = 1; width = 4; break;
    case ZKWG_IN_HEADER_MASK: cap = s.mask_header ? c->lay.cfg.max_header : 0; break;
    case ZKWG_IN_BODY_MASK: cap = s.mask_body ? c->lay.cfg.max_body : 0; break;
    case ZKWG_IN_DECODED_BODY: cap = s.rslb ? c->lay.cfg.max_body : 0; break;
    case ZKWG_IN_SUBSTRING_START: case ZKWG_IN_SUBSTRING_LEN: cap = s.app.present ? 1 : 0; width = 4; break;
  }
  if (first > cap || count > cap - first) return ZKWG_RC_BAD_ARG;
  u32 flags;
  memcpy(&flags, rec + s.in_off[ZKWG_IN_RANGE_FLAGS], 4);
  const Fr p = fr_p();
  for (u64 i = 0; i < count; ++i) {
    Fr v;
    memcpy(v.l, values32 + 32 * i, 32);
    while (fr_geq(v, p)) { u64 bw; v = fr_sub_raw(v, p, bw); }   // circom_runtime: normalize(BigInt(v), prime)
    u8* dst = rec + s.in_off[field] + (first + i) * width;
    bool fits;
    if (width == 1) { fits = !(v.l[0] >> 8) && !v.l[1] && !v.l[2] && !v.l[3]; dst[0] = (u8)v.l[0]; }
    else if (width == 4) { fits = !(v.l[0] >> 32) && !v.l[1] && !v.l[2] && !v.l[3]; const u32 w = (u32)v.l[0]; memcpy(dst, &w, 4); }
    else { fits = !v.l[2] && !v.l[3]; memcpy(dst, v.l, 16); }
    if (!fits) flags |= 1u << field;
  }
  memcpy(rec + s.in_off[ZKWG_IN_RANGE_FLAGS], &flags, 4);
  return ZKWG_RC_OK;
}

int zkwg_pack_masks(const zkwg_circuit_t* c, uint8_t* rec, const uint8_t* header_mask, const uint8_t* body_mask) {
  if (!c || !rec) return ZKWG_RC_BAD_ARG;
  if (header_mask && c->lay.s.mask_header) memcpy(rec + c->lay.s.in_off[ZKWG_IN_HEADER_MASK], header_mask, c->lay.cfg.max_header);
  if (body_mask && c->lay.s.mask_body) memcpy(rec + c->lay.s.in_off[ZKWG_IN_BODY_MASK], body_mask, c->lay.cfg.max_body);
  return ZKWG_RC_OK;
}
int zkwg_pack_decoded_body(const zkwg_circuit_t* c, uint8_t* rec, const uint8_t* decoded_body) {
  if (!c || !rec || !decoded_body || !c->lay.s.rslb) return ZKWG_RC_BAD_ARG;
  memcpy(rec + c->lay.s.in_off[ZKWG_IN_DECODED_BODY], decoded_body, c->lay.cfg.max_body);
  return ZKWG_RC_OK;
}

// ---- the first Groth16 prover stage from the compact image -------------------------------------------
// A.w, B.w, C.w of every constraint are linear combinations over the witness, exactly like the wires of a numbered
// circuit that are sums of others: the 3 m combinations become one more descriptor table (zkwg_o0.h) over the image --
// a combination that is one wire copies that wire's descriptor, one of bits / small integers with small coefficients is
// a 64-bit integer row, the rest are rows mod r -- and zk_expand3_o0 streams them out.  No 32-byte witness is read.
int zkwg_circuit_attach_r1cs(zkwg_circuit_t* c, const uint8_t* r1cs, uint64_t len) {
  if (!c || !r1cs) return ZKWG_RC_BAD_ARG;
  // lock order of the host-buffer path: hb_mutex, then dev_mutex.  Both are held: the attachment grows the image layout (c->lay.s)
  // that the host-path calls read under hb_mutex and the device entry points under dev_mutex.
  std::lock_guard<std::mutex> hb_lock(c->hb_mutex);
  std::lock_guard<std::mutex> lock(c->dev_mutex);
  if (c->abc.m) { g_last_error = "attach_r1cs: the handle already has a constraint system"; return ZKWG_RC_BAD_CONFIG; }
  if (c->lay.s.sub.present) { g_last_error = "attach_r1cs: not available for the substring mains and EmailReveal"; return ZKWG_RC_BAD_CONFIG; }
  if (c->lay.s.cea.present) { g_last_error = "attach_r1cs: not available for CleanEmailAddress"; return ZKWG_RC_BAD_CONFIG; }
  try {
    ZkR1csHost R;
    if (!zk_r1cs_parse(r1cs, len, R)) { g_last_error = "the .r1cs file could not be parsed: " + R.err; return ZKWG_RC_BAD_CONFIG; }
    // A numbered handle (zkwg_circuit_create_full) is keyed to the compiler's `.r1cs` -- the system a zkey carries
    // (packages/helpers/src/chunked-zkey.ts:80-84): its wires are the file's, not kept-v1 slots.
    const bool numbered = c->lay.full_W != 0;
    const u64 n_wires = numbered ? c->lay.full_W : c->lay.s.W;
    if (R.n_wires != n_wires) { g_last_error = "the .r1cs has " + std::to_string(R.n_wires) + " wires, the witness layout " + std::to_string(n_wires); return ZKWG_RC_BAD_CONFIG; }
    const u64 m = R.n_constraints;
    if (3 * m >= 0x7fffffffull) { g_last_error = "too many constraints"; return ZKWG_RC_BAD_CONFIG; }
    // numbered: wire -> kept-v1 slot it copies, or its definition over kept-v1 slots (the linear plan of zkwg_full.h, derived
    // again from this file: the handle dropped its host copy after building the device tables)
    std::vector<u32> inv;
    std::vector<u64> row_of;
    ZkLinPlan Pn;
    if (numbered) {
      if (c->lay.kept_dst.empty()) { g_last_error = "attach_r1cs: the numbered handle has no layout map"; return ZKWG_RC_BAD_CONFIG; }
      inv.assign(n_wires, 0xffffffffu);
      for (u64 slot = 0; slot < c->lay.kept_dst.size(); ++slot) if (c->lay.kept_dst[slot] != 0xffffffffu && c->lay.kept_dst[slot] < n_wires) inv[c->lay.kept_dst[slot]] = (u32)slot;
      std::vector<u8> produced(n_wires, 0);
      for (u64 w = 0; w < n_wires; ++w) produced[w] = inv[w] != 0xffffffffu;
      std::string perr;
      if (!zk_linear_plan(R, produced, Pn, perr)) { g_last_error = perr; return ZKWG_RC_BAD_CONFIG; }
      row_of.assign(n_wires, ~0ull);
      for (u64 r = 0; r < Pn.n_rows(); ++r) row_of[Pn.dst[r]] = r;
    }
    // output order: the A values, then B, then C (zkwg_r1cs_evaluate_device's)
    ZkLinPlan P;
    std::vector<u32> desc_slot(3 * m);
    P.row_ptr.assign(1, 0);
    P.src.reserve(R.wire.size()); P.coef.reserve(R.wire.size()); P.kind.reserve(R.wire.size());
    const Fr one_m = fr_R(), minus_one_m = fr_neg(fr_R());
    std::vector<std::pair<u32, Fr>> acc;
    for (u32 which = 0; which < 3; ++which)
      for (u64 i = 0; i < m; ++i) {
        const u64 a = R.row_ptr[3 * i + which], b = R.row_ptr[3 * i + which + 1];
        const u64 dst = (u64)which * m + i;
        const u64 t0 = P.src.size();
        if (!numbered) {
          for (u64 t = a; t < b; ++t) {
            if (R.wire[t] >= n_wires) { g_last_error = "the .r1cs names a wire outside the witness"; return ZKWG_RC_BAD_CONFIG; }
            P.src.push_back(R.wire[t]); P.coef.push_back(fr_from_mont(R.coef[t])); P.kind.push_back(R.kind[t]);
          }
        } else {
          // substitute every wire by its kept-v1 source(s), merge equal slots (Montgomery coefficients throughout)
          acc.clear();
          for (u64 t = a; t < b; ++t) {
            const u32 w = R.wire[t];
            if (w >= n_wires) { g_last_error = "the .r1cs names a wire outside the witness"; return ZKWG_RC_BAD_CONFIG; }
            if (inv[w] != 0xffffffffu) { acc.emplace_back(inv[w], R.coef[t]); continue; }
            const u64 r = row_of[w];
            if (r == ~0ull) { g_last_error = "internal: wire " + std::to_string(w) + " has neither a slot nor a definition"; return ZKWG_RC_BAD_CONFIG; }
            for (u64 q = Pn.row_ptr[r]; q < Pn.row_ptr[r + 1]; ++q) {
              const u32 sl = inv[Pn.src[q]];
              if (sl == 0xffffffffu) { g_last_error = "internal: a linear row reads a wire the schedule does not produce"; return ZKWG_RC_BAD_CONFIG; }
              const u8 k = Pn.kind[q];
              acc.emplace_back(sl, k == ZK_COEF_ONE ? R.coef[t] : (k == ZK_COEF_MINUS_ONE ? fr_neg(R.coef[t]) : fr_mont_mul(R.coef[t], fr_to_mont(Pn.coef[q]))));
            }
          }
          if (acc.size() > 1) std::stable_sort(acc.begin(), acc.end(), [](const std::pair<u32, Fr>& x, const std::pair<u32, Fr>& y) { return x.first < y.first; });
          for (size_t t = 0; t < acc.size();) {
            Fr sum = acc[t].second;
            size_t q = t + 1;
            while (q < acc.size() && acc[q].first == acc[t].first) { sum = fr_add(sum, acc[q].second); ++q; }
            if (!fr_is_zero(sum)) {
              P.src.push_back(acc[t].first); P.coef.push_back(fr_from_mont(sum));
              P.kind.push_back(fr_eq(sum, one_m) ? ZK_COEF_ONE : (fr_eq(sum, minus_one_m) ? ZK_COEF_MINUS_ONE : ZK_COEF_GENERIC));
            }
            t = q;
          }
        }
        P.row_ptr.push_back(P.src.size());
        P.dst.push_back((u32)dst);
        desc_slot[dst] = (P.src.size() - t0 == 1 && P.kind[t0] == ZK_COEF_ONE) ? P.src[t0] : 0xfffffffeu;
      }
    { ZkLinPlan e; std::swap(Pn, e); std::vector<u64>().swap(row_of); std::vector<u32>().swap(inv); }
    std::string err;
    ZkSched s2 = c->lay.s;   // (the image grows by the row results: committed only when everything succeeded)
    ZkO0Tables T;         // (built aside: a failed attachment leaves the handle as it was)
    if (!zk_o0_build(s2, c->lay.segs, P, desc_slot, P.src, T, err)) { g_last_error = err; return ZKWG_RC_BAD_CONFIG; }
    if (getenv("ZKWG_DEBUG_PLAN"))
      fprintf(stderr, "[zkwg] A.w|B.w|C.w tables: %llu combinations, %llu single wires, %llu empty, %llu small rows (%llu terms), %llu field rows (%llu terms), %llu pre-decoded slots; image %u -> %u small words, %u -> %u field elements\n",
              (unsigned long long)(3 * m), (unsigned long long)T.n_alias, (unsigned long long)T.n_const, (unsigned long long)T.n_small(),
              (unsigned long long)T.s_coef.size(), (unsigned long long)T.n_fr(), (unsigned long long)T.f_kind.size(),
              (unsigned long long)T.gen_seg.size(), c->lay.s.img_small, s2.img_small, c->lay.s.img_fr, s2.img_fr);
    if (c->device >= 0) {
      ZkDeviceGuard dg(c->device);
      if (!dg.ok) return ZKWG_RC_HIP_ERROR;
      if (!upload_o0(c, c->abc, T, 3 * m, true)) return ZKWG_RC_OOM;   // (the host copy serves zkwg_expand_abc_host)
    }
    c->abc.t = std::move(T);
    c->lay.s = s2;
    c->abc.m = m;
    // the cached staging buffers of the host paths were sized for the old image layout (zkwg_scratch_bytes grew):
    // drop them, the next zkwg_calculate_batch / _resident allocates them again
    if (c->device >= 0 && (c->hb.tile || c->hb.hx_bytes || c->rp.scr_bytes)) {
      ZkDeviceGuard dg(c->device);
      hipDeviceSynchronize();
      c->hb.clear();
      c->rp.clear_scratch();
    }
  } catch (const std::bad_alloc&) {
    return ZKWG_RC_OOM;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return ZKWG_RC_BAD_CONFIG;
  }
  return ZKWG_RC_OK;
}
uint64_t zkwg_abc_bytes(const zkwg_circuit_t* c) { return c ? 96 * c->abc.m : 0; }

uint64_t zkwg_wtns_size(const zkwg_circuit_t* c) { return 12 + 12 + 40 + 12 + out_W(c) * 32; }

int zkwg_write_wtns(const zkwg_circuit_t* c, const uint8_t* witness, uint8_t* out, uint64_t cap) {
  if (!c || !witness || !out) return ZKWG_RC_BAD_ARG;
  if (cap < zkwg_wtns_size(c)) return ZKWG_RC_BAD_ARG;
  u8* p = out;
  auto w32 = [&](u32 v) { memcpy(p, &v, 4); p += 4; };
  auto w64 = [&](u64 v) { memcpy(p, &v, 8); p += 8; };
  memcpy(p, "wtns", 4); p += 4;
  w32(2); w32(2);
  w32(1); w64(40);
  w32(32);
  const u64 prime[4] = {ZK_P0, ZK_P1, ZK_P2, ZK_P3};
  memcpy(p, prime, 32); p += 32;
  w32((u32)out_W(c));
  w32(2); w64(out_W(c) * 32);
  memcpy(p, witness, out_W(c) * 32);
  return ZKWG_RC_OK;
}

uint64_t zkwg_write_sym(const zkwg_circuit_t* c, char* out, uint64_t cap) {
  ZkSched tmp = c->lay.s;
  ZkWalker w;
  w.net = c->rx.net;
  w.names = true;
  u64 pos = 0;
  auto put = [&](u64 slot, const std::string& name) {
    char buf[64];
    int n = snprintf(buf, sizeof(buf), "%llu,%llu,0,", (unsigned long long)slot, (unsigned long long)slot);
    u64 need = (u64)n + name.size() + 1;
    if (out && pos + need <= cap) {
      memcpy(out + pos, buf, n);
      memcpy(out + pos + n, name.data(), name.size());
      out[pos + n + name.size()] = '\n';
    }
    pos += need;
  };
  if (!c->lay.sym_names.empty()) {
    for (u64 i = 0; i < c->lay.sym_names.size(); ++i) put(i, c->lay.sym_names[i]);
    return pos;
  }
  w.sink = put;
  zk_walk_main(w, tmp);
  return pos;
}

}  // extern "C"
