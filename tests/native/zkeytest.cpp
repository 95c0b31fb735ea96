// Host build of csrc/zkwg_zkey_core.h for the CPU tests (tests/test_zkey_core_cpu.py): the zkey / .wtns readers and the row evaluation the
// kernels of zkwg_kernels_zkey.hip compile, with the range checks of zkwg_fr29.h counting (ZKWG_FR29_CHECK).  Test infrastructure only.
#define ZKWG_FR29_CHECK
#include "zkwg_zkey_core.h"

extern "C" {
unsigned long long zt_violations() { return zk_fr29_violations.load(); }
// the checks of zkwg_prover_create_wtns that need no device; info = {nVars, nPublic, rows, constraints evaluated by a wavefront}
int zt_zkey_check(const u8* z, u64 len, u64* info) {
  ZkZkeyHeader H;
  int rc = zk_zkey_header(z, len, H);
  if (rc != ZKWG_RC_OK) return rc;
  ZkZkeyHost T;
  rc = zk_zkey_rows(z, H, T);
  if (rc == ZKWG_RC_OK) rc = zk_zkey_b_bitmaps(z, H);
  if (rc != ZKWG_RC_OK) return rc;
  if (info) { info[0] = H.n_vars; info[1] = H.n_public; info[2] = T.n_rows; info[3] = T.n_long; }
  return ZKWG_RC_OK;
}
int zt_wtns_parse(const u8* p, u64 len, u64* n_witness, u64* values_offset) { return zk_wtns_parse(p, len, n_witness, values_offset); }
// n witnesses -> A.w | B.w | C.w per witness (Montgomery form), as zk_zkey_abc writes them
int zt_abc(const u8* z, u64 len, const u8* wit, u64 stride, u64 n, u8* out, u64 out_stride) {
  ZkZkeyHeader H;
  int rc = zk_zkey_header(z, len, H);
  if (rc != ZKWG_RC_OK) return rc;
  ZkZkeyHost T;
  rc = zk_zkey_rows(z, H, T);
  if (rc != ZKWG_RC_OK) return rc;
  if (stride < 32ull * H.n_vars || out_stride < 96 * T.n_rows) return ZKWG_RC_BAD_ARG;
  zk_zkey_abc_host(T, wit, stride, n, out, out_stride);
  return ZKWG_RC_OK;
}
int zt_range_ok(const u8* wit, u64 n_vars) { return zk_zkey_range_host(wit, n_vars) ? 1 : 0; }
unsigned zt_max_row() { return ZK_ZKEY_MAX_ROW; }
unsigned zt_long_threshold() { return ZK_ZKEY_LONG; }
}
