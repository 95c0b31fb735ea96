// C-ABI of DKIM verification of raw emails (include/zkwg.h "DKIM verification of raw emails"): zkwg_dkim_parse, zkwg_dkim_verify_batch,
// zkwg_dkim_batch_free.  The host parses every message and canonicalises its signed header (csrc/zkwg_dkim_host.h); the bodies go to the
// device once, 16-byte aligned in one buffer, and three kernels (csrc/zkwg_kernels_dkim.hip) leave the canonical bodies, both digests,
// the verdicts and the filled zkwg_dkim_batch there.  device = -1 runs the same cores on host threads.
#include <string.h>
#include <algorithm>
#include <exception>
#include <memory>
#include <thread>
#include <hip/hip_runtime.h>
#include "zkwg_dkim_host.h"
#include "zkwg_points_host.h"

#if !defined(__HIP_DEVICE_COMPILE__)
namespace {
static_assert(sizeof(ZkDkimKey) == sizeof(zkwg_dkim_key), "ZkDkimKey is zkwg_dkim_key");
static_assert(sizeof(ZkDkimRec) == 80, "ZkDkimRec");

// f(i) for i < n on up to `threads` threads.  An exception in a worker (the parser allocates) does not leave its thread: the first one is
// kept and thrown again here, on the caller's thread, after every worker has ended.
template <class F> void parallel_for(u64 n, int threads, F f) {
  const int t = (int)std::max<u64>(1, std::min<u64>((u64)std::max(threads, 1), n));
  if (t == 1) { for (u64 i = 0; i < n; ++i) f(i); return; }
  std::vector<std::thread> pool;
  std::vector<std::exception_ptr> err((size_t)t);
  for (int k = 0; k < t; ++k)
    pool.emplace_back([&, k] {
      try {
        for (u64 i = (u64)k; i < n; i += (u64)t) f(i);
      } catch (...) {
        err[(size_t)k] = std::current_exception();
      }
    });
  for (std::thread& th : pool) th.join();
  for (const std::exception_ptr& e : err) if (e) std::rethrow_exception(e);
}

// 0 = as many host threads as the machine has, at most 16
int host_threads(int asked) { return asked > 0 ? asked : (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency())); }

struct Host {      // what the parser leaves for a batch
  std::vector<zkwg_dkim_parsed> parsed;
  std::vector<ZkDkimRec> recs;
  std::vector<u8> headers, sigs, bh64;
  std::vector<u32> header_len;
};

// the verdict of one email on the host: the statements of zk_dkim_verify
void verify_host(const ZkDkimRec& r, const zkwg_dkim_key* keys, u32 fits, const u8* body_digest, const u8* header_digest, const u8* sig, u32 flags,
                 int32_t& status, int32_t& key_index) {
  int st = r.pre_status, idx = -1;
  if (!st && !fits) st = ZK_DKIM_ST_DOES_NOT_FIT;
  if (!st && !(flags & ZKWG_DKIM_SKIP_BODY_HASH) && memcmp(body_digest, r.bh, 32) != 0) st = ZK_DKIM_ST_BODY_HASH;
  if (!st && r.key_count == 0) st = ZK_DKIM_ST_NO_KEY;
  if (!st) {
    u32 usable = 0;
    for (u32 k = 0; k < r.key_count && idx < 0; ++k) {
      const zkwg_dkim_key& key = keys[r.key_first + k];
      if (!zk_dkim_key_usable(key.bits, key.exponent)) continue;
      ++usable;
      if (zkdkim::rsa_host(key.modulus_be, sig, header_digest)) idx = (int)k;
    }
    if (idx < 0) st = usable ? ZK_DKIM_ST_BAD_SIGNATURE : ZK_DKIM_ST_UNSUPPORTED;
  }
  status = st; key_index = idx;
}
}  // namespace

extern "C" {

int zkwg_dkim_parse(const uint8_t* raw, uint64_t len, const char* domain, uint8_t* header_out, uint32_t header_cap, zkwg_dkim_parsed* out) {
  if (!out || (len && !raw)) return ZKWG_RC_BAD_ARG;
  try {
    return zkdkim::parse(raw, len, domain, header_out, header_cap, out);
  } catch (const std::bad_alloc&) {
    return ZKWG_RC_OOM;
  }
}

int zkwg_dkim_parse_batch(uint64_t n, const uint8_t* const* emails, const uint64_t* email_len, const char* domain, int32_t threads, zkwg_dkim_parsed* out) {
  if (n && (!emails || !email_len || !out)) return ZKWG_RC_BAD_ARG;
  for (u64 i = 0; i < n; ++i) if (email_len[i] && !emails[i]) return ZKWG_RC_BAD_ARG;
  try {
    parallel_for(n, host_threads(threads), [&](u64 i) {
      zkwg_dkim_parsed& P = out[i];
      if (zkdkim::parse(emails[i], email_len[i], domain, nullptr, 0xffffffffu, &P) != ZKWG_DKIM_PASS) return;
      const u8* body = emails[i] + P.body_offset;
      u64 bare = 0;                              // a relaxed body grows by one CR per LF that has none; SP c only replaces a blank
      for (const u8* q = body, *end = body + P.body_len; (q = (const u8*)memchr(q, '\n', (size_t)(end - q))) != nullptr; ++q) bare += q == body || q[-1] != '\r';
      P.body_bound = P.body_len + bare + 2;
    });
    return ZKWG_RC_OK;
  } catch (const std::bad_alloc&) {
    return ZKWG_RC_OOM;
  }
}

int zkwg_dkim_batch_free(int device, zkwg_dkim_batch* b) {
  if (!b) return ZKWG_RC_BAD_ARG;
  if (device < 0) return ZKWG_RC_NO_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return ZKWG_RC_HIP_ERROR;
  const void* p[] = {b->headers, b->header_len, b->bodies, b->body_len, b->body_hash_b64, b->pubkey_be, b->signature_be};
  for (const void* q : p) if (q) hipFree((void*)q);
  memset(b, 0, sizeof *b);
  return ZKWG_RC_OK;
}

int zkwg_dkim_verify_batch(const zkwg_dkim_verify_args* A) {
  if (!A || (A->n && (!A->emails || !A->email_len || !A->key_first || !A->status)) || A->n > 0x7fffffffu || !A->header_stride || !A->body_stride) return ZKWG_RC_BAD_ARG;
  if (A->device < 0 && A->device_batch) return ZKWG_RC_NO_DEVICE;
  const u64 n = A->n;
  const u32 hs = A->header_stride, bs = A->body_stride;
  for (u64 i = 0; i < n; ++i)
    if ((A->email_len[i] && !A->emails[i]) || A->key_first[i + 1] < A->key_first[i] || (A->key_first[n] && !A->keys)) return ZKWG_RC_BAD_ARG;
  if (A->seconds) for (int i = 0; i < 6; ++i) A->seconds[i] = 0;
  try {
    double t = now();
    Host H;
    H.parsed.resize(n); H.recs.resize(n); H.headers.assign(n * hs, 0); H.sigs.assign(n * 256, 0); H.bh64.assign(n * 44, 0); H.header_len.assign(n, 0);
    // host threads: the parser and the packing of the bodies on the device path, everything with device = -1 (0 = up to 16 of the machine's)
    const int threads = host_threads(A->threads);
    parallel_for(n, threads, [&](u64 i) {
      zkwg_dkim_parsed& P = H.parsed[i];
      zkdkim::parse(A->emails[i], A->email_len[i], A->domain, H.headers.data() + i * hs, hs, &P);
      ZkDkimRec& r = H.recs[i];
      memset(&r, 0, sizeof r);
      r.l = P.l; r.raw_len = (u32)P.body_len; r.body_mode = P.body_canon; r.has_l = P.has_l; r.pre_status = P.status;
      r.key_first = A->key_first[i]; r.key_count = A->key_first[i + 1] - A->key_first[i];
      memcpy(r.bh, P.bh, 32);
      if (P.status == ZKWG_DKIM_PASS) {
        H.header_len[i] = P.header_len;
        memcpy(H.sigs.data() + 256 * i, P.signature, 256);
        memcpy(H.bh64.data() + 44 * i, P.bh_b64, 44);
      } else {
        r.raw_len = 0;
      }
    });
    if (A->parsed) memcpy(A->parsed, H.parsed.data(), n * sizeof(zkwg_dkim_parsed));
    if (A->seconds) { A->seconds[0] = now() - t; t = now(); }
    const bool want_bodies = A->bodies != nullptr;
    if (A->header_len) memcpy(A->header_len, H.header_len.data(), 4 * n);
    if (A->headers) for (u64 i = 0; i < n; ++i) memcpy(A->headers + i * hs, H.headers.data() + i * hs, H.header_len[i]);

    if (A->device < 0) {
      // the same cores on the host; a caller that does not want the bodies still needs them for the digests: rows of the call's own,
      // not filled beforehand (a row is written up to its body's length by the thread that then hashes that much of it)
      std::unique_ptr<u8[]> own;
      u8* bodies = A->bodies;
      if (!want_bodies) { own.reset(new u8[n * bs ? n * bs : 1]); bodies = own.get(); }
      std::vector<u32> blen(n, 0), fits(n, 1);
      std::vector<u8> bd(32 * n, 0), hd(32 * n, 0);
      double t_body = 0, t_hash = 0, t_ver = 0;
      const bool timed = A->seconds != nullptr;
      auto stage = [&](int which) {
        parallel_for(n, threads, [&](u64 i) {
          const ZkDkimRec& r = H.recs[i];
          if (which == 0) {
            if (r.pre_status == 0)
              blen[i] = zk_dkim_body_serial(A->emails[i] + H.parsed[i].body_offset, r.raw_len, r.body_mode, r.has_l != 0, r.l, bodies + i * bs, bs, &fits[i]);
          } else if (which == 1) {
            if (r.pre_status == 0) {
              if (fits[i]) zkdkim::sha256_host(bodies + i * bs, blen[i], bd.data() + 32 * i);
              zkdkim::sha256_host(H.headers.data() + i * hs, H.header_len[i], hd.data() + 32 * i);
            }
          } else {
            int32_t ki = -1;
            verify_host(r, A->keys, fits[i], bd.data() + 32 * i, hd.data() + 32 * i, H.sigs.data() + 256 * i, A->flags, A->status[i], ki);
            if (A->key_index) A->key_index[i] = ki;
          }
        });
      };
      stage(0); if (timed) { t_body = now() - t; t = now(); }
      stage(1); if (timed) { t_hash = now() - t; t = now(); }
      stage(2); if (timed) { t_ver = now() - t; t = now(); }
      if (timed) { A->seconds[2] = t_body; A->seconds[3] = t_hash; A->seconds[4] = t_ver; }
      if (A->body_len) memcpy(A->body_len, blen.data(), 4 * n);
      if (A->body_digest) memcpy(A->body_digest, bd.data(), 32 * n);
      if (A->header_digest) memcpy(A->header_digest, hd.data(), 32 * n);
      return ZKWG_RC_OK;
    }

    if (hipSetDevice(A->device) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    if (!n) { if (A->device_batch) memset(A->device_batch, 0, sizeof *A->device_batch); return ZKWG_RC_OK; }
    hipStream_t st = nullptr;
    // the raw bodies, each at a multiple of 16 bytes
    u64 total = 0;
    for (u64 i = 0; i < n; ++i) { H.recs[i].raw_off = total; total += ((u64)H.recs[i].raw_len + 15) & ~15ull; }
    std::unique_ptr<u8[]> raw(new u8[total ? total : 16]);          // (not zeroed: every byte is written below)
    parallel_for(n, threads, [&](u64 i) {
      const u32 len = H.recs[i].raw_len;
      if (len) memcpy(raw.get() + H.recs[i].raw_off, A->emails[i] + H.parsed[i].body_offset, len);
      memset(raw.get() + H.recs[i].raw_off + len, 0, (size_t)((16 - (len & 15)) & 15));
    });
    DevBufs D;          // the buffers of this call; the ones of the batch are taken out of it when the caller keeps them
    void* d_raw = D.get(total);
    if (d_raw && total && hipMemcpy(d_raw, raw.get(), total, hipMemcpyHostToDevice) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    raw.reset();
    void* d_recs = D.up(H.recs);
    std::vector<zkwg_dkim_key> keys(A->keys, A->keys + A->key_first[n]);
    void* d_keys = D.up(keys);
    void *d_fits = D.get(4 * n), *d_bd = D.get(32 * n), *d_hd = D.get(32 * n), *d_status = D.get(4 * n), *d_idx = D.get(4 * n);
    void* d_headers = D.up(H.headers);
    void* d_hlen = D.up(H.header_len);
    void* d_bh64 = D.up(H.bh64);
    void* d_sigs = D.up(H.sigs);
    void *d_bodies = D.get(n * bs), *d_blen = D.get(4 * n), *d_pk = D.get(256 * n);
    if (D.oom) return ZKWG_RC_OOM;
    // rows keep what the caller has there beyond each body's length: his buffer goes up first
    if ((want_bodies ? hipMemcpyAsync(d_bodies, A->bodies, n * bs, hipMemcpyHostToDevice, st) : hipMemsetAsync(d_bodies, 0, n * bs, st)) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return ZKWG_RC_HIP_ERROR;
    if (A->seconds) { A->seconds[1] = now() - t; t = now(); }
    ZkStageClock clock(st, A->seconds);
    zk_dkim_body_launch(d_recs, d_raw, d_bodies, d_blen, d_fits, bs, (u32)n, st);
    if (!clock.lap(2)) return ZKWG_RC_HIP_ERROR;
    zk_dkim_hash_launch(d_recs, d_bodies, d_blen, d_fits, bs, d_headers, d_hlen, hs, d_bd, d_hd, (u32)n, st);
    if (!clock.lap(3)) return ZKWG_RC_HIP_ERROR;
    zk_dkim_verify_launch(d_recs, d_keys, d_fits, d_bd, d_hd, d_sigs, A->flags, d_status, d_idx, d_pk, (u32)n, st);
    if (hipGetLastError() != hipSuccess) return ZKWG_RC_HIP_ERROR;
    if (!clock.lap(4)) return ZKWG_RC_HIP_ERROR;
    t = now();                               // (the kernels were timed by the stage clock: the download starts here)
    std::vector<int32_t> idx(n);
    bool ok = hipMemcpyAsync(A->status, d_status, 4 * n, hipMemcpyDeviceToHost, st) == hipSuccess &&
              hipMemcpyAsync(idx.data(), d_idx, 4 * n, hipMemcpyDeviceToHost, st) == hipSuccess;
    if (ok && want_bodies) ok = hipMemcpyAsync(A->bodies, d_bodies, n * bs, hipMemcpyDeviceToHost, st) == hipSuccess;
    if (ok && A->body_len) ok = hipMemcpyAsync(A->body_len, d_blen, 4 * n, hipMemcpyDeviceToHost, st) == hipSuccess;
    if (ok && A->body_digest) ok = hipMemcpyAsync(A->body_digest, d_bd, 32 * n, hipMemcpyDeviceToHost, st) == hipSuccess;
    if (ok && A->header_digest) ok = hipMemcpyAsync(A->header_digest, d_hd, 32 * n, hipMemcpyDeviceToHost, st) == hipSuccess;
    if (!ok || hipStreamSynchronize(st) != hipSuccess) return ZKWG_RC_HIP_ERROR;
    if (A->key_index) memcpy(A->key_index, idx.data(), 4 * n);
    if (A->seconds) A->seconds[5] = now() - t;
    if (A->device_batch) {
      zkwg_dkim_batch& B = *A->device_batch;
      memset(&B, 0, sizeof B);
      B.headers = (const uint8_t*)d_headers; B.header_len = (const uint32_t*)d_hlen; B.bodies = (const uint8_t*)d_bodies; B.body_len = (const uint32_t*)d_blen;
      B.body_hash_b64 = (const uint8_t*)d_bh64; B.pubkey_be = (const uint8_t*)d_pk; B.signature_be = (const uint8_t*)d_sigs;
      B.header_stride = hs; B.body_stride = bs;
      for (void*& q : D.p)
        if (q == d_headers || q == d_hlen || q == d_bodies || q == d_blen || q == d_bh64 || q == d_pk || q == d_sigs) q = nullptr;
    }
    return ZKWG_RC_OK;
  } catch (const std::bad_alloc&) {
    return ZKWG_RC_OOM;
  }
}

}
#endif
