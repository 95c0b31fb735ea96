#!/usr/bin/env python3
"""Times EmailReveal's input generation from needles against the call it replaces, on one handle
EmailReveal(576, 192, body, S = 12, uniq = 1): --n synthetic results RESIDENT on the device (DISTINCT of them, repeated), bodies of 0.9 KB
and of 62 KB (the sizes of DESIGN.md 24.6), one marker at the same offset in every body -- 9 bytes, 100 bytes before the body's end, so
that the SHA prefix must be cut -- and

  (a) zkwg_generate_inputs_device with the marker as the shared selector, then the strided copy of the (start, length) pairs: the call
      as it was before the needles;
  (b) zkwg_generate_reveal_inputs_device with the marker as every email's needle;
  (c) (b) with a needle that is in no body: the kernel searches every body to its end, computes no midstate and counts nothing, so its
      time is an UPPER BOUND of what the search (and everything that is not midstate or count) costs in (b).

(a) and (b) must give the same records (CHECKED; exits non-zero otherwise), every status 0; (c)'s are all 5.  One warm-up, then --reps
runs of each, interleaved, timed with events on the stream around the calls; medians, every run listed.  No threshold is gated here;
DESIGN.md 28 says what is required of the figures.  Prints one JSON line.

    python tools/bench_locate.py [--n 4096] [--reps 5] > profiles/r22/r22_bench_locate.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zk-email-verify_amd", "py"))
DISTINCT = 16
MARK = b"~MARK~ER~"
SHAPE = dict(main_kind=6, max_header=576, max_body=192, ignore_body_hash_check=0, reveal_from_body=1, max_substring=12,
             check_uniqueness=1, with_nullifier=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    import zkwg
    from zkwg import _lib, synth
    dev = torch.device("cuda", 0)
    c = zkwg.Circuit(device=0, **SHAPE)
    n = args.n
    base = [synth.synthetic_dkim_result(22, i, body_len=64) for i in range(DISTINCT)]
    rep = (n + DISTINCT - 1) // DISTINCT
    up = lambda rows, width: torch.from_numpy(np.stack([np.frombuffer(r.ljust(width, b"\0"), dtype=np.uint8) for r in rows] * rep)[:n].copy()).to(dev)
    hs = max(len(d["headers"]) for d in base)
    t_hdr = up([d["headers"] for d in base], hs)
    t_hl = torch.tensor(([len(d["headers"]) for d in base] * rep)[:n], dtype=torch.int32, device=dev)
    t_bh = up([d["bodyHash"].encode() for d in base], 44)
    t_pk = up([int(d["publicKey"]).to_bytes(256, "big") for d in base], 256)
    t_sg = up([int(d["signature"]).to_bytes(256, "big") for d in base], 256)
    t_mark = torch.frombuffer(bytearray(MARK), dtype=torch.uint8).to(dev)
    absent = b"~ABSENT~~"
    first = np.arange(n + 1, dtype=np.int32) * len(MARK)
    t_first = torch.from_numpy(first).to(dev)
    t_needles = torch.frombuffer(bytearray(MARK * n), dtype=torch.uint8).to(dev)
    t_absent = torch.frombuffer(bytearray(absent * n), dtype=torch.uint8).to(dev)
    off = c.lib.zkwg_input_offset(c.h, _lib.IN_SUBSTRING_START)
    out = {"tool": "bench_locate", "n": n, "reps": args.reps, "shape": SHAPE, "marker_bytes": len(MARK), "cases": []}
    ok = True
    for body_len in (900, 62 * 1024):
        rng = np.random.default_rng(body_len)
        bodies = rng.integers(97, 123, size=(n, body_len), dtype=np.uint8)          # lower-case letters: the marker's '~' is in none
        at = body_len - 100
        bodies[:, at:at + len(MARK)] = np.frombuffer(MARK, dtype=np.uint8)
        t_body = torch.from_numpy(bodies).to(dev)
        t_bl = torch.full((n,), body_len, dtype=torch.int32, device=dev)
        cut = (at // 64) * 64
        pairs = torch.tensor([at - cut, len(MARK)], dtype=torch.int32).view(torch.uint8).repeat(n, 1).to(dev)

        def batch(selector):
            return _lib.DkimBatch(t_hdr.data_ptr(), t_hl.data_ptr(), t_body.data_ptr(), t_bl.data_ptr(), t_bh.data_ptr(), t_pk.data_ptr(),
                                  t_sg.data_ptr(), t_mark.data_ptr() if selector else None, hs, body_len, len(MARK) if selector else 0)
        b_sel, b_plain = batch(True), batch(False)
        recs = {k: torch.empty((n, c.in_stride), dtype=torch.uint8, device=dev) for k in "abc"}
        st = {k: torch.zeros(n, dtype=torch.int32, device=dev) for k in "abc"}
        q_mark, q_absent = _lib.Needles(t_needles.data_ptr(), t_first.data_ptr()), _lib.Needles(t_absent.data_ptr(), t_first.data_ptr())

        def run(k):
            if k == "a":
                zkwg._check(c.lib.zkwg_generate_inputs_device(c.h, C.byref(b_sel), n, recs[k].data_ptr(), st[k].data_ptr(), None))
                recs[k][:, off:off + 8].copy_(pairs)
            else:
                zkwg._check(c.lib.zkwg_generate_reveal_inputs_device(c.h, C.byref(b_plain), C.byref(q_mark if k == "b" else q_absent), n,
                                                                     recs[k].data_ptr(), st[k].data_ptr(), None))

        def timed(k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(k)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        for k in "abc":
            run(k)                                                                   # warm-up
        torch.cuda.synchronize()
        ms = {k: [] for k in "abc"}
        for _ in range(args.reps):
            for k in "abc":
                ms[k].append(round(timed(k), 4))
        same = bool(torch.equal(recs["a"], recs["b"]))
        status_ok = st["a"].cpu().tolist() == [0] * n and st["b"].cpu().tolist() == [0] * n and st["c"].cpu().tolist() == [5] * n
        ok = ok and same and status_ok
        med = {k: statistics.median(v) for k, v in ms.items()}
        out["cases"].append({
            "body_bytes": body_len, "marker_at": at, "cut": cut, "records_equal": same, "statuses_as_expected": status_ok,
            "a_selector_ms": ms["a"], "b_needle_ms": ms["b"], "c_absent_needle_ms": ms["c"],
            "a_median_ms": med["a"], "b_median_ms": med["b"], "c_median_ms": med["c"],
            "a_spread_ms": round(max(ms["a"]) - min(ms["a"]), 4), "b_minus_a_ms": round(med["b"] - med["a"], 4),
            "search_share_of_b_upper_bound": round(med["c"] / med["b"], 4),
            "b_emails_per_s": round(n / med["b"] * 1e3, 1), "c_body_GBps": round(n * body_len / med["c"] / 1e6, 2)})
    out["ok"] = ok
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
