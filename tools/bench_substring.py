#!/usr/bin/env python3
"""Times the substring mains: CountSubstringOccurrences(1024, 128) and RevealSubstring(256, 16, 1), the reference's own
test mains, at a batch of --n emails with the witnesses resident on the device.  Every email is a random text with one planted
occurrence of what is searched for, so every status is 0 (CHECKED; exits non-zero otherwise).  One warm-up, then --reps timed runs of
prepare + expand each; medians, every run listed.  Reported per main: witnesses/s from the wall time of prepare + expand, the
milliseconds of zk_substr and of the expansion (zk_expand3_subm) from the handle's events, the expansion's 32 W n / t in TB/s, that rate
as a fraction of the headline zk_expand rate when --headline names the file bench.py's JSON line of the same session was written to,
and the share of slots that leave as reference codes (negative differences, inverses: values that do not fit 31 bits), counted on the
first witness.  No threshold is gated.  Prints one JSON line.

    python tools/bench_substring.py [--n 4096] [--reps 5] [--headline bench.json] > profiles/r17/r17_bench_substring.json
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zk-email-verify_amd", "py"))


def inputs(kind_reveal, L, S, i):
    r = random.Random(1000003 * i + L)
    n = r.randrange(S // 2, S + 1)
    text = [r.randrange(1, 200) for _ in range(L)]
    a = r.randrange(0, L - n + 1)
    needle = [200 + r.randrange(56) for _ in range(n)]        # bytes no other position holds: exactly one occurrence
    text[a:a + n] = needle
    if kind_reveal:
        return {"in": text, "substringStartIndex": a, "substringLength": n}
    return {"in": text, "substring": needle + [0] * (S - n)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--headline", help="file holding bench.py's JSON result line of the same session (roofline.achieved, GB/s)")
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    import zkwg
    headline = None
    if a.headline:
        for line in open(a.headline):
            if line.startswith("{") and '"roofline"' in line:
                headline = json.loads(line)["roofline"]["achieved"] / 1e3      # TB/s
    dev = torch.device("cuda", a.device)
    out = {"tool": "bench_substring", "n": a.n, "reps": a.reps, "headline_zk_expand_TBps": headline, "mains": []}
    ok = True
    for name, kind, L, S, u in (("CountSubstringOccurrences(1024,128)", zkwg.MAIN_COUNT_SUBSTRING, 1024, 128, 0),
                                ("RevealSubstring(256,16,1)", zkwg.MAIN_REVEAL_SUBSTRING, 256, 16, 1)):
        c = zkwg.Circuit(kind, max_header=L, max_body=S, n=u, k=0, device=a.device)
        recs = b"".join(c.pack(inputs(kind == zkwg.MAIN_REVEAL_SUBSTRING, L, S, i)) for i in range(a.n))
        d_in = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to(dev)
        d_out = torch.empty(a.n * c.witness_bytes, dtype=torch.uint8, device=dev)
        d_status = torch.zeros(a.n, dtype=torch.int32, device=dev)
        d_scr = torch.empty(c.scratch_bytes(a.n, montgomery=False), dtype=torch.uint8, device=dev)
        c.set_timing(True)
        runs = []
        for rep in range(a.reps + 1):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            c.prepare_device(d_in, a.n, d_status, d_scr)
            c.expand_device(d_in, a.n, d_scr, 0, a.n, d_out)
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            km = c.kernel_times_ms()
            if rep:                                   # (the first run is the warm-up)
                runs.append({"seconds": dt, "zk_substr_ms": km["zk_rsa"][0], "expand_ms": km["zk_expand"][0]})
        ok = ok and d_status.cpu().tolist() == [0] * a.n
        w0 = np.frombuffer(d_out[:c.witness_bytes].cpu().numpy().tobytes(), dtype="<u4").reshape(c.W, 8)
        ref_share = float(np.count_nonzero((w0[:, 1:].any(axis=1)) | (w0[:, 0] >> 31 != 0))) / c.W
        med = statistics.median(r["seconds"] for r in runs)
        ex = statistics.median(r["expand_ms"] for r in runs)
        tbps = 32.0 * c.W * a.n / (ex * 1e-3) / 1e12
        out["mains"].append({"main": name, "witness_len": c.W, "witness_GB": 32.0 * c.W * a.n / 1e9, "median_seconds": med,
                             "witnesses_per_s": a.n / med, "zk_substr_ms": statistics.median(r["zk_substr_ms"] for r in runs),
                             "expand_ms": ex, "expand_TBps": tbps, "fraction_of_headline": tbps / headline if headline else None,
                             "reference_code_share": ref_share, "runs": runs})
        del d_in, d_out, d_scr, c
        torch.cuda.empty_cache()
    out["statuses_ok"] = ok
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
