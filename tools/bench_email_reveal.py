#!/usr/bin/env python3
"""Times the application main EmailReveal at the headline sizes: EmailReveal(1024, 1536, 121, 17, 0, header, S = 32,
uniq = 1, nullifier = 1) and the body variant with S = 64, beside the plain EmailVerifier(1024, 1536) measured THE SAME WAY in the same
session -- a batch of --n synthetic emails resident on the device, one prepare of the whole batch, then its expansion tile by tile
into a two-tile ring in HBM (no overlap of the two phases: this is not bench.py's pipeline, the plain main's figure here is the
yardstick of this tool only).  Every email reveals its message id (header) or 64 bytes of its body, so every status is 0 (CHECKED;
exits non-zero otherwise).  One warm-up, then --reps timed runs; medians, every run listed.  Reported per main: witnesses/s from the
wall time of prepare + expansion, the expansion's 32 W n / t in TB/s from the wall time of that phase, and from ONE more run with kernel timing
on -- which runs zk_substr and zk_app_tail in line instead of beside EmailVerifier's roles -- the milliseconds of every prepare kernel.
No threshold is gated.  Prints one JSON line.

    python tools/bench_email_reveal.py [--n 4096] [--tile 512] [--reps 5] > profiles/r19/r19_b_bench_email_reveal.json
"""
import argparse
import json
import os
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zk-email-verify_amd", "py"))
DISTINCT = 64


def records(zkwg, c, n):
    """n resident records: DISTINCT synthetic emails (1 KB bodies) repeated, with the indices of the revealed bytes"""
    from zkwg import synth
    recs, fields = synth.packed_batch(c, seed=19, n=DISTINCT, body_len=1024)
    app = getattr(c, "app", None)
    if app is not None:
        out = bytearray(recs)
        off = c.lib.zkwg_input_offset(c.h, 13)
        N = c.cfg.max_header
        for e in range(DISTINCT):
            pair = (10, 64) if app.reveal_from_body else (bytes(fields["header"][e * N:(e + 1) * N]).index(b"message-id:"), app.max_substring)
            struct.pack_into("<II", out, e * c.in_stride + off, *pair)
        recs = bytes(out)
    return (recs * ((n + DISTINCT - 1) // DISTINCT))[:n * c.in_stride]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    import torch
    import zkwg
    dev = torch.device("cuda", a.device)
    assert a.n % a.tile == 0
    out = {"tool": "bench_email_reveal", "n": a.n, "tile": a.tile, "reps": a.reps, "mains": []}
    ok = True
    E = zkwg.MAIN_EMAIL_REVEAL
    for name, kw in (("EmailVerifier(1024,1536)", dict(main_kind=zkwg.MAIN_EMAIL_VERIFIER)),
                     ("EmailReveal(1024,1536,header,S=32,uniq=1,nullifier=1)", dict(main_kind=E, reveal_from_body=0, max_substring=32, check_uniqueness=1, with_nullifier=1)),
                     ("EmailReveal(1024,1536,body,S=64,uniq=1,nullifier=1)", dict(main_kind=E, reveal_from_body=1, max_substring=64, check_uniqueness=1, with_nullifier=1))):
        c = zkwg.Circuit(max_header=1024, max_body=1536, device=a.device, **kw)
        d_in = torch.frombuffer(bytearray(records(zkwg, c, a.n)), dtype=torch.uint8).to(dev)
        ring = [torch.empty(a.tile * c.witness_bytes, dtype=torch.uint8, device=dev) for _ in range(2)]
        d_status = torch.zeros(a.n, dtype=torch.int32, device=dev)
        d_scr = torch.empty(c.scratch_bytes(a.n, montgomery=False), dtype=torch.uint8, device=dev)
        runs, kernels = [], None
        for rep in range(a.reps + 2):
            timed = rep == a.reps + 1                 # the last run: per-kernel times (the two extra roles then run in line)
            c.set_timing(timed)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            c.prepare_device(d_in, a.n, d_status, d_scr)
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            for t in range(a.n // a.tile):            # one stream: a tile of the ring is rewritten only after its previous expansion
                c.expand_device(d_in, a.n, d_scr, t * a.tile, a.tile, ring[t & 1])
            torch.cuda.synchronize(dev)
            t2 = time.perf_counter()
            if timed:
                kernels = {k: round(v[0], 3) for k, v in c.kernel_times_ms().items() if k != "zk_expand"}
            elif rep:                                 # (the first run is the warm-up)
                runs.append({"seconds": t2 - t0, "prepare_seconds": t1 - t0, "expand_seconds": t2 - t1})
        ok = ok and d_status.cpu().tolist() == [0] * a.n
        med = statistics.median(r["seconds"] for r in runs)
        ex = statistics.median(r["expand_seconds"] for r in runs)
        out["mains"].append({"main": name, "witness_len": c.W, "witness_GB": 32.0 * c.W * a.n / 1e9, "median_seconds": med,
                             "witnesses_per_s": a.n / med, "prepare_ms": 1e3 * statistics.median(r["prepare_seconds"] for r in runs),
                             "expand_ms": 1e3 * ex, "expand_TBps": 32.0 * c.W * a.n / ex / 1e12, "prepare_kernels_ms_in_line": kernels, "runs": runs})
        del d_in, ring, d_scr, c
        torch.cuda.empty_cache()
    base = out["mains"][0]
    for m in out["mains"][1:]:
        m["rate_vs_plain"] = m["witnesses_per_s"] / base["witnesses_per_s"]
        m["slots_vs_plain"] = m["witness_len"] / base["witness_len"]
    out["statuses_ok"] = ok
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
