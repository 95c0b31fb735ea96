#!/usr/bin/env python3
"""Times the CleanEmailAddress main: CleanEmailAddress(32), the reference's own test main, and CleanEmailAddress(320), the
longest legal address, at a batch of --n emails with the witnesses resident on the device.  Every email is a seeded address with
periods and an alias, `decoded` by zkwg.inputs.clean_email_address, so every isValid is 1 and every status 0 (CHECKED; exits non-zero
otherwise).  One warm-up, then --reps timed runs of prepare + expand each; medians, every run listed.  Reported per shape: witnesses/s
from the wall time of prepare + expand, the milliseconds of zk_cea_chunks, zk_cea_tail and the expansion (zk_expand3_cea) from the
handle's events, the expansion's 32 W n / t in TB/s, that rate as a fraction of the headline zk_expand rate when --headline names the
file bench.py's JSON line of the same session was written to, and the nanoseconds per Poseidon(16) of zk_cea_chunks.

The same evaluator runs in zk_rslb_chunks: an EmailVerifier(1024, 1536, removeSoftLineBreaks) handle hashes --rslb-n emails' 192 chunks
each (only that kernel is launched, on records of random bytes, every chunk hashed) in the same call.  A launch of w wavefronts fills the
chip's 1,024 one-per-SIMD slots ceil(w / 1024) times, so beside the nanoseconds per hash both kernels report the milliseconds per such
round -- the evaluator's latency, which is what a launch of fewer than 1,024 wavefronts costs whatever its size.
No threshold is gated.  Prints one JSON line.

    python tools/bench_clean_address.py [--n 4096] [--reps 5] [--headline bench.json] > profiles/r21/r21_b_bench_clean_address.json
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

SLOTS = 1024      # 256 CUs x 4 SIMDs, one wavefront each (the evaluator's state takes 39 KB of a CU's 160 KB of LDS)


def address(L, i):
    """a seeded address of up to L bytes: periods in the local part, an alias, a domain"""
    r = random.Random(1000003 * i + L)
    word = lambda n: "".join(r.choice("abcdefghijklmnopqrstuvwxyz0123456789") for _ in range(n))
    domain = word(r.randrange(3, 9)) + "." + r.choice(("com", "org", "net"))
    room = L - len(domain) - 1
    alias = "+" + word(r.randrange(1, max(2, room // 4)))
    local = ".".join(word(r.randrange(1, 6)) for _ in range(max(1, (room - len(alias)) // 6)))
    return (local + alias)[:room] + "@" + domain


def kernel_ms(c, name):
    """the last launch's milliseconds of one kernel of the handle (kernel_times_ms asks for all of them, the expansion included)"""
    import ctypes as C
    i = next(i for i in range(c.lib.zkwg_num_kernels(c.h)) if c.lib.zkwg_kernel_name(c.h, i).decode() == name)
    ms = C.c_float()
    if c.lib.zkwg_last_kernel_ms(c.h, i, C.byref(ms)) != 0:
        raise RuntimeError("no timing of " + name)
    return ms.value


def rounds(wavefronts):
    return (wavefronts + SLOTS - 1) // SLOTS


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--rslb-n", type=int, default=1024, help="emails of the removeSoftLineBreaks comparison run")
    ap.add_argument("--headline", help="file holding bench.py's JSON result line of the same session (roofline.achieved, GB/s)")
    a = ap.parse_args(argv)
    import torch
    import zkwg
    from zkwg import inputs as zi
    headline = None
    if a.headline:
        for line in open(a.headline):
            if line.startswith("{") and '"roofline"' in line:
                headline = json.loads(line)["roofline"]["achieved"] / 1e3      # TB/s
    dev = torch.device("cuda", a.device)
    out = {"tool": "bench_clean_address", "n": a.n, "reps": a.reps, "headline_zk_expand_TBps": headline, "mains": []}
    ok = True
    for L in (32, 320):
        c = zkwg.Circuit(zkwg.MAIN_CLEAN_EMAIL_ADDRESS, max_header=L, max_body=L, n=0, k=0, device=a.device)
        recs = b"".join(c.pack(zi.generate_clean_email_address_inputs(address(L, i), L)) for i in range(a.n))
        d_in = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to(dev)
        d_out = torch.empty(a.n * c.witness_bytes, dtype=torch.uint8, device=dev)
        d_status = torch.ones(a.n, dtype=torch.int32, device=dev)
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
                runs.append({"seconds": dt, "zk_cea_chunks_ms": km["zk_cea_chunks"][0], "zk_cea_tail_ms": km["zk_cea_tail"][0],
                             "expand_ms": km["zk_expand"][0]})
        valid = d_out.view(a.n, c.witness_bytes)[:, 32:64].cpu()             # slot 1 = main.isValid
        ok = ok and d_status.cpu().tolist() == [0] * a.n and bool((valid[:, 0] == 1).all()) and int(valid[:, 1:].max()) == 0
        med = statistics.median(r["seconds"] for r in runs)
        ch, tl, ex = (statistics.median(r[k] for r in runs) for k in ("zk_cea_chunks_ms", "zk_cea_tail_ms", "expand_ms"))
        tbps = 32.0 * c.W * a.n / (ex * 1e-3) / 1e12
        hashes = a.n * (L // 8)
        out["mains"].append({"main": f"CleanEmailAddress({L})", "witness_len": c.W, "witness_GB": 32.0 * c.W * a.n / 1e9,
                             "median_seconds": med, "witnesses_per_s": a.n / med, "zk_cea_chunks_ms": ch, "zk_cea_tail_ms": tl,
                             "expand_ms": ex, "expand_TBps": tbps, "fraction_of_headline": tbps / headline if headline else None,
                             "poseidon16": hashes, "ns_per_poseidon16": ch * 1e6 / hashes, "chunk_wavefronts": (hashes + 63) // 64,
                             "chunks_ms_per_round": ch / rounds((hashes + 63) // 64), "runs": runs})
        del d_in, d_out, d_scr, c
        torch.cuda.empty_cache()
    # zk_rslb_chunks alone, every chunk hashed (no constant-chunk split), on random bytes
    os.environ["ZKWG_RSLB_CONST_CHUNKS"] = "0"
    c = zkwg.Circuit(zkwg.MAIN_EMAIL_VERIFIER, max_header=1024, max_body=1536, remove_soft_line_breaks=1, device=a.device)
    del os.environ["ZKWG_RSLB_CONST_CHUNKS"]
    n = a.rslb_n
    g = torch.Generator(device="cpu").manual_seed(7)
    d_in = torch.randint(1, 256, (n * c.in_stride,), dtype=torch.uint8, generator=g).to(dev)
    d_status = torch.zeros(n, dtype=torch.int32, device=dev)
    d_scr = torch.empty(c.scratch_bytes(n, montgomery=False), dtype=torch.uint8, device=dev)
    c.set_prepare_mask(64)                                # zk_rslb_chunks only
    c.set_timing(True)
    ms = []
    for rep in range(a.reps + 1):
        c.prepare_device(d_in, n, d_status, d_scr)
        torch.cuda.synchronize(dev)
        if rep:
            ms.append(kernel_ms(c, "zk_rslb_chunks"))
    t = statistics.median(ms)
    hashes = n * 192
    out["zk_rslb_chunks"] = {"emails": n, "poseidon16": hashes, "ms": t, "ns_per_poseidon16": t * 1e6 / hashes,
                             "chunk_wavefronts": hashes // 64, "ms_per_round": t / rounds(hashes // 64), "runs_ms": ms}
    out["statuses_ok"] = ok
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
