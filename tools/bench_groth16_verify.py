#!/usr/bin/env python3
"""Times batched groth16 verification (zkwg.verify.verify_batch -> zkwg_groth16_verify_batch; Miller loops, subgroup flags, scalings and the
product tree on the device, three Miller loops and one final exponentiation per check on the host).

Fabricated valid proofs of a toy key with 3 public inputs (the trapdoor is drawn here; points by zkwg.prover.fixed_base), at n = 4,096 and
n = 256 -- and at n = 32,768, the first size at which every SIMD of the device holds a wavefront of zk_pair_miller (32 pairs a wavefront,
one wavefront a SIMD) --: one warm-up call, then --reps timed calls; medians, every run listed.  Recorded per n: total seconds and proofs/s, the six stage
times of zkwg_groth16_verify_stats, ns per pair of the Miller + subgroup stage.  Also: n = 4,096 with exactly ONE bad proof (what a
bisection costs), the host path (device = -1) at n = 64 as time per proof, and the parent's host pairing in the same run
(zkwg_pairing_check: the difference between 17 pairs and 1 pair, over 16 = one Miller loop and one subgroup test on the host).

PREDICTED: Fq2 products per pair (csrc/zkwg_pair_core.h: 5,748.5 with the subgroup flag) / 848 x 16.56 ns -- the subgroup test's product
count and its measured cost per point.  CONDITIONS, against the host in the same run: the device's Miller stage per pair
at n = 4,096 below the host's per pair, and whole-call proofs/s at n = 4,096 above the host path's.  The verdicts are CHECKED; exits
non-zero on a wrong one.  Prints one JSON line.

    python tools/bench_groth16_verify.py [--reps 5] > profiles/r13/r13_a_bench_groth16_verify.json
"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zk-email-verify_amd", "py"))

PRODUCTS_PER_PAIR = 64 * (13 + 23.5 + 19.5) + (36 + 2) * (15 + 19.5) + 2.5 + 3 + 848
PREDICTED_NS_PER_PAIR = PRODUCTS_PER_PAIR / 848 * 16.56


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, nargs="*", default=[4096, 256, 32768])
    args = ap.parse_args(argv)
    from zkwg import _lib, prover, verify
    from zkwg.zkey import Q, R
    lib = _lib.load()
    rng = random.Random(1330)
    n_public, n_max = 3, max(args.n + [64])
    alpha, beta, gamma, delta = (rng.randrange(2, R) for _ in range(4))
    ic = [rng.randrange(1, R) for _ in range(n_public + 1)]
    publics = [[rng.randrange(R) for _ in range(n_public)] for _ in range(n_max)]
    logs, dinv = [], pow(delta, R - 2, R)
    for x in publics:
        a, b = rng.randrange(1, R), rng.randrange(1, R)
        vkx = (ic[0] + sum(v * k for v, k in zip(x, ic[1:]))) % R
        logs.append((a, b, (a * b - alpha * beta - vkx * gamma) % R * dinv % R))
    pts = lambda group, ks: bytes(prover.fixed_base(0, group, ks).cpu().numpy())
    rinv = pow(1 << 256, -1, Q)
    std = lambda raw: [int.from_bytes(raw[o:o + 32], "little") * rinv % Q for o in range(0, len(raw), 32)]
    k1, k2 = std(pts(1, [alpha] + ic)), std(pts(2, [beta, gamma, delta]))
    g1j = lambda v: [str(v[0]), str(v[1]), "1"]
    g2j = lambda v: [[str(v[0]), str(v[1])], [str(v[2]), str(v[3])], ["1", "0"]]
    vkey = {"protocol": "groth16", "curve": "bn128", "nPublic": n_public, "vk_alpha_1": g1j(k1[0:2]), "vk_beta_2": g2j(k2[0:4]), "vk_gamma_2": g2j(k2[4:8]),
            "vk_delta_2": g2j(k2[8:12]), "IC": [g1j(k1[2 + 2 * i:4 + 2 * i]) for i in range(n_public + 1)]}
    pa, pb, pc = pts(1, [l[0] for l in logs]), pts(2, [l[1] for l in logs]), pts(1, [l[2] for l in logs])
    pc_bad = pts(1, [(l[2] + 1) % R for l in logs])
    to_std = lambda raw: b"".join(v.to_bytes(32, "little") for v in std(raw))
    proofs = [to_std(pa[64 * i:64 * i + 64] + pb[128 * i:128 * i + 128] + pc[64 * i:64 * i + 64]) for i in range(n_max)]
    ok = True

    def timed(n, device, bad=None, reps=args.reps):
        nonlocal ok
        batch = list(proofs[:n])
        if bad is not None:
            batch[bad] = to_std(pa[64 * bad:64 * bad + 64] + pb[128 * bad:128 * bad + 128] + pc_bad[64 * bad:64 * bad + 64])
        runs = []
        for rep in range(reps + 1):                                # (the first call warms up)
            t0 = time.time()
            got = verify.verify_batch(vkey, publics[:n], batch, device=device)
            dt = time.time() - t0
            ok &= got == [i != bad for i in range(n)]
            if rep:
                runs.append((dt, verify.stats()))
        med = statistics.median(r[0] for r in runs)
        sec, cnt = min(runs, key=lambda r: abs(r[0] - med))[1]
        return {"n": n, "device": device, "bad_proofs": 0 if bad is None else 1, "seconds": round(med, 5), "proofs_per_s": round(n / med, 1),
                "stage_seconds": dict(zip(("host_checks_upload", "scalings", "miller_subgroup", "product_download", "batch_check_host", "bisection"), (round(s, 6) for s in sec))),
                "counts": dict(zip(("pairs", "final_exponentiations", "excluded", "found_bad"), cnt)),
                "miller_subgroup_ns_per_pair": round(sec[2] / n * 1e9, 1), "all_runs_seconds": [round(r[0], 5) for r in runs]}

    # the parent's host pairing: 17 pairs against 1 pair (the final exponentiation and the call's overhead cancel)
    g1m, g2m = pa[:64 * 17], pb[:128 * 17]
    one, host_runs = C.c_int(), {1: [], 17: []}
    for rep in range(args.reps + 1):
        for k in (1, 17):
            t0 = time.time()
            assert lib.zkwg_pairing_check(g1m, g2m, k, C.byref(one)) == 0
            if rep:
                host_runs[k].append(time.time() - t0)
    host_pair_s = (statistics.median(host_runs[17]) - statistics.median(host_runs[1])) / 16
    device = [timed(n, 0) for n in args.n]
    n_cond = 4096 if 4096 in args.n else max(args.n)               # the size the conditions are stated for
    one_bad = timed(n_cond, 0, bad=n_cond // 3)
    host = timed(64, -1, reps=max(1, min(args.reps, 3)))
    big = device[args.n.index(n_cond)]
    out = {"n_public": n_public, "device": device, "one_bad_proof": one_bad, "host_path": dict(host, ms_per_proof=round(host["seconds"] / 64 * 1e3, 3)),
           "host_miller_and_subgroup_ms_per_pair": round(host_pair_s * 1e3, 3), "host_pairing_all_runs_s": {str(k): [round(t, 5) for t in v] for k, v in host_runs.items()},
           "fq2_products_per_pair": PRODUCTS_PER_PAIR, "predicted_ns_per_pair": round(PREDICTED_NS_PER_PAIR, 1), "measured_ns_per_pair": big["miller_subgroup_ns_per_pair"], "conditions_at_n": n_cond,
           "measured_over_predicted": round(big["miller_subgroup_ns_per_pair"] / PREDICTED_NS_PER_PAIR, 2),
           "condition_miller_stage_below_host": bool(big["miller_subgroup_ns_per_pair"] < host_pair_s * 1e9),
           "condition_proofs_per_s_above_host": bool(big["proofs_per_s"] > host["proofs_per_s"]),
           "verdicts_right": bool(ok), "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "runtime default")}
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
