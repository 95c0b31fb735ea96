#!/usr/bin/env python3
"""Times per-proof groth16 verification (zkwg.verify.verify_each -> zkwg_groth16_verify_each: the scalings of the public inputs, three Miller
loops and one final exponentiation per proof on the device) AND the batch verifier (verify_batch) on the same inputs in the same run.

Fabricated proofs of a toy key with 3 public inputs (the trapdoor is drawn here; points by zkwg.prover.fixed_base), the method of
tools/bench_groth16_verify.py: one warm-up call, then --reps timed calls; medians, every run listed, the verdicts CHECKED (exits non-zero on
a wrong one).  At n = 256, 4,096 and 32,768, with every proof good, with exactly one bad proof, and with 10 % bad proofs (every tenth).
verify_batch with 10 % bad is MEASURED only at n = 256 (at most 511 checks); at the larger sizes the record holds the bound on the number
of checks, min(2 n - 1, 1 + 2 k ceil(log2 n)), times the seconds per check measured at n = 256, labelled "extrapolated".

CONDITION: verify_each beats verify_batch with one bad proof among 4,096 (plain "less than").  Recorded, not gated: the ratio verify_each /
verify_batch with every proof good at the three sizes, and the final-exponentiation stage in ns per proof at the largest n against the
PREDICTION from the operation count (csrc/zkwg_fexp_core.h: 6,213 Fq2 products per proof) / 848 x 16.56 ns, the rate of DESIGN 23.8.
Prints one JSON line.

    python tools/bench_groth16_verify_each.py [--reps 5] > profiles/r14/r14_b_bench_groth16_verify_each.json
"""
import argparse
import json
import math
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zk-email-verify_amd", "py"))

PRODUCTS_PER_PROOF = 89 + 455.5 + 3 * 1653.5 + 708          # fold, easy part, three powers by u, hard part (csrc/zkwg_fexp_core.h)
PREDICTED_NS_PER_PROOF = PRODUCTS_PER_PROOF / 848 * 16.56
EACH_STAGES = ("host_checks_eab_upload", "vkx", "miller_subgroup", "final_exponentiation", "download_compare", "unused")
BATCH_STAGES = ("host_checks_upload", "scalings", "miller_subgroup", "product_download", "batch_check_host", "bisection")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, nargs="*", default=[256, 4096, 32768])
    ap.add_argument("--batch-ten-percent-up-to", type=int, default=256, help="the largest n at which verify_batch with 10 %% bad proofs is measured")
    args = ap.parse_args(argv)
    from zkwg import prover, verify
    from zkwg.zkey import Q, R
    rng = random.Random(1430)
    n_public, n_max = 3, max(args.n)
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
    good = [to_std(pa[64 * i:64 * i + 64] + pb[128 * i:128 * i + 128] + pc[64 * i:64 * i + 64]) for i in range(n_max)]
    wrong = lambda i: to_std(pa[64 * i:64 * i + 64] + pb[128 * i:128 * i + 128] + pc_bad[64 * i:64 * i + 64])
    ok = True

    def bad_set(n, share):
        return set() if share == "good" else {n // 3} if share == "one_bad" else set(range(5, n, 10))

    def timed(mode, n, share):
        nonlocal ok
        bad = bad_set(n, share)
        batch = [wrong(i) if i in bad else good[i] for i in range(n)]
        call, stats, names = (verify.verify_each, verify.stats_each, EACH_STAGES) if mode == "each" else (verify.verify_batch, verify.stats, BATCH_STAGES)
        runs = []
        for rep in range(args.reps + 1):                           # (the first call warms up)
            t0 = time.time()
            got = call(vkey, publics[:n], batch, device=0)
            dt = time.time() - t0
            ok &= got == [i not in bad for i in range(n)]
            if rep:
                runs.append((dt, stats()))
        med = statistics.median(r[0] for r in runs)
        sec, cnt = min(runs, key=lambda r: abs(r[0] - med))[1]
        return {"seconds": round(med, 5), "proofs_per_s": round(n / med, 1), "bad_proofs": len(bad), "stage_seconds": dict(zip(names, (round(s, 6) for s in sec))),
                "counts": list(cnt), "all_runs_seconds": [round(r[0], 5) for r in runs]}

    sizes, per_check = {}, None
    for n in sorted(args.n):
        row = {"each": {s: timed("each", n, s) for s in ("good", "one_bad", "ten_percent_bad")}, "batch": {s: timed("batch", n, s) for s in ("good", "one_bad")}}
        k = len(bad_set(n, "ten_percent_bad"))
        bound = min(2 * n - 1, 1 + 2 * k * math.ceil(math.log2(n)))
        if n <= args.batch_ten_percent_up_to:
            t = timed("batch", n, "ten_percent_bad")
            checks = t["counts"][1]
            per_check = (t["stage_seconds"]["batch_check_host"] + t["stage_seconds"]["bisection"]) / checks
            row["batch"]["ten_percent_bad"] = dict(t, checks=checks, bound_on_checks=bound, seconds_per_check=round(per_check, 6))
        elif per_check is not None:
            row["batch"]["ten_percent_bad"] = {"extrapolated": True, "bad_proofs": k, "bound_on_checks": bound, "seconds_per_check": round(per_check, 6),
                                               "seconds": round(row["batch"]["good"]["seconds"] + (bound - 1) * per_check, 3)}
        row["each_over_batch_all_good"] = round(row["each"]["good"]["seconds"] / row["batch"]["good"]["seconds"], 2)
        row["each_over_batch_one_bad"] = round(row["each"]["one_bad"]["seconds"] / row["batch"]["one_bad"]["seconds"], 3)
        row["each_counts_do_not_depend_on_the_bad_share"] = len({tuple(row["each"][s]["counts"][:2]) for s in row["each"]}) == 1
        sizes[str(n)] = row
    n_cond = 4096 if 4096 in args.n else max(args.n)
    n_big = max(args.n)
    fe_ns = sizes[str(n_big)]["each"]["good"]["stage_seconds"]["final_exponentiation"] / n_big * 1e9
    cond = sizes[str(n_cond)]
    out = {"n_public": n_public, "sizes": sizes, "conditions_at_n": n_cond,
           "condition_each_beats_batch_with_one_bad_proof": bool(cond["each"]["one_bad"]["seconds"] < cond["batch"]["one_bad"]["seconds"]),
           "each_one_bad_seconds": cond["each"]["one_bad"]["seconds"], "batch_one_bad_seconds": cond["batch"]["one_bad"]["seconds"],
           "fq2_products_per_proof_final_exponentiation": PRODUCTS_PER_PROOF, "predicted_ns_per_proof": round(PREDICTED_NS_PER_PROOF, 1),
           "measured_ns_per_proof": round(fe_ns, 1), "measured_at_n": n_big, "measured_over_predicted": round(fe_ns / PREDICTED_NS_PER_PROOF, 2),
           "verdicts_right": bool(ok), "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "runtime default")}
    print(json.dumps(out))
    return 0 if ok and out["condition_each_beats_batch_with_one_bad_proof"] else 1


if __name__ == "__main__":
    sys.exit(main())
