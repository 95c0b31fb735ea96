#!/usr/bin/env python3
"""Times `groth16 setup` on the device (zkwg.setup.new_zkey -> zkwg_zkey_new) for the headline system: the .r1cs `python -m zkwg.r1cs
--max-header 1024 --max-body 1536` exports (domain 2^21), powers of tau from a known (tau, alpha, beta) as device-resident slices
(prover.fixed_base).  Prints one JSON line: wall time split into parse + plans / upload + curve check / each of the four sums (with the
conversion to affine points and the download of the section) / the H copy + download, group operations and group operations per
second of each sum, the term and wire-degree histograms of the system, and -- for context -- the mixed-addition rate of
zk_msm_slice_sum<G1> from profiles/r06/r06_zz_prove_kernel_stats.csv.

The key is CHECKED: sampled wires, the longest included, against the discrete logarithms of their A, B1, B2 and K points, and sampled H
points (tools/bench_prove.py checks its sums the same way).

    python tools/bench_setup.py [--max-header 1024 --max-body 1536] [--samples 24] [--reps 1] [--out key.zkey]
"""
import argparse
import collections
import csv
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "zk-email-verify_amd", "py"))

H_SERIES_MIXED_ADDITIONS = 8 * 33.5e6      # level-0 slices of the H sum of a series of 8 emails at 2^21


def lagrange_at(tau, power, R):
    """L_j(tau), j < 2^power, over the domain of ffjavascript's root of unity (w_28 = 5^((r - 1) / 2^28), squared down):
    L_j(t) = (t^n - 1) x_j / (n (t - x_j)).  The toy ceremony's discrete logarithms."""
    n = 1 << power
    w = pow(5, (R - 1) >> 28, R)
    for _ in range(28 - power):
        w = w * w % R
    xs, x = [0] * n, 1
    for j in range(n):
        xs[j] = x
        x = x * w % R
    pref = [1] * (n + 1)
    for j in range(n):
        pref[j + 1] = pref[j] * ((tau - xs[j]) % R) % R
    inv = pow(pref[n], R - 2, R)
    k = (pow(tau, n, R) - 1) * pow(n, R - 2, R) % R
    out = [0] * n
    for j in range(n - 1, -1, -1):
        out[j] = k * xs[j] % R * (inv * pref[j] % R) % R
        inv = inv * ((tau - xs[j]) % R) % R
    return out


def msm_context():
    """the longest zk_msm_slice_sum<G1, level 0> call of the round-6 prover profile: the H sum's slices of a series of 8"""
    path = os.path.join(ROOT, "profiles", "r06", "r06_zz_prove_kernel_stats.csv")
    try:
        for row in csv.DictReader(open(path)):
            if row["Name"].startswith("void zk_msm_slice_sum<ZkEcG1, true>"):
                return {"kernel": "zk_msm_slice_sum<ZkEcG1, true>", "max_call_ms": round(int(row["MaxNs"]) / 1e6, 3),
                        "mixed_additions_of_that_call": H_SERIES_MIXED_ADDITIONS,
                        "mixed_additions_per_s": round(H_SERIES_MIXED_ADDITIONS / (int(row["MaxNs"]) / 1e9) / 1e9, 2), "unit": "G"}
    except OSError:
        pass
    return None


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-header", type=int, default=1024)
    ap.add_argument("--max-body", type=int, default=1536)
    ap.add_argument("--samples", type=int, default=24)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--out", help="write the key here")
    args = ap.parse_args(argv)
    import torch
    import zkwg
    from zkwg import prover, setup, zkey
    from zkwg import r1cs as zr
    R = prover.R
    N, M, n_public = args.max_header, args.max_body, 20
    t0 = time.time()
    c = zkwg.Circuit(zkwg.MAIN_EMAIL_VERIFIER, max_header=N, max_body=M, device=-1)
    cons = zr.email_verifier_constraints(c.symbols(), N, M)
    r1cs = zr.write_r1cs(c.W, cons, n_pub_out=3, n_pub_in=17, n_prv_in=N + 1 + 17 + 1 + 32 + M + 1)
    power, zkey_bytes = setup.key_shape(r1cs)
    m, n = len(cons), 1 << power
    # histograms: terms by class of coefficient, wires by degree (terms of the wire in A, B, C together)
    half = R // 2
    cls = collections.Counter()
    degree = collections.Counter()
    for row in cons:
        for mtx in range(3):
            for w, v in row[mtx].items():
                v %= R
                if not v:
                    continue
                mag = v if v <= half else R - v
                cls[("A", "B", "C")[mtx] + (" +-1" if mag == 1 else " +-2^k" if mag & (mag - 1) == 0 else f" other <= {8 * ((mag.bit_length() + 7) // 8)} bits")] += 1
                degree[w] += 1
    buckets = collections.Counter()
    for w, d in degree.items():
        buckets["1" if d == 1 else "2" if d == 2 else "3" if d == 3 else "4-8" if d <= 8 else "9-64" if d <= 64 else "65-4096" if d <= 4096 else "> 4096"] += 1
    longest = [w for w, _ in degree.most_common(3)]
    t_system = time.time() - t0
    # the toy ceremony
    t0 = time.time()
    rng = random.Random(6)
    tau, alpha, beta = (rng.randrange(2, R) for _ in range(3))
    lag, nxt = lagrange_at(tau, power, R), lagrange_at(tau, power + 1, R)
    up = lambda g, s: prover.fixed_base(0, g, s)
    down = lambda t: bytes(t.cpu().numpy())
    slices = {"power": power, "tau_g1": up(1, lag), "tau_g2": up(2, lag), "alpha_tau_g1": up(1, [x * alpha % R for x in lag]),
              "beta_tau_g1": up(1, [x * beta % R for x in lag]), "tau_g1_next": up(1, nxt),
              "alpha1": down(up(1, [alpha])), "beta1": down(up(1, [beta])), "beta2": down(up(2, [beta]))}
    torch.cuda.synchronize()
    t_ceremony = time.time() - t0
    runs = []
    for _ in range(args.reps):
        t0 = time.time()
        z = setup.new_zkey(r1cs, slices)
        st = setup.last_stats()
        st["wall_s"] = round(time.time() - t0, 3)
        runs.append(st)
    best = min(runs, key=lambda r: r["wall_s"])
    sums = {}
    for name, sec in (("a", "sum_a"), ("b1", "sum_b1"), ("b2", "sum_b2"), ("k", "sum_k")):
        o = best["ops"][name]
        s = best["seconds"][sec]
        sums[name] = {"seconds": round(s, 4), "additions": o["add"], "doublings": o["dbl"], "group_ops_per_s": round((o["add"] + o["dbl"]) / s / 1e6, 2), "unit": "M"}
    # ---- the check ----------------------------------------------------------------------------------------------------------------------
    d = zkey.read_zkey(z, coeffs=False)
    srng = random.Random(2)
    wires = sorted(set(longest + list(range(0, n_public + 2)) + [srng.randrange(c.W) for _ in range(args.samples)]))
    want = {w: [0, 0, 0] for w in wires}
    for j, row in enumerate(cons):
        for mtx in range(3):
            for w in want.keys() & row[mtx].keys():
                want[w][mtx] = (want[w][mtx] + row[mtx][w] * lag[j]) % R
    for s in range(n_public + 1):
        if s in want:
            want[s][0] = (want[s][0] + lag[m + s]) % R
    ws = list(want)
    a = down(up(1, [want[w][0] for w in ws]))
    b1 = down(up(1, [want[w][1] for w in ws]))
    b2 = down(up(2, [want[w][1] for w in ws]))
    k = down(up(1, [(beta * want[w][0] + alpha * want[w][1] + want[w][2]) % R for w in ws]))
    ok = True
    for i, w in enumerate(ws):
        ok &= d["a"][64 * w:64 * w + 64] == a[64 * i:64 * i + 64] and d["b1"][64 * w:64 * w + 64] == b1[64 * i:64 * i + 64]
        ok &= d["b2"][128 * w:128 * w + 128] == b2[128 * i:128 * i + 128]
        kp = d["ic"][64 * w:64 * w + 64] if w <= n_public else d["c"][64 * (w - n_public - 1):64 * (w - n_public)]
        ok &= kp == k[64 * i:64 * i + 64]
    hj = [0, 1, n - 1] + [srng.randrange(n) for _ in range(args.samples)]
    hp = down(up(1, [nxt[2 * j + 1] for j in hj]))
    ok &= all(d["h"][64 * j:64 * j + 64] == hp[64 * i:64 * i + 64] for i, j in enumerate(hj))
    ok &= d["alpha1"] == slices["alpha1"] and d["beta2"] == slices["beta2"] and (d["n_vars"], d["n_public"], d["domain_size"]) == (c.W, n_public, n)
    if args.out:
        open(args.out, "wb").write(z)
    out = {"circuit": f"EmailVerifier({N},{M},121,17,0,0,0,0)", "W": c.W, "constraints": m, "domain_log2": power, "zkey_bytes": len(z),
           "seconds": {k_: round(v, 4) for k_, v in best["seconds"].items()}, "wall_s": best["wall_s"], "wall_s_all_runs": [r["wall_s"] for r in runs],
           "sums": sums, "key_checked_against_discrete_logarithms": bool(ok), "wires_checked": len(ws), "longest_wires": {str(w): degree[w] for w in longest},
           "terms_by_class": dict(sorted(cls.items())), "wires_by_degree": dict(buckets), "msm_context": msm_context(),
           "system_s": round(t_system, 1), "toy_ceremony_s": round(t_ceremony, 1), "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "runtime default")}
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
