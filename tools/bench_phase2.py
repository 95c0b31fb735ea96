#!/usr/bin/env python3
"""Times one phase-2 contribution on the device (zkwg.phase2.apply_delta -> zkwg_zkey_apply_delta -> zk_phase2_scale) for a key of the
headline shape: domain 2^21, 1,776,821 wires, 20 public -- sections 8 and 9 are multiples of the generator with known logarithms
(prover.fixed_base), sections 3 - 7 points at infinity (the operation copies them), section 4 empty.  Prints one JSON line: the wall
time split of zkwg_zkey_apply_delta_stats, group operations per second of the two scalings, and the time per point.

The key is CHECKED: sampled points of sections 8 and 9, the first and the last of each included, and delta1 / delta2 against their
discrete logarithms.

THE YARDSTICK is the primitive that existed before this kernel, in the same process on the same device: zk_setup_mul, plain binary
double-and-add, which zkwg_zkey_new runs when a wire has a single field-size coefficient.  An .r1cs of --yard-power (default 2^20)
one-term constraints, every A term with the SAME field-size coefficient on a wire of its own, makes the section-5 sum exactly that many
one-term zk_setup_mul calls (plus nPublic + 1 mixed additions); its seconds come from zkwg_zkey_new_stats.  That figure includes the
sum's own conversion to affine points and the download of its section, so the comparison is made twice: kernel time of the scaling
against the whole yardstick (favours the new code) and scaling + conversion + download of this run against it (like for like).

    python tools/bench_phase2.py [--power 21 --wires 1776821] [--yard-power 20] [--samples 32] [--reps 2]
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "zk-email-verify_amd", "py"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--power", type=int, default=21)
    ap.add_argument("--wires", type=int, default=1776821)
    ap.add_argument("--yard-power", type=int, default=20)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args(argv)
    import torch
    from zkwg import phase2, prover, setup, zkey
    from zkwg import r1cs as zr
    R = prover.R
    up = lambda g, s: prover.fixed_base(0, g, s)
    down = lambda t: bytes(t.cpu().numpy())
    n_public, nv, n = 20, args.wires, 1 << args.power
    n8 = nv - n_public - 1
    rng = random.Random(9)
    # ---- the key -------------------------------------------------------------------------------------------------------------------------
    t0 = time.time()
    c0, c1, h0, h1, delta0 = (rng.randrange(2, R) for _ in range(5))
    c_log = lambda i: (c0 + c1 * i) % R
    h_log = lambda j: (h0 + h1 * j) % R
    sec8, sec9 = down(up(1, [c_log(i) for i in range(n8)])), down(up(1, [h_log(j) for j in range(n)]))
    pts = {"alpha1": down(up(1, [3])), "beta1": down(up(1, [5])), "beta2": down(up(2, [5])), "gamma2": down(up(2, [1])),
           "delta1": down(up(1, [delta0])), "delta2": down(up(2, [delta0]))}
    z = zkey.write_zkey(nv, n_public, n, pts, bytes(64 * (n_public + 1)), bytes(64 * nv), bytes(64 * nv), bytes(128 * nv), sec8, sec9)
    del sec8, sec9
    zlen = len(z)
    t_key = time.time() - t0
    # ---- the contribution ----------------------------------------------------------------------------------------------------------------
    k = phase2.derive_scalar(b"bench")
    kinv = pow(k, -1, R)
    runs = []
    for _ in range(args.reps):
        t0 = time.time()
        z1 = phase2.apply_delta(z, k, bytes(68))
        st = phase2.last_stats()
        st["wall_s"] = round(time.time() - t0, 3)
        runs.append(st)
    best = min(runs, key=lambda r: r["wall_s"])
    sec = best["seconds"]
    d = zkey.read_zkey(z1, coeffs=False)
    srng = random.Random(2)
    i8 = [0, 1, n8 - 1] + [srng.randrange(n8) for _ in range(args.samples)]
    i9 = [0, 1, n - 1] + [srng.randrange(n) for _ in range(args.samples)]
    w8, w9 = down(up(1, [c_log(i) * kinv % R for i in i8])), down(up(1, [h_log(j) * kinv % R for j in i9]))
    ok = all(d["c"][64 * i:64 * i + 64] == w8[64 * t:64 * t + 64] for t, i in enumerate(i8))
    ok &= all(d["h"][64 * j:64 * j + 64] == w9[64 * t:64 * t + 64] for t, j in enumerate(i9))
    ok &= d["delta1"] == down(up(1, [delta0 * k % R])) and d["delta2"] == down(up(2, [delta0 * k % R]))
    ok &= d["a"] == bytes(64 * nv) and d["alpha1"] == pts["alpha1"] and d["gamma2"] == pts["gamma2"] and len(z1) == len(z)
    ops = best["ops"]
    scal = {}
    for name, key in (("c", "scale_c"), ("h", "scale_h")):
        o = ops[name]
        scal[name] = {"seconds": round(sec[key], 4), "additions": o["add"], "doublings": o["dbl"],
                      "group_ops_per_s": round((o["add"] + o["dbl"]) / sec[key] / 1e9, 3), "unit": "G"}
    new_kernel_ns = (sec["scale_c"] + sec["scale_h"]) / (n8 + n) * 1e9
    new_all_ns = (sec["scale_c"] + sec["scale_h"] + sec["affine_download"]) / (n8 + n) * 1e9
    del z, z1, d
    # ---- the yardstick -------------------------------------------------------------------------------------------------------------------
    t0 = time.time()
    yn = 1 << args.yard_power
    m = yn - 2                                                  # constraints; one public wire: m + nPublic + 1 <= 2^yard_power
    coef = kinv                                                 # the same field-size coefficient on every wire
    cons = [({j: coef}, {0: 1}, {}) for j in range(m)]
    r1cs = zr.write_r1cs(m, cons, n_pub_out=1, n_pub_in=0, n_prv_in=m - 2)
    del cons
    g1 = up(1, list(range(1, 2 * yn + 1)))
    g2 = up(2, list(range(1, yn + 1)))
    slices = {"power": args.yard_power, "tau_g1": g1[:64 * yn], "tau_g2": g2, "alpha_tau_g1": g1[:64 * yn], "beta_tau_g1": g1[:64 * yn],
              "tau_g1_next": g1, "alpha1": pts["alpha1"], "beta1": pts["beta1"], "beta2": pts["beta2"]}
    yard_runs = []
    for _ in range(args.reps):
        zy = setup.new_zkey(r1cs, slices)
        yard_runs.append(setup.last_stats())
    ys = min(yard_runs, key=lambda r: r["seconds"]["sum_a"])
    # (the yardstick's own result: wire j of section 5 = coef (j + 1) G)
    dy = zkey.read_zkey(zy, coeffs=False)
    jy = [2, 3, m - 1] + [srng.randrange(2, m) for _ in range(8)]
    wy = down(up(1, [coef * (j + 1) % R for j in jy]))
    ok_y = all(dy["a"][64 * j:64 * j + 64] == wy[64 * t:64 * t + 64] for t, j in enumerate(jy))
    yard_ns = ys["seconds"]["sum_a"] / m * 1e9
    t_yard = time.time() - t0
    torch.cuda.synchronize()
    out = {"key": {"domain_log2": args.power, "wires": nv, "n_public": n_public, "points_section_8": n8, "points_section_9": n, "zkey_bytes": zlen},
           "seconds": {k_: round(v, 4) for k_, v in sec.items()}, "wall_s": best["wall_s"], "wall_s_all_runs": [r["wall_s"] for r in runs],
           "scaling": scal, "scaling_share_of_wall": round((sec["scale_c"] + sec["scale_h"]) / best["wall_s"], 3),
           "ns_per_point": {"zk_phase2_scale": round(new_kernel_ns, 2), "zk_phase2_scale_plus_conversion_and_download": round(new_all_ns, 2),
                            "yardstick_zk_setup_mul_sum_a": round(yard_ns, 2)},
           "ratio_to_yardstick": {"kernel_only": round(new_kernel_ns / yard_ns, 3), "with_conversion_and_download": round(new_all_ns / yard_ns, 3)},
           "yardstick": {"constraints": m, "domain_log2": args.yard_power, "sum_a_s": round(ys["seconds"]["sum_a"], 4), "ops_a": ys["ops"]["a"],
                         "sum_a_s_all_runs": [round(r["seconds"]["sum_a"], 4) for r in yard_runs], "checked": bool(ok_y)},
           "key_checked_against_discrete_logarithms": bool(ok), "points_checked": len(i8) + len(i9) + 2,
           "key_build_s": round(t_key, 1), "yardstick_build_and_run_s": round(t_yard, 1), "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "runtime default")}
    print(json.dumps(out))
    return 0 if ok and ok_y else 1


if __name__ == "__main__":
    sys.exit(main())
