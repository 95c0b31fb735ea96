#!/usr/bin/env python3
"""Times `powersoftau new / contribute` on the device (zkwg.ptau.contribute -> zkwg_ptau_apply_key -> zk_ptau_key_walk): the file of
--power is made by zkwg.ptau.new, then contributed to TWICE with seeded secrets (the second contribution meets bases that are no
generators), and CHECKED: sampled points of every section of the result, the first and the last included, against their closed-form
logarithms (point k of sections 2 / 3: (tau1 tau2)^k; 4: alpha1 alpha2 (tau1 tau2)^k; 5: beta ...; 6: beta1 beta2) through
zkwg_fixed_base_device.  Prints one JSON line: per contribution the wall time and the split of zkwg_ptau_apply_key_stats per section.

THE PRIMITIVE AND ITS YARDSTICK, in the same process, alternating, on 2^20 G1 / 2^19 G2 points of the contributed file (curve check and
conversion to affine included in both; best of --reps after one warm-up call each, every run listed):
    N   ns per point of zkwg_point_mul_device (each point its own scalar, uniform below 2^253), and of zkwg_point_powers_device
    Y   ns per point of zkwg_point_scale_device (one shared scalar below r): the parent's kernel
A call built on the existing predicated walk would cost about 1.58 Y (csrc/zkwg_ptau_core.h); the window of csrc/zkwg_ptau_key_core.h
earns its place if N / Y is below that.  PREDICTED_RATIO is the ratio of the field-product counts of that header (3,198 + 27 against
3,136 + 27; with the older count of 11 / 15 products per mixed / full addition: 3,269 + 27 against 3,221 + 27).

    python tools/bench_ptau_contribute.py [--power 20] [--samples 8] [--reps 3]
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

PREDICTED_RATIO = (63 * 46 + (7 + 10 + 6 * 14) + 7 * 27 + 10 + 27) / (254 * 9 + 85 * 10 + 27)
PREDICTED_RATIO_OLD_COUNTS = (63 * 47 + (7 + 11 + 6 * 15) + 7 * 27 + 11 + 27) / (254 * 9 + 85 * 11 + 27)
PREDICATED_WALK_RATIO = 1.58


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--power", type=int, default=20)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args(argv)
    import torch
    from zkwg import _lib, prover, ptau
    R = prover.R
    lib = _lib.load()
    down = lambda t: bytes(t.cpu().numpy())
    p, n = args.power, 1 << args.power
    # ---- new, then two contributions -----------------------------------------------------------------------------------------------------------
    t0 = time.time()
    pot = ptau.new(p)
    t_new = time.time() - t0
    keys, runs = [], []
    for i in range(2):
        seed = bytes([i + 1]) * 64
        keys.append(ptau.key_scalars(seed)[0])
        t0 = time.time()
        pot = ptau.contribute(pot, f"bench {i + 1}", urandom=lambda m, s=seed: s[:m])
        wall = time.time() - t0
        st = ptau.apply_key_stats()
        sections = {sid: {k: (round(v, 4) if isinstance(v, float) else v) for k, v in st[sid].items()} for sid in (2, 3, 4, 5)}
        for sid, cnt in ((2, 2 * n - 1), (3, n), (4, n), (5, n)):
            sections[sid]["points"] = cnt
            sections[sid]["device_ns_per_point"] = round((st[sid]["tables"] + st[sid]["walk"]) / cnt * 1e9, 2)
        apply_s = sum(st[sid][k] for sid in (2, 3, 4, 5) for k in ("upload_check", "tables", "walk", "affine_download")) + st["parse_copy"] + st[6]
        runs.append({"wall_s": round(wall, 3), "apply_key_s": round(apply_s, 3), "record_and_hash_s": round(wall - apply_s, 3), "parse_copy_s": round(st["parse_copy"], 4),
                     "section6_s": round(st[6], 4), "sections": sections})
    # ---- the check -------------------------------------------------------------------------------------------------------------------------------
    tau, alpha, beta = (keys[0][j] * keys[1][j] % R for j in range(3))
    info = ptau.read_ptau(pot, prepared=False)
    srng = random.Random(3)
    ok, checked = True, 0
    for sid, group, cnt, factor in ((2, 1, 2 * n - 1, 1), (3, 2, n, 1), (4, 1, n, alpha), (5, 1, n, beta), (6, 2, 1, beta)):
        pt = 64 if group == 1 else 128
        ks = sorted({0, cnt - 1, cnt // 2, min(cnt - 1, 1 << 20), min(cnt - 1, (1 << 20) - 1)} | {srng.randrange(cnt) for _ in range(args.samples)})
        want = down(prover.fixed_base(0, group, [factor * pow(tau, k, R) % R if sid != 6 else beta for k in ks]))
        o = info["sections"][sid][0]
        for t, k in enumerate(ks):
            ok &= pot[o + pt * k:o + pt * k + pt] == want[pt * t:pt * t + pt]
        checked += len(ks)
    ok &= len(ptau.read_contributions(pot)) == 2
    # ---- the primitive against the yardstick ---------------------------------------------------------------------------------------------------------
    rng = random.Random(11)
    shared = rng.randrange(R).to_bytes(32, "little")
    c32, t32 = rng.randrange(1, R).to_bytes(32, "little"), rng.randrange(1, R).to_bytes(32, "little")
    prim = {}
    for group, sid, cnt in ((1, 2, min(1 << 20, 2 * n - 1)), (2, 3, min(1 << 19, n))):
        pt = 64 if group == 1 else 128
        o = info["sections"][sid][0]
        src = torch.frombuffer(bytearray(pot[o:o + cnt * pt]), dtype=torch.uint8).to("cuda:0")
        dst = torch.empty_like(src)
        k = torch.randint(0, 256, (cnt, 32), dtype=torch.uint8, generator=torch.Generator().manual_seed(5 + group))
        k[:, 31] &= 0x1f                                               # below 2^253 < r
        k = k.to("cuda:0")
        calls = {"point_mul": lambda: lib.zkwg_point_mul_device(0, group, src.data_ptr(), cnt, k.data_ptr(), dst.data_ptr(), 0),
                 "point_powers": lambda: lib.zkwg_point_powers_device(0, group, src.data_ptr(), cnt, c32, t32, 0, dst.data_ptr(), 0),
                 "point_scale": lambda: lib.zkwg_point_scale_device(0, group, src.data_ptr(), cnt, shared, dst.data_ptr(), 0)}
        ts = {name: [] for name in calls}
        for rep in range(args.reps + 1):                               # (the first round warms every call up)
            for name, call in calls.items():
                torch.cuda.synchronize()
                t0 = time.time()
                rc = call()
                dt = time.time() - t0
                assert rc == 0, (name, rc)
                if rep:
                    ts[name].append(dt)
        ns = {name: round(min(v) / cnt * 1e9, 2) for name, v in ts.items()}
        prim[group] = {"points": cnt, "N_point_mul_ns_per_point": ns["point_mul"], "N_point_powers_ns_per_point": ns["point_powers"], "Y_point_scale_ns_per_point": ns["point_scale"],
                       "ratio_N_over_Y": round(ns["point_mul"] / ns["point_scale"], 3), "ratio_powers_over_Y": round(ns["point_powers"] / ns["point_scale"], 3),
                       "all_runs_ns_per_point": {name: [round(t / cnt * 1e9, 2) for t in v] for name, v in ts.items()}}
        del src, dst, k
    torch.cuda.synchronize()
    res = {"power": p, "file_bytes": len(pot), "new_s": round(t_new, 3), "contributions": runs, "primitive": prim,
           "predicted_ratio_N_over_Y": round(PREDICTED_RATIO, 3), "predicted_ratio_with_the_older_counts": round(PREDICTED_RATIO_OLD_COUNTS, 3),
           "predicated_walk_ratio_to_beat": PREDICATED_WALK_RATIO,
           "below_the_predicated_walk": bool(all(v["ratio_N_over_Y"] < PREDICATED_WALK_RATIO for v in prim.values())),
           "checked_against_discrete_logarithms": bool(ok), "points_checked": checked,
           "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "runtime default")}
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
