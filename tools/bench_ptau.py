#!/usr/bin/env python3
"""Times `powersoftau prepare phase2` on the device (zkwg.ptau.prepare -> zkwg_ptau_prepare -> zk_ptau_stage): an UNPREPARED file of
--power is made from a known (tau, alpha, beta) with zkwg_fixed_base_device, prepared, and CHECKED: sampled points of every level of
every section, the first and the last of each level included, against their discrete logarithms -- level q <= power in closed form,
L_j(tau) = (tau^m - 1) w^j / (m (tau - w^j)), m = 2^q; the padded level of section 12 less tau^(2 n - 1) w^j / (2 n).  Prints one JSON
line: wall time, the split of zkwg_ptau_prepare_stats, and per level of sections 12 and 13 the nanoseconds per butterfly (a level of 2^q
points is 2^(q - 1) q butterflies; its 2^-q scaling is in the time) beside a PREDICTION from operation counts.

THE YARDSTICK, in the same process: zkwg_point_scale_device (one shared scalar, curve check and conversion included) on as many points
as the largest level, in ns per point -- Y.  Field products (csrc/zkwg_ptau_core.h): a scaled point 3,221 + 27 = 3,248; a butterfly
whose wavefront holds k twiddles 254 x 9 + f(k) 254 x 11 + 23 + 2 x 27 with f(1) = 85 / 254, f(k) = 1 - (2/3)^k, none for twiddle 1.
predicted(level q) = Y / 3,248 x (2^q x 3,248 + sum over stages of the butterflies' products) / (2^(q - 1) q).

    python tools/bench_ptau.py [--power 16] [--samples 8] [--reps 2]
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

SCALE_PRODUCTS = 254 * 9 + 85 * 11 + 27


def stage_products(q, s, per):
    """field products of all butterflies of stage s of a 2^q-point transform; per: butterflies a wavefront (64 / 32)"""
    groups, tw = 1 << (q - 1 - s), 1 << s
    k = max(1, min(tw, per // groups)) if groups < per else 1          # twiddles a wavefront
    f = 85 / 254 if k == 1 else 1 - (2 / 3) ** k
    walk = 254 * 9 + f * 254 * 11
    return groups * ((tw - 1) * walk + tw * (23 + 2 * 27))


def predicted_ns_per_butterfly(q, per, yard_ns):
    total = (1 << q) * SCALE_PRODUCTS + sum(stage_products(q, s, per) for s in range(q))
    return yard_ns / SCALE_PRODUCTS * total / ((1 << (q - 1)) * q)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--power", type=int, default=16)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args(argv)
    import torch
    from zkwg import _lib, prover, ptau
    R = prover.R
    lib = _lib.load()
    up = lambda g, s: prover.fixed_base(0, g, s)
    down = lambda t: bytes(t.cpu().numpy())
    p, n = args.power, 1 << args.power
    rng = random.Random(11)
    tau, alpha, beta = (rng.randrange(2, R) for _ in range(3))
    # ---- the unprepared file ---------------------------------------------------------------------------------------------------------------
    t0 = time.time()
    pw = [1] * (2 * n - 1)
    for k in range(1, 2 * n - 1):
        pw[k] = pw[k - 1] * tau % R
    d2, d3 = up(1, pw), up(2, pw[:n])
    secs = {2: down(d2), 3: down(d3), 4: down(up(1, [alpha * x % R for x in pw[:n]])), 5: down(up(1, [beta * x % R for x in pw[:n]])), 6: down(up(2, [beta]))}
    del pw
    pot = ptau.write_ptau(p, secs)
    del secs
    t_file = time.time() - t0
    # ---- the preparation -------------------------------------------------------------------------------------------------------------------
    runs = []
    for _ in range(args.reps):
        t0 = time.time()
        out = ptau.prepare(pot)
        st = ptau.last_stats()
        st["wall_s"] = round(time.time() - t0, 3)
        runs.append(st)
    best = min(runs, key=lambda r: r["wall_s"])
    info = ptau.read_ptau(out)
    # ---- the check -------------------------------------------------------------------------------------------------------------------------
    root = lambda q: pow(5, ((R - 1) >> 28) << (28 - q), R)          # Fr.w[q] of ffjavascript (nqr = 5, s = 28)

    def lagrange(q, j, padded):
        m, w = 1 << q, pow(root(q), j, R)
        v = (pow(tau, m, R) - 1) * w % R * pow(m * (tau - w) % R, -1, R) % R
        return (v - pow(tau, m - 1, R) * w % R * pow(m, -1, R)) % R if padded else v

    srng = random.Random(3)
    ok, checked = True, 0
    for sid, group, factor in ((12, 1, 1), (13, 2, 1), (14, 1, alpha), (15, 1, beta)):
        pt = 64 if group == 1 else 128
        where, logs = [], []
        for q in range(p + (2 if sid == 12 else 1)):
            m = 1 << q
            for j in sorted({0, m - 1, m // 2} | {srng.randrange(m) for _ in range(args.samples)}):
                where.append((q, j))
                logs.append(lagrange(q, j, q == p + 1) * factor % R)
        want = down(up(group, logs))
        for t, (q, j) in enumerate(where):
            ok &= bytes(ptau.level(out, info, sid, q)[pt * j:pt * j + pt]) == want[pt * t:pt * t + pt]
        checked += len(where)
    src = ptau.read_ptau(pot, prepared=False)
    ok &= all(out[info["sections"][s][0]:info["sections"][s][0] + info["sections"][s][1]] == pot[src["sections"][s][0]:src["sections"][s][0] + src["sections"][s][1]] for s in range(1, 8))
    out_bytes = len(out)
    del out, pot
    # ---- the yardstick ---------------------------------------------------------------------------------------------------------------------
    scalar = (rng.randrange(R)).to_bytes(32, "little")
    yard = {}
    for group, d, cnt in ((1, d2, 2 * n), (2, d3, n)):
        pt = 64 if group == 1 else 128
        src_t = torch.zeros(cnt * pt, dtype=torch.uint8, device="cuda:0")
        src_t[:d.numel()] = d.reshape(-1)
        dst = torch.empty_like(src_t)
        ts = []
        for _ in range(max(3, args.reps)):
            torch.cuda.synchronize()
            t0 = time.time()
            rc = lib.zkwg_point_scale_device(0, group, src_t.data_ptr(), cnt, scalar, dst.data_ptr(), 0)
            ts.append(time.time() - t0)
            assert rc == 0
        yard[group] = {"points": cnt, "ns_per_point": round(min(ts) / cnt * 1e9, 2), "ns_per_point_all_runs": [round(t / cnt * 1e9, 2) for t in ts]}
        del src_t, dst
    levels = {}
    for i, (sid, group, per) in enumerate(((12, 1, 64), (13, 2, 32))):
        y = yard[group]["ns_per_point"]
        rows = []
        for q in range(1, p + (2 if sid == 12 else 1)):
            bf = (1 << (q - 1)) * q
            got = [r[sid]["levels"][q] / bf * 1e9 for r in runs]
            pred = predicted_ns_per_butterfly(q, per, y)
            rows.append({"level": q, "butterflies": bf, "ns_per_butterfly": round(min(got), 2), "all_runs": [round(g, 2) for g in got],
                         "predicted": round(pred, 2), "ratio": round(min(got) / pred, 3)})
        levels[sid] = rows
    torch.cuda.synchronize()
    sec = {sid: {k: (round(v, 4) if isinstance(v, float) else v) for k, v in best[sid].items() if k != "levels"} for sid in (12, 13, 14, 15)}
    res = {"power": p, "prepared_bytes": out_bytes, "wall_s": best["wall_s"], "wall_s_all_runs": [r["wall_s"] for r in runs], "sections": sec,
           "transforms_share_of_wall": round(sum(best[s]["transforms"] for s in (12, 13, 14, 15)) / best["wall_s"], 3),
           "yardstick_zkwg_point_scale_device": yard, "levels": levels,
           "checked_against_discrete_logarithms": bool(ok), "points_checked": checked, "file_build_s": round(t_file, 1),
           "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "runtime default")}
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
