#!/usr/bin/env python3
"""Times `powersoftau verify` on the device (zkwg.ptau.verify -> zkwg_g2_subgroup_device / zkwg_point_rlc_device; pairings on the host).

THE KERNEL AND ITS YARDSTICK, in the same process, alternating, on the 2^20 G2 points of section 3 of a contributed power-20 file (one
warm-up call each, then --reps timed calls; medians, every run listed):
    N   ns per point of zkwg_g2_subgroup_device (curve check + the criterion A + Q + psi(A) + psi^2(A) = psi^3(2 A), A = [u] Q)
    Y   ns per point of zkwg_point_scale_device(2, scalar = r): the DEFINITION [r] Q = infinity by the parent commit's kernel (curve check,
        the walk over the non-adjacent form of r, and the conversion to affine points the call ends with)
PREDICTED_RATIO is the ratio of the Fq2-product counts of csrc/zkwg_verify_core.h: 848 against 3,016 + 27.  The new kernel has to beat
ratio 1.0 -- the definition's own walk -- to be worth keeping.  The verdicts are CHECKED: none of the file's points may be outside, and
planted points (a raw twist point, points of order 10069) must be counted and located; Y must give zeros for every point.

THE WHOLE VERIFICATION of the prepared file, split by where the time goes (uploads, the subgroup test, the powers' sums, the Lagrange
sums and transforms, pairings and challenge points, the rest: hashing, scalars).  Prints one JSON line; exits non-zero on a wrong verdict.

    python tools/bench_ptau_verify.py [--power 20] [--reps 5] > profiles/r11/r11_a_bench_ptau_verify_p20.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "zk-email-verify_amd", "py"))

PREDICTED_RATIO = (62 * 9 + 23 * 10 + (10 + 2 * 14 + 9) + 9 + 4) / (254 * 9 + 73 * 10 + 27)


def _twist_point_outside(seed):
    """a point of the twist by try-and-increment, the cofactor not cleared, and its multiple of order 10069 (bytes in the zkey's form)"""
    import hashlib
    from zkwg import _call, phase2
    from zkwg.zkey import Q, R
    for counter in range(1 << 16):
        h = [hashlib.blake2b(seed + bytes([counter & 255, counter >> 8, half]), digest_size=64).digest() for half in (0, 1)]
        x = (int.from_bytes(h[0], "little") % Q, int.from_bytes(h[1], "little") % Q)
        x3 = phase2._f2_mul(phase2._f2_mul(x, x), x)
        y = phase2._f2_sqrt(((x3[0] + phase2._B2[0]) % Q, (x3[1] + phase2._B2[1]) % Q))
        if y is None:
            continue
        raw = b"".join(_call.mont(v) for v in (x[0], x[1], y[0], y[1]))
        small = phase2.scale_points(2, phase2.scale_points(2, raw, R), (2 * Q - R) // 10069)
        if any(small):
            return raw, small
    raise RuntimeError("no twist point found")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--power", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args(argv)
    import torch
    from zkwg import _lib, pairing, phase2, ptau
    from zkwg.zkey import R
    lib = _lib.load()
    p, n = args.power, 1 << args.power
    t0 = time.time()
    pot = ptau.contribute(ptau.new(p), "bench", urandom=lambda m: (bytes([7]) * 64)[:m])
    pot = ptau.beacon(pot, "bench beacon", "01" * 32, 10)
    t_make = time.time() - t0
    t0 = time.time()
    prepared = ptau.prepare(pot)
    t_prepare = time.time() - t0
    info = ptau.read_ptau(pot, prepared=False)
    ok = True
    # ---- the kernel against the definition -----------------------------------------------------------------------------------------------------
    import ctypes as C
    o = info["sections"][3][0]
    src = torch.frombuffer(bytearray(pot[o:o + 128 * n]), dtype=torch.uint8).to("cuda:0")
    dst = torch.empty_like(src)
    r32 = R.to_bytes(32, "little")
    n_bad, first = C.c_uint64(), C.c_uint64()
    calls = {"subgroup": lambda: lib.zkwg_g2_subgroup_device(0, src.data_ptr(), n, C.byref(n_bad), C.byref(first), 0),
             "definition": lambda: lib.zkwg_point_scale_device(0, 2, src.data_ptr(), n, r32, dst.data_ptr(), 0)}
    ts = {name: [] for name in calls}
    for rep in range(args.reps + 1):                               # (the first round warms both calls up)
        for name, call in calls.items():
            torch.cuda.synchronize()
            t0 = time.time()
            rc = call()
            dt = time.time() - t0
            assert rc == 0, (name, rc)
            if rep:
                ts[name].append(dt)
        ok &= n_bad.value == 0 and not bool(dst.any().item())
    raw, small = _twist_point_outside(b"zkwg bench verify")
    planted = src.clone()
    spots = sorted({1, n // 3, n - 1})
    for k, at in enumerate(spots):
        planted[128 * at:128 * at + 128] = torch.frombuffer(bytearray(raw if k == 0 else small), dtype=torch.uint8).to("cuda:0")
    rc = lib.zkwg_g2_subgroup_device(0, planted.data_ptr(), n, C.byref(n_bad), C.byref(first), 0)
    ok &= rc == 0 and n_bad.value == len(spots) and first.value == spots[0]
    rc = lib.zkwg_point_scale_device(0, 2, planted.data_ptr(), n, r32, dst.data_ptr(), 0)
    nonzero = dst.view(n, 128).any(dim=1).nonzero().flatten().tolist()
    ok &= rc == 0 and nonzero == spots
    med = {name: statistics.median(v) for name, v in ts.items()}
    kernel = {"points": n, "N_subgroup_ns_per_point": round(med["subgroup"] / n * 1e9, 2), "Y_definition_ns_per_point": round(med["definition"] / n * 1e9, 2),
              "ratio_N_over_Y": round(med["subgroup"] / med["definition"], 3), "predicted_ratio": round(PREDICTED_RATIO, 3), "ratio_to_beat": 1.0,
              "all_runs_ns_per_point": {name: [round(t / n * 1e9, 2) for t in v] for name, v in ts.items()},
              "planted_points_found": bool(n_bad.value == len(spots))}
    del src, dst, planted
    # ---- the whole verification, split -------------------------------------------------------------------------------------------------------------
    split = {"upload": 0.0, "subgroup": 0.0, "powers_sums": 0.0, "lagrange_sums": 0.0, "lagrange_transforms": 0.0, "pairings": 0.0, "challenge_points": 0.0}

    def timed(key, fn, sync=True):
        def wrapper(*a, **kw):
            t = time.time()
            out = fn(*a, **kw)
            if sync:
                torch.cuda.synchronize()
            split[key(*a, **kw) if callable(key) else key] += time.time() - t
            return out
        return wrapper
    D = ptau._Device
    saved = (D.upload, D.g2_subgroup, D.rlc, D.ifft, pairing.check, ptau.pok_challenge_point)
    D.upload, D.g2_subgroup, D.ifft = timed("upload", D.upload), timed("subgroup", D.g2_subgroup), timed("lagrange_transforms", D.ifft)
    D.rlc = timed(lambda *a, **kw: "powers_sums" if kw.get("shifted") else "lagrange_sums", D.rlc)
    pairing.check = timed("pairings", pairing.check, sync=False)
    ptau.pok_challenge_point = timed("challenge_points", ptau.pok_challenge_point)
    walls, results = [], []
    try:
        for state, data in (("not prepared", pot), ("prepared", prepared), ("prepared", prepared)):      # (the second prepared run is the warm one)
            for k in split:
                split[k] = 0.0
            t0 = time.time()
            res = ptau.verify(data)
            wall = time.time() - t0
            ok &= res["ok"]
            walls.append(wall)
            results.append({"state": state, "wall_s": round(wall, 3), "split_s": {k: round(v, 3) for k, v in split.items()},
                            "rest_s": round(wall - sum(split.values()), 3), "checks": {name: (o_ if o_ is None else bool(o_)) for name, o_, _ in res["checks"]}})
    finally:
        D.upload, D.g2_subgroup, D.rlc, D.ifft, pairing.check, ptau.pok_challenge_point = saved
    # a tampered file must fail
    o13 = ptau.read_ptau(prepared)["sections"][13][0]
    bad = bytearray(prepared)
    a, c = o13 + 128 * ((n >> 1) - 1 + 3), o13 + 128 * ((n >> 1) - 1 + 4)
    bad[a:a + 128], bad[c:c + 128] = prepared[c:c + 128], prepared[a:a + 128]
    res = ptau.verify(bytes(bad))
    ok &= (not res["ok"]) and [name for name, o_, _ in res["checks"] if o_ is False] == ["lagrange_13"]
    out = {"power": p, "file_bytes": len(pot), "prepared_file_bytes": len(prepared), "make_s": round(t_make, 3), "prepare_s": round(t_prepare, 3),
           "kernel": kernel, "verify": results, "verdicts_right": bool(ok), "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "runtime default")}
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
