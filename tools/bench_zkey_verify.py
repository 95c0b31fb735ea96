#!/usr/bin/env python3
"""Times `zkey verify` on the device (zkwg.phase2.verify_from_init / verify -> zkwg_point_rlc_device with two arrays, zkwg_zkey_new;
pairings on the host) for a key of the headline shape: domain 2^21, 1,776,821 wires, 20 public.

THE KEY is made by the operations under test themselves, so that a verification of it has a verdict: an .r1cs of 2^21 - 21 constraints
with one term a side (A: coefficient 1, B: r - 1, C: a small integer; the wires in turn, the last private wire in no constraint, so
section 8 holds a point at infinity) and toy multiples of the generators for the powers of tau (prover.fixed_base of 1, 2, 3, ..., as
tools/bench_phase2.py's yardstick has them) go through setup.new_zkey; phase2.contribute makes the key that is checked.

THE YARDSTICKS are the parent's own operations, timed in the same process: that contribute (what the verification checks) and that
new_zkey (what `verify` repeats before it does anything else).  Every run is recorded; the ratios use the fastest of each.

verify_from_init is split by where the time goes: uploads, the two folds, the pairings, the challenge points (one scaling of a G2 point
each), and the host's share -- zkwg_zkey_check of both files, the byte comparison of sections 3 - 7, the rest (random scalars, hashing).
The verdicts are CHECKED: the contributed key passes every check from the initial key and by rebuild, and with two points of section 9
swapped it fails `section_9` alone.  Prints one JSON line; exits non-zero on a wrong verdict.

    python tools/bench_zkey_verify.py [--power 21 --wires 1776821] [--reps 2] [--no-rebuild] > profiles/r12/r12_a_bench_zkey_verify.json
"""
import argparse
import json
import os
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "zk-email-verify_amd", "py"))

N_PUBLIC = 20


def headline_r1cs(power, n_wires):
    """2^power - N_PUBLIC - 1 constraints (a_k)(-b_k) = 3 c_k over the wires in turn, written with numpy (the dict form of
    zkwg.r1cs.write_r1cs would take minutes at this size); the last wire occurs in no constraint"""
    import numpy as np
    from zkwg.zkey import R
    m, used = (1 << power) - N_PUBLIC - 1, n_wires - 2
    term = [("n", "<u4"), ("wire", "<u4"), ("value", "u1", 32)]
    rows = np.zeros(m, dtype=[(f"{name}_{f}", *t) for name in "abc" for f, *t in term])
    k = np.arange(m, dtype=np.int64)
    for j, (name, coef) in enumerate((("a", 1), ("b", R - 1), ("c", 3))):
        rows[f"{name}_n"] = 1
        rows[f"{name}_wire"] = 1 + (k * 3 + j) % used
        rows[f"{name}_value"] = np.frombuffer(coef.to_bytes(32, "little"), dtype=np.uint8)
    hdr = struct.pack("<I", 32) + R.to_bytes(32, "little") + struct.pack("<IIIIQI", n_wires, 0, N_PUBLIC, n_wires - 1 - N_PUBLIC, n_wires, m)
    secs = [(1, hdr), (2, rows.tobytes()), (3, np.arange(n_wires, dtype="<u8").tobytes())]
    return b"r1cs" + struct.pack("<II", 1, len(secs)) + b"".join(struct.pack("<IQ", t, len(d)) + d for t, d in secs)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--power", type=int, default=21)
    ap.add_argument("--wires", type=int, default=1776821)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--no-rebuild", action="store_true", help="skip `verify` with its rebuild (a second key in host memory)")
    args = ap.parse_args(argv)
    import torch
    from zkwg import pairing, phase2, prover, ptau, setup, zkey
    n, nv = 1 << args.power, args.wires
    sync = lambda: torch.cuda.synchronize()
    t0 = time.time()
    r1cs = headline_r1cs(args.power, nv)
    assert setup.key_shape(r1cs)[0] == args.power
    g1 = prover.fixed_base(0, 1, range(1, 2 * n + 1))
    g2 = prover.fixed_base(0, 2, range(1, n + 1))
    down = lambda t: bytes(t.cpu().numpy())
    slices = {"power": args.power, "tau_g1": g1[:64 * n], "tau_g2": g2, "alpha_tau_g1": g1[64 * n:], "beta_tau_g1": g1[:64 * n], "tau_g1_next": g1,
              "alpha1": down(prover.fixed_base(0, 1, [3])), "beta1": down(prover.fixed_base(0, 1, [5])), "beta2": down(prover.fixed_base(0, 2, [5]))}
    t_inputs = time.time() - t0
    # ---- yardstick: new_zkey (its first run at this size) ------------------------------------------------------------------------------------
    new_runs = []
    for _ in range(args.reps):
        sync()
        t0 = time.time()
        z0 = setup.new_zkey(r1cs, slices)
        st = setup.last_stats()
        new_runs.append({"wall_s": round(time.time() - t0, 3), "seconds": {k: round(v, 4) for k, v in st["seconds"].items()}})
    # ---- yardstick: the contribution that is checked -----------------------------------------------------------------------------------------
    con_runs = []
    for _ in range(args.reps):
        sync()
        t0 = time.time()
        z1 = phase2.contribute(z0, "bench", urandom=lambda m: (bytes([7]) * 64)[:m])
        con_runs.append({"wall_s": round(time.time() - t0, 3), "apply_delta_s": {k: round(v, 4) for k, v in phase2.last_stats()["seconds"].items()}})
    # ---- verify_from_init, split -------------------------------------------------------------------------------------------------------------
    split = {"upload": 0.0, "folds": 0.0, "pairings": 0.0, "challenge_points": 0.0, "host_zkey_check": 0.0, "host_compare_sections": 0.0}

    def timed(key, fn, device=True):
        def wrapper(*a, **kw):
            t = time.time()
            out = fn(*a, **kw)
            if device:
                sync()
            split[key] += time.time() - t
            return out
        return wrapper
    D = ptau._Device
    saved = (D.upload, D.rlc, pairing.check, phase2.challenge_g2, phase2._zkey_check, phase2._first_difference)
    D.upload, D.rlc = timed("upload", D.upload), timed("folds", D.rlc)
    pairing.check = timed("pairings", pairing.check, device=False)
    phase2.challenge_g2 = timed("challenge_points", phase2.challenge_g2)
    phase2._zkey_check = timed("host_zkey_check", phase2._zkey_check, device=False)
    phase2._first_difference = timed("host_compare_sections", phase2._first_difference, device=False)
    ok, ver_runs, reb_runs = True, [], []
    verdict = lambda res: {name: (o if o is None else bool(o)) for name, o, _ in res["checks"]}
    try:
        for _ in range(args.reps):
            for k in split:
                split[k] = 0.0
            sync()
            t0 = time.time()
            res = phase2.verify_from_init(z0, z1)
            wall = time.time() - t0
            ok &= res["ok"] and all(o is True for _, o, _ in res["checks"])
            ver_runs.append({"wall_s": round(wall, 3), "split_s": {k: round(v, 3) for k, v in split.items()}, "host_rest_s": round(wall - sum(split.values()), 3),
                             "checks": verdict(res)})
    finally:
        D.upload, D.rlc, pairing.check, phase2.challenge_g2, phase2._zkey_check, phase2._first_difference = saved
    # ---- verify, with its rebuild ------------------------------------------------------------------------------------------------------------
    if not args.no_rebuild:
        for _ in range(args.reps):
            sync()
            t0 = time.time()
            res = phase2.verify(r1cs, slices, z1)
            reb_runs.append({"wall_s": round(time.time() - t0, 3)})
            ok &= res["ok"] and all(o is True for _, o, _ in res["checks"])
    # ---- a tampered key must fail --------------------------------------------------------------------------------------------------------------
    o9 = zkey.sections(z1)[9][0]
    bad = bytearray(z1)
    a, c = o9 + 64 * (n - 3), o9 + 64 * (n - 2)
    bad[a:a + 64], bad[c:c + 64] = z1[c:c + 64], z1[a:a + 64]
    res = phase2.verify_from_init(z0, bytes(bad))
    tampered = [name for name, o, _ in res["checks"] if o is False]
    ok &= (not res["ok"]) and tampered == ["section_9"]
    sec8 = zkey.sections(z1)[8]
    ok &= not any(z1[sec8[0] + sec8[1] - 64:sec8[0] + sec8[1]])               # the unused wire: a point at infinity among the folded points
    best = lambda runs: min(r["wall_s"] for r in runs)
    v, c_, s_ = best(ver_runs), best(con_runs), best(new_runs)
    out = {"key": {"domain_log2": args.power, "wires": nv, "n_public": N_PUBLIC, "points_section_8": nv - N_PUBLIC - 1, "points_section_9": n,
                   "zkey_bytes": len(z1), "r1cs_bytes": len(r1cs), "constraints": n - N_PUBLIC - 1},
           "new_zkey": new_runs, "contribute": con_runs, "verify_from_init": ver_runs, "verify_with_rebuild": reb_runs,
           "ratio": {"verify_from_init_over_contribute": round(v / c_, 3), "verify_from_init_over_new_zkey": round(v / s_, 3),
                     "verify_with_rebuild_over_new_zkey": round(best(reb_runs) / s_, 3) if reb_runs else None,
                     "verify_with_rebuild_over_contribute": round(best(reb_runs) / c_, 3) if reb_runs else None},
           "tampered_key_fails": tampered, "verdicts_right": bool(ok), "inputs_build_s": round(t_inputs, 1)}
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
