#!/usr/bin/env python3
"""Times the prover of witnesses (zkwg.prover.WitnessProver: `groth16.prove(zkey, wtns)` for any key) beside what the handle path offers,
in one process, alternating, after a warm-up, device-event timed:

  * zk_zkey_abc (A.w | B.w | C.w of 8 resident witnesses from the key's own rows) against zkwg_r1cs_evaluate_device(montgomery = 0) on the
    same rows followed by zkwg_convert_montgomery_device of its output; its rate as terms/s and as bytes gathered per second;
  * proofs per second from host witnesses and from device-resident witnesses beside the handle path's (zkwg_prover_prove_prepared).

The key is tools/bench_prove.py's (bases from known discrete logarithms), written as a .zkey with its section 4.  Prints one JSON line.

    python tools/bench_prove_wtns.py [--max-header 1024 --max-body 1536] [--emails 8] [--slots 24] [--proofs 48]
"""
import argparse
import json
import os
import random
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "zk-email-verify_amd", "py"))

LAZY_RATE = 162.9e9         # field products/s of the 9 x 29-bit product in limb form (tools/mulbench.hip, profiles/r05/r05_g_mulbench.txt)


def section4_bytes(full):
    """section 4 of a .zkey from rows [(A, B, C) dicts]: (matrix, row, wire, coefficient x 2^512 mod r) for A and B"""
    from zkwg.zkey import R
    r2 = pow(1 << 256, 2, R)
    enc, parts, n = {}, [], 0
    for j, row in enumerate(full):
        for m in (0, 1):
            for w, v in row[m].items():
                v %= R
                if not v:
                    continue
                b = enc.get(v)
                if b is None:
                    b = enc[v] = (v * r2 % R).to_bytes(32, "little")
                parts.append(struct.pack("<III", m, j, w) + b)
                n += 1
    return n, struct.pack("<I", n) + b"".join(parts)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-header", type=int, default=1024)
    ap.add_argument("--max-body", type=int, default=1536)
    ap.add_argument("--emails", type=int, default=8)
    ap.add_argument("--slots", type=int, default=24)
    ap.add_argument("--proofs", type=int, default=48)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-only", type=int, default=0, help="1: skip the proofs-per-second part")
    args = ap.parse_args(argv)
    import torch
    import zkwg
    from zkwg import prover, synth, zkey
    from zkwg import r1cs as zr
    N, M, n = args.max_header, args.max_body, args.emails
    R = prover.R
    dev = torch.device("cuda", 0)
    t0 = time.time()
    c = zkwg.Circuit(zkwg.MAIN_EMAIL_VERIFIER, max_header=N, max_body=M, device=0)
    sym = c.symbols()
    n_public = 20
    full = zr.append_public_rows(zr.email_verifier_constraints(sym, N, M), n_public)
    data = zr.write_r1cs(len(sym), full, n_pub_out=3, n_pub_in=17, n_prv_in=N + 1 + 17 + 1 + 32 + M + 1)
    n_rows = len(full)
    power = max(1, (n_rows - 1).bit_length())
    rng = random.Random(1)
    pool = [rng.randrange(1, R) for _ in range(4096)]
    rep = lambda k: [pool[(7 * i + 3) % 4096] for i in range(k)]
    pk = prover.ProvingKey.from_scalars(0, n_public, power, rep(c.W), rep(c.W), rep(c.W - n_public - 1), rep(1 << power), 5, 7, 11)
    n_terms, s4 = section4_bytes(full)
    del full
    down = lambda t: bytes(t.cpu().numpy())
    hdr = struct.pack("<I", 32) + zkey.Q.to_bytes(32, "little") + struct.pack("<I", 32) + R.to_bytes(32, "little") + struct.pack("<III", c.W, n_public, 1 << power)
    hdr += pk.alpha1 + pk.beta1 + pk.beta2 + bytes(128) + pk.delta1 + pk.delta2
    secs = [(1, struct.pack("<I", 1)), (2, hdr), (3, bytes(64 * (n_public + 1))), (4, s4), (5, down(pk.d_a)), (6, down(pk.d_b1)), (7, down(pk.d_b2)),
            (8, down(pk.d_c)), (9, down(pk.d_h)), (10, bytes(64) + struct.pack("<I", 0))]
    z = b"zkey" + struct.pack("<II", 1, len(secs)) + b"".join(struct.pack("<IQ", i, len(p)) + p for i, p in secs)
    del s4, secs
    pv = prover.Prover(c, data, n_rows, pk)                      # the handle path (attaches the system to c)
    t_setup = time.time() - t0
    t0 = time.time()
    wp = prover.WitnessProver(z, device=0, slots=args.slots)
    t_create = time.time() - t0
    cs = zkwg.R1cs(data, device=0)
    recs, _ = synth.packed_batch(c, seed=9, n=n, body_len=min(1024 if M >= 1536 else 100, M - 80))
    wit, st = c.calculate_batch_host(recs)
    assert st == [0] * n
    W = c.W
    host_w = b"".join(wit[e * c.witness_bytes:e * c.witness_bytes + 32 * W] for e in range(n))
    del wit
    d_w = torch.frombuffer(bytearray(host_w), dtype=torch.uint8).to(dev)
    # ---- the kernel against zkwg_r1cs_evaluate_device + zkwg_convert_montgomery_device ------------------------------------------------
    def ours():
        return wp.abc_device(d_w, n)

    def theirs():
        out = cs.evaluate_device(d_w, n, 32 * W, montgomery=False)
        zkwg.convert_montgomery_device(out, 3 * n_rows * n, True)
        return out

    def event_ms(f):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); f(); b.record(); torch.cuda.synchronize()
        return a.elapsed_time(b)
    o1, o2 = ours(), theirs()
    torch.cuda.synchronize()
    # A.w and B.w must agree byte for byte (the C block differs by construction: A.w o B.w here, the system's C rows there)
    same = all(bool(torch.equal(o1[96 * n_rows * e:96 * n_rows * e + 64 * n_rows], o2.reshape(-1)[96 * n_rows * e:96 * n_rows * e + 64 * n_rows])) for e in range(n))
    del o1, o2
    t_ours, t_theirs = [], []
    for _ in range(args.reps):
        t_ours.append(event_ms(ours)); t_theirs.append(event_ms(theirs))
    best = min(t_ours) * 1e-3
    r_handle = r_host = r_dev = float("nan")
    p_host = p_dev = p_handle = None
    count = args.proofs
    if not args.kernel_only:
        # ---- proofs per second -----------------------------------------------------------------------------------------------------------
        d_in = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to(dev)
        d_status = torch.zeros(n, dtype=torch.int32, device=dev)
        d_scratch = torch.empty(c.scratch_bytes(n), dtype=torch.uint8, device=dev)
        c.prepare_device(d_in, n, d_status, d_scratch)
        torch.cuda.synchronize()
        count = args.proofs
        bl = [(3 + e, 4 + e) for e in range(count)]
        idx = [e % n for e in range(count)]
        host_all = b"".join(host_w[32 * W * e:32 * W * (e + 1)] for e in idx)
        d_all = torch.frombuffer(bytearray(host_all), dtype=torch.uint8).to(dev)

        def rate(f):
            f(); torch.cuda.synchronize(); t = time.time()
            out = f(); torch.cuda.synchronize()
            return count / (time.time() - t), out
        r_handle, p_handle = rate(lambda: pv.prove_batch_bytes(d_in, n, d_scratch, idx, bl, slots=args.slots))
        r_host, p_host = rate(lambda: wp.prove_bytes(host_all, bl))
        r_dev, p_dev = rate(lambda: wp.prove_bytes(d_all, bl))
    out = {"circuit": f"EmailVerifier({N},{M},121,17,0,0,0,0)", "W": W, "rows": n_rows, "terms_A_B": n_terms, "witnesses": n,
           "zk_zkey_abc_ms": [round(x, 3) for x in t_ours], "r1cs_evaluate_plus_convert_ms": [round(x, 3) for x in t_theirs],
           "speedup_best_over_best": round(min(t_theirs) / min(t_ours), 2), "A_B_equal_bytes": same,
           "terms_per_s": round(n_terms * n / best / 1e9, 2), "terms_per_s_unit": "G", "gathered_GBps": round(32 * n_terms * n / best / 1e9, 1),
           "share_of_product_rate_if_every_term_multiplied": round(n_terms * n / best / LAZY_RATE, 4),
           "witnesses_per_lane": os.environ.get("ZKWG_ZKEY_G", "2"),
           "proofs_per_s": None if args.kernel_only else {"handle_path_prepared": round(r_handle, 2), "witnesses_host": round(r_host, 2), "witnesses_device": round(r_dev, 2)},
           "proofs_equal": None if args.kernel_only else {"host_vs_device": p_host == p_dev, "witness_vs_handle": p_host[1] == p_handle},
           "slots": args.slots, "proofs_timed": count, "setup_s": round(t_setup, 1), "witness_prover_create_s": round(t_create, 1),
           "zkey_bytes": len(z), "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "runtime default")}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
