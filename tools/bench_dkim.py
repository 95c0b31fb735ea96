#!/usr/bin/env python3
"""Times DKIM verification of raw emails (zkwg.dkim -> zkwg_dkim_verify_batch): n messages signed here with the synthetic
key, relaxed/relaxed, whose raw bodies need work (doubled blanks, trailing white space, a bare LF in every fourth line) and whose
canonical form is known by construction.  For every body size: the device path (its parser and the packing of the bodies on --threads host threads), then the same cores on the host
(device = -1) on one thread and on --threads, in the same run; one warm-up call, then --reps timed calls each; medians, every run listed.  Reported per path:
the seconds of the C call (zkwg_dkim_verify_batch), emails/s and raw body bytes/s from it, the seconds of the whole Python entry
(what zkwg.dkim.verify_batch_device does: the threaded parse for the key names, the key look-up, the buffers, then that C call), the six stages the call reports (parse, upload, zk_dkim_body,
zk_dkim_hash, zk_dkim_verify, download) and the parser's own time per email; and once, on the device, a batch that alternates the two
smallest sizes (what ragged lengths cost the one-lane-per-stream hash).  The canonical bodies stay where they are computed (no copy
back to the caller), as in verify_batch_device.  The verdicts are CHECKED (every message passes; exits non-zero otherwise).  No ratio is
gated.  Prints one JSON line.

    python tools/bench_dkim.py [--n 4096] [--sizes 1024 65536 1048576] [--reps 5] [--threads 16] > profiles/r15/r15_a_bench_dkim.json
"""
import argparse
import base64
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zk-email-verify_amd", "py"))

STAGES = ("parse", "upload", "zk_dkim_body", "zk_dkim_hash", "zk_dkim_verify", "download")
CANON_LINE = b"the quick brown fox jumps over the lazy dog 0123456789 abcdefghijklmnopq\r\n"      # 75 bytes
RAW_LINES = [CANON_LINE.replace(b" fox ", b"  fox\t").replace(b"\r\n", b" \t\r\n"), CANON_LINE.replace(b" dog ", b" \t dog  "),
             CANON_LINE.replace(b"\r\n", b"  \r\n"), CANON_LINE.replace(b"\r\n", b"\n")]


def make_email(synth, i, size):
    """-> raw message whose raw body has about `size` bytes"""
    head = b"message %08d\r\n" % i
    k = max(0, (size - len(head)) // 78)
    raw_body = head + b"".join(RAW_LINES[j & 3] for j in range(k)) + b"\r\n \r\n"
    canon_body = head + CANON_LINE * k
    bh = base64.b64encode(hashlib.sha256(canon_body).digest()).decode()
    sig_text = f"v=1; a=rsa-sha256; c=relaxed/relaxed; d=example.com; s=sel; bh={bh}; h=from:subject:to; b="
    header = (f"from:Bench <bench{i}@example.com>\r\nsubject:message {i}\r\nto:someone@example.org\r\ndkim-signature:" + sig_text).encode()
    key = synth.test_key()
    b64 = base64.b64encode(synth.pkcs1_sign_digest(key, hashlib.sha256(header).digest()).to_bytes(256, "big")).decode()
    return (f"DKIM-Signature: {sig_text}{b64[:64]}\r\n\t{b64[64:]}\r\nFrom: Bench <bench{i}@example.com>\r\nSubject:  message {i} \r\n"
            f"To: someone@example.org\r\n\r\n").encode() + raw_body, len(raw_body)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1024, 65536, 1048576])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--ragged", type=int, default=1, help="also time a batch that alternates the two smallest sizes (N=1)")
    a = ap.parse_args(argv)
    from zkwg import dkim, synth
    keys = {"sel._domainkey.example.com": [dkim.txt_record(synth.test_key()["n"])]}
    out = {"tool": "bench_dkim", "n": a.n, "reps": a.reps, "threads": a.threads, "sizes": []}
    ok = True
    for size in a.sizes:
        made = [make_email(synth, i, size) for i in range(a.n)]
        emails, raw_bytes = [m for m, _ in made], sum(b for _, b in made)
        rec = {"body_bytes_per_email": raw_bytes // a.n, "raw_body_bytes": raw_bytes, "paths": {}}
        for label, device, threads in (("device", a.device, a.threads), ("host_1_thread", -1, 1), (f"host_{a.threads}_threads", -1, a.threads)):
            runs = []
            for rep in range(a.reps + 1):
                call = dkim._Call(emails, "", keys, False, device, threads, want_bodies=False, timed=True)
                if call.status != [0] * a.n:
                    ok = False
                if rep:                                   # (the first call is the warm-up)
                    runs.append({"seconds": call.call_seconds, "python_seconds": call.total_seconds, "stages": dict(zip(STAGES, call.seconds))})
                del call
            med = statistics.median(r["seconds"] for r in runs)
            pmed = statistics.median(r["python_seconds"] for r in runs)
            rec["paths"][label] = {
                "python_median_seconds": pmed, "python_emails_per_s": a.n / pmed,
                "median_seconds": med, "emails_per_s": a.n / med, "body_bytes_per_s": raw_bytes / med,
                "median_stage_seconds": {s: statistics.median(r["stages"][s] for r in runs) for s in STAGES},
                "parser_us_per_email_times_threads": statistics.median(r["stages"]["parse"] for r in runs) / a.n * 1e6 * threads, "host_threads": threads,
                "runs": runs}
        out["sizes"].append(rec)
        del made, emails
    if a.ragged and len(a.sizes) >= 2:
        # ragged lengths: the two smallest sizes alternating in one batch, device path only.  zk_dkim_hash maps one lane to one stream, so
        # a wavefront runs as long as its longest stream; without that waste its time would be the mean of the two uniform batches'
        lo, hi = sorted(a.sizes)[:2]
        emails = [make_email(synth, i, hi if i & 1 else lo)[0] for i in range(a.n)]
        runs = []
        for rep in range(a.reps + 1):
            call = dkim._Call(emails, "", keys, False, a.device, a.threads, want_bodies=False, timed=True)
            ok = ok and call.status == [0] * a.n
            if rep:
                runs.append(dict(zip(STAGES, call.seconds)))
        uniform = {r["body_bytes_per_email"]: r["paths"]["device"]["median_stage_seconds"] for r in out["sizes"]}
        med = {s: statistics.median(r[s] for r in runs) for s in STAGES}
        mean_of_uniform = {s: statistics.mean(v[s] for v in list(uniform.values())[:2]) for s in ("zk_dkim_body", "zk_dkim_hash")}
        out["ragged"] = {"sizes_alternating": [lo, hi], "median_stage_seconds": med, "mean_of_the_two_uniform_batches": mean_of_uniform,
                         "hash_time_over_that_mean": med["zk_dkim_hash"] / mean_of_uniform["zk_dkim_hash"], "runs": runs}
    out["verdicts_ok"] = ok
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
