"""`python -m zkwg.generate_witness <circuit> <input.json> <witness.wtns> [device]` -- counterpart of circom's
generated `generate_witness.js` as the reference documents it (docs/zk-email-docs/UsageGuide/README.md:132-140:
`node generate_witness.js circuit.wasm input.json witness.wtns`).  <circuit> names the circuit by its template
parameters instead of a WASM file: `EmailVerifier(1024,1536,121,17,0,0,0,0)`, `CleanEmailAddress(32)` or a JSON object / file with the
keyword arguments of zkwg.Circuit.  An input file holding a list writes <witness>_<i>.wtns per email and exits 1
if any email failed.  `--eml`: <input> is a raw email; it is verified first (zkwg.dkim, keys from `--keys keys.json`:
name -> TXT records) and its inputs are generated for the circuit's sizes (zkwg.inputs.generate_email_verifier_inputs)."""
import json
import os
import re
import sys

import zkwg


def circuit_kwargs(arg):
    m = re.fullmatch(r"\s*EmailVerifier\(([\d\s,]+)\)\s*", arg)
    if m:
        p = [int(x) for x in m.group(1).split(",")]
        if len(p) != 8:
            raise SystemExit("EmailVerifier takes 8 parameters")
        return dict(main_kind=zkwg.MAIN_EMAIL_VERIFIER, max_header=p[0], max_body=p[1], n=p[2], k=p[3],
                    ignore_body_hash_check=p[4], enable_header_masking=p[5], enable_body_masking=p[6],
                    remove_soft_line_breaks=p[7])
    m = re.fullmatch(r"\s*RevealSubstring\(\s*(\d+)\s*,\s*(\d+)\s*,\s*([01])\s*\)\s*", arg)
    if m:   # helpers/reveal-substring.circom:13
        return dict(main_kind=zkwg.MAIN_REVEAL_SUBSTRING, max_header=int(m.group(1)), max_body=int(m.group(2)), n=int(m.group(3)), k=0)
    m = re.fullmatch(r"\s*CountSubstringOccurrences\(\s*(\d+)\s*,\s*(\d+)\s*\)\s*", arg)
    if m:   # utils/array.circom:226
        return dict(main_kind=zkwg.MAIN_COUNT_SUBSTRING, max_header=int(m.group(1)), max_body=int(m.group(2)), n=0, k=0)
    m = re.fullmatch(r"\s*CleanEmailAddress\(\s*(\d+)\s*\)\s*", arg)
    if m:   # utils/email.circom:16
        return dict(main_kind=zkwg.MAIN_CLEAN_EMAIL_ADDRESS, max_header=int(m.group(1)), max_body=int(m.group(1)), n=0, k=0)
    m = re.fullmatch(r"\s*EmailReveal\(([\d\s,]+)\)\s*", arg)
    if m:   # circuits/email-reveal.circom
        p = [int(x) for x in m.group(1).split(",")]
        if len(p) != 9:
            raise SystemExit("EmailReveal takes 9 parameters")
        return dict(main_kind=zkwg.MAIN_EMAIL_REVEAL, max_header=p[0], max_body=p[1], n=p[2], k=p[3], ignore_body_hash_check=p[4],
                    reveal_from_body=p[5], max_substring=p[6], check_uniqueness=p[7], with_nullifier=p[8])
    text = open(arg).read() if os.path.exists(arg) else arg
    kw = json.loads(text)
    base = os.path.dirname(arg) if os.path.exists(arg) else "."
    if isinstance(kw.get("sym"), str) and os.path.exists(os.path.join(base, kw["sym"])):
        kw["sym"] = open(os.path.join(base, kw["sym"])).read()
    if isinstance(kw.get("r1cs"), str):
        kw["r1cs"] = open(os.path.join(base, kw["r1cs"]), "rb").read()
    return kw


def main(argv=None):
    a = list(sys.argv[1:] if argv is None else argv)
    eml = "--eml" in a
    keys = {}
    if eml:
        a.remove("--eml")
    if "--keys" in a:
        keys = json.load(open(a.pop(a.index("--keys") + 1)))
        a.remove("--keys")
    if len(a) < 3:
        print("Usage: python -m zkwg.generate_witness <circuit> <input.json | --eml email.eml --keys keys.json> <witness.wtns> [device]", file=sys.stderr)
        return 2
    c = zkwg.Circuit(device=int(a[3]) if len(a) > 3 else 0, **circuit_kwargs(a[0]))
    if eml:
        from zkwg import inputs
        keys = {k: [v] if isinstance(v, str) else v for k, v in keys.items()}
        inp = inputs.generate_email_verifier_inputs(open(a[1], "rb").read(), {
            "maxHeadersLength": c.cfg.max_header, "maxBodyLength": c.cfg.max_body, "ignoreBodyHashCheck": bool(c.cfg.ignore_body_hash_check),
            "removeSoftLineBreaks": bool(c.cfg.remove_soft_line_breaks)}, keys=keys, device=c.device)
    else:
        inp = json.load(open(a[1]))
    many = isinstance(inp, list)
    wits, status = c.calculate_batch_host(b"".join(c.pack(x) for x in (inp if many else [inp])))
    wb = c.witness_bytes
    stem = re.sub(r"\.wtns$", "", a[2])
    failed = 0
    for i, st in enumerate(status):
        if st != 0:
            print(f"email {i}: Error: Assert Failed (status {st})", file=sys.stderr)
            failed += 1
            continue
        with open(f"{stem}_{i}.wtns" if many else a[2], "wb") as f:
            f.write(c.wtns(wits[i * wb:(i + 1) * wb]))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
