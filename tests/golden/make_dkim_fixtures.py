"""Regenerates tests/golden/dkim/: the reference's ten signed .eml files (data, 65 KB together) and dkim_expected.json -- the verdict
strings of packages/helpers/tests/dkim.test.ts with their line numbers, and per email the lengths of its canonical body and of its
canonical signed header, computed with the literal restatement of the reference's canonicalisers (tests/dkim_ref.py).

    python tests/golden/make_dkim_fixtures.py [/path/to/zk-email-verify]

Needs the reference tree; the tests read only what this leaves under tests/golden/dkim/."""
import base64
import hashlib
import json
import os
import re
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dkim_ref  # noqa: E402

FILES = [("packages/helpers/tests/test-data", n) for n in (
    "email-good.eml", "email-good-large.eml", "email-bodyless.eml", "email-body-tampered.eml", "email-different-domain.eml",
    "email-invalid-domain.eml", "email-invalid-selector.eml", "multi-dkim-sig.eml")] + [
    ("packages/circuits/tests/test-emails", n) for n in ("test.eml", "lorem_ipsum.eml")]

# packages/helpers/tests/dkim.test.ts: what each case expects (the message of the thrown error, or the fields of the result)
VERDICTS = [
    {"line": "10-17", "email": "email-good.eml", "pass": True, "signingDomain": "icloud.com", "appliedSanitization": None},
    {"line": "19-29", "email": "email-invalid-selector.eml", "error": "DKIM signature verification failed for domain icloud.com. Reason: no key"},
    {"line": "31-43", "email": "email-body-tampered.eml", "error": "DKIM signature verification failed for domain icloud.com. Reason: body hash did not verify"},
    {"line": "45-56", "email": "email-invalid-domain.eml", "error": "DKIM signature not found for domain gmail.com"},
    {"line": "58-63", "email": "email-different-domain.eml", "pass": True},
    {"line": "65-73", "email": "email-different-domain.eml", "domain": "domain.com", "error": "DKIM signature not found for domain domain.com"},
    {"line": "76-84", "email": "email-bodyless.eml", "skip_body_hash": True, "pass": True, "signingDomain": "icloud.com"},
    {"line": "200-210", "email": "email-good.eml", "replace": ["Subject: ", "Subject: [EmailListABC]"], "pass": True, "appliedSanitization": "removeLabels"},
    {"line": "161-176", "email": "email-good.eml", "no_keys": True, "error": "DKIM signature verification failed for domain icloud.com. Reason: no key"},
]


def signatures(raw):
    """every DKIM-Signature of a message -> [(d, canonical body, canonical header, bh)]"""
    off = dkim_ref.body_offset(raw)
    parsed = dkim_ref.parse_headers(raw[:off])
    out = []
    for key, _, line in parsed:
        if key != "dkim-signature":
            continue
        text = re.sub(r"\s+", "", line.decode("latin-1").split(":", 1)[1])
        tags = dict(t.split("=", 1) for t in text.split(";") if "=" in t)
        hc, _, bc = tags.get("c", "simple/simple").partition("/")
        body = (dkim_ref.relaxed_body if (bc or "simple") == "relaxed" else dkim_ref.simple_body)(raw[off:], int(tags["l"]) if "l" in tags else None)
        # h= keeps its colons: take it from the unfolded field, not from the tag text above
        h = re.search(r"[;\s]h=([^;]*)", re.sub(r"\r?\n", "", line.decode("latin-1"))).group(1)
        lines = dkim_ref.signing_lines(parsed, h)
        header = (dkim_ref.relaxed_header if hc == "relaxed" else dkim_ref.simple_header)(lines, line)
        out.append((tags["d"], body, header, tags["bh"]))
    return out


def main(ref):
    out_dir = os.path.join(HERE, "dkim")
    os.makedirs(out_dir, exist_ok=True)
    emails = {}
    for d, name in FILES:
        shutil.copyfile(os.path.join(ref, d, name), os.path.join(out_dir, name))
        os.chmod(os.path.join(out_dir, name), 0o644)
        raw = open(os.path.join(out_dir, name), "rb").read()
        emails[name] = {"source": f"{d}/{name}", "signatures": [
            {"d": dom, "body_len": len(body), "header_len": len(header), "bh": bh,
             "body_sha256_is_bh": base64.b64encode(hashlib.sha256(body).digest()).decode() == bh}
            for dom, body, header, bh in signatures(raw)]}
    json.dump({"source": "packages/helpers/tests/dkim.test.ts", "verdicts": VERDICTS, "emails": emails},
              open(os.path.join(out_dir, "dkim_expected.json"), "w"), indent=1)
    for name, e in emails.items():
        print(name, [(s["d"], s["body_len"], s["header_len"], s["body_sha256_is_bh"]) for s in e["signatures"]])


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
