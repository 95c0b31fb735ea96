"""Test-only: the messages and keys that tests/test_dkim_cpu.py and tests/test_dkim_gpu.py share -- the reference's .eml files
(tests/golden/dkim), messages signed here with the synthetic key over the canonical forms of tests/dkim_ref.py, the bodies that sit on
the tile boundaries of zk_dkim_body, and one message per failure kind."""
import base64
import hashlib
import json
import os
import random

import dkim_ref
import real_email
from zkwg import dkim, synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "dkim")
TILE = 1024                     # ZK_DKIM_TILE (tests/test_dkim_cpu.py checks it against the library)
_cache = {}


def eml(name):
    if name not in _cache:
        _cache[name] = open(os.path.join(GOLDEN, name), "rb").read()
    return _cache[name]


def expected():
    if "expected" not in _cache:
        _cache["expected"] = json.load(open(os.path.join(GOLDEN, "dkim_expected.json")))
    return _cache["expected"]


def keys():
    """selector._domainkey.domain -> TXT records: the icloud key of the reference's emails, wrapped here, and the synthetic key"""
    return {"1a1hai._domainkey.icloud.com": [dkim.txt_record(real_email.icloud_modulus())],
            "sel._domainkey.example.com": [dkim.txt_record(synth.test_key()["n"])]}


def canonical_body(raw_body, mode, l=None):
    return (dkim_ref.relaxed_body if mode == "relaxed" else dkim_ref.simple_body)(raw_body, l)


def signed_email(raw_body, canon="relaxed/relaxed", key=None, l=None, d="example.com", s="sel", a="rsa-sha256", bh=None, subject="boundary"):
    """a message around raw_body, signed over the reference's canonical forms (tests/dkim_ref.py)"""
    key = key or synth.test_key()
    hc, bc = canon.split("/")
    if bh is None:
        bh = base64.b64encode(hashlib.sha256(canonical_body(raw_body, bc, l)).digest()).decode()
    fields = [b"From: Case <case@example.com>", b"Subject:  " + subject.encode() + b" ", b"To: someone@example.org,\r\n\tother@example.org"]
    sig = f"DKIM-Signature: v=1; a={a}; c={canon}; d={d}; s={s};\r\n bh={bh};{'' if l is None else f' l={l};'} h=From:Subject:To; b=".encode()
    parsed = dkim_ref.parse_headers(b"\r\n".join(fields + [sig]))
    lines = dkim_ref.signing_lines(parsed, "From:Subject:To")
    header = (dkim_ref.relaxed_header if hc == "relaxed" else dkim_ref.simple_header)(lines, sig)
    value = synth.pkcs1_sign_digest(key, hashlib.sha256(header).digest())
    b64 = base64.b64encode(value.to_bytes((key["n"].bit_length() + 7) // 8, "big"))
    return b"\r\n".join([sig + b64[:70] + b"\r\n\t" + b64[70:]] + fields) + b"\r\n\r\n" + raw_body


def boundary_bodies():
    """(name, raw body): what can go wrong at the edges of a 1024-byte tile and of a lane's 16 bytes"""
    T = TILE
    x = lambda n: (b"abcdefghijklmnopqrstuvwxyz" * (n // 26 + 1))[:n]
    out = [
        ("empty", b""),
        ("one byte", b"a"),
        ("line ends only", b"\r\n\n\r\n\r\n"),
        ("white space only", b" \t  \t"),
        ("white space and line ends", b" \r\n\t\r\n  \n"),
        ("WSP run across the tile boundary", x(T - 3) + b" \t \t  " + b"tail\r\n"),
        ("WSP run that ends the tile", x(T - 4) + b"    " + b"tail\r\n"),
        ("CR last in the tile, LF first in the next", x(T - 1) + b"\r\nnext line\r\n"),
        ("CR LF just inside the tile", x(T - 2) + b"\r\nnext\r\n"),
        ("trailing empty lines across the boundary", x(T - 5) + b"\r\n" * 9),
        ("trailing empty lines fill a tile of their own", x(T - 2) + b"\r\n" + b"\r\n" * (T // 2)),
        ("empty lines across the boundary, then content", x(T - 6) + b"\r\n" * 7 + b"more\r\n"),
        ("bare LFs around the boundary", x(T - 2) + b"\n\n\nx\ny"),
        ("no line end at all", x(2 * T + 1)),
        ("a space before the last byte of the tile", x(T - 2) + b" z" + b"w\r\n"),
        ("lane boundary: SP at byte 15, text at 16", x(15) + b" " + b"q\r\n"),
        ("lane boundary: CR at byte 15, LF at 16", x(15) + b"\r\n" + b"q\r\n"),
    ]
    for n in (15, 16, 17, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1):
        out.append((f"{n} letters", x(n)))
        out.append((f"{n} bytes of lines", (b"line of text \r\n" * (n // 15 + 1))[:n]))
    return out


def random_body(rng, n):
    """over {letters, SP, TAB, CRLF, bare LF}"""
    out = bytearray()
    while len(out) < n:
        out += rng.choice([b"a", b"b", b"Z", b"q", b" ", b" ", b"\t", b"\r\n", b"\n"])
    return bytes(out[:n]) if not out[:n].endswith(b"\r") else bytes(out[:n - 1]) + b"x"


def failure_emails():
    """(what, message, the status it gets with keys()) -- one per failure kind"""
    L = dkim._lib
    good = signed_email(b"fine\r\n")
    two_from = good.replace(b"From: Case <case@example.com>", b"From: Case <case@example.com>, Other <other@elsewhere.org>")
    return [
        ("not found", eml("email-invalid-domain.eml"), L.DKIM_NOT_FOUND),
        ("multiple From", two_from, L.DKIM_MULTIPLE_FROM),
        ("no key", eml("email-invalid-selector.eml"), L.DKIM_NO_KEY),
        ("body hash", eml("email-body-tampered.eml"), L.DKIM_BODY_HASH),
        ("bad signature", good.replace(b"Subject:  boundary", b"Subject:  tampered"), L.DKIM_BAD_SIGNATURE),
        ("unsupported algorithm", signed_email(b"fine\r\n", a="rsa-sha1"), L.DKIM_UNSUPPORTED),
    ]


def mixed_batch(n, seed=7):
    """n messages: the reference's emails, synthetic ones of all four c= modes, the boundary bodies in both body modes, every failure
    kind -> [(message, expected status or None when the verdict is left to the comparison)]"""
    rng = random.Random(seed)
    pool = [(eml(name), 0) for name in ("test.eml", "email-good-large.eml", "email-different-domain.eml")]
    pool += [(eml("lorem_ipsum.eml"), dkim._lib.DKIM_NO_KEY), (eml("multi-dkim-sig.eml"), dkim._lib.DKIM_NO_KEY)]
    for i, canon in enumerate(("relaxed/relaxed", "relaxed/simple", "simple/relaxed", "simple/simple")):
        pool.append((synth.synthetic_raw_email(seed, i, 300 + 97 * i, canon), 0))
    pool += [(m, st) for _, m, st in failure_emails()]
    for i, (_, body) in enumerate(boundary_bodies()):
        pool.append((signed_email(body, "relaxed/relaxed" if i % 2 == 0 else "relaxed/simple"), 0))
    for i in range(8):
        body = random_body(rng, rng.randrange(0, 200))
        pool.append((signed_email(body, rng.choice(["relaxed/relaxed", "simple/simple"]), l=rng.choice([None, None, 0, 5, 1000])), 0))
    if n <= len(pool):
        # small batches: always a real email first, then a spread over the pool
        step = max(1, len(pool) // n)
        return [pool[0]] + [pool[(1 + i * step) % len(pool)] for i in range(n - 1)]
    return [pool[i % len(pool)] for i in range(n)]
