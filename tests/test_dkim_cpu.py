"""DKIM verification of raw emails without a GPU: the parser, the cores of the device = -1 path of
zkwg_dkim_verify_batch, and the bodies of zk_dkim_body / zk_dkim_verify on the simulated wavefront (tests/native/dkimtest.cpp), against
the reference's verdicts (packages/helpers/tests/dkim.test.ts, tests/golden/dkim/dkim_expected.json), the existing fixtures of the two
real emails, and the literal restatement of the reference's canonicalisers (tests/dkim_ref.py)."""
import base64
import hashlib
import os
import random
import struct
import subprocess

import pytest

import dkim_cases as cases
import dkim_ref
import dkimtest
import real_email
from zkwg import _lib, dkim, inputs, synth

HOST = -1
MODES = [("relaxed", dkimtest.RELAXED, dkim_ref.relaxed_body), ("simple", dkimtest.SIMPLE, dkim_ref.simple_body)]


def verify(email, **kw):
    kw.setdefault("keys", cases.keys())
    return dkim.verify_dkim_signature(email, device=HOST, **kw)


# ------------------------------------------------------------------ the verdicts of dkim.test.ts
@pytest.mark.parametrize("case", cases.expected()["verdicts"], ids=lambda c: f"dkim.test.ts:{c['line']}")
def test_verdicts_of_the_reference_suite(case):
    email = cases.eml(case["email"])
    if "replace" in case:
        email = email.decode().replace(*case["replace"], 1).encode()
    kw = dict(domain=case.get("domain", ""), skip_body_hash=case.get("skip_body_hash", False))
    if case.get("no_keys"):
        kw["keys"] = {}
    if "error" in case:
        with pytest.raises(dkim.DkimError) as e:
            verify(email, **kw)
        assert str(e.value) == case["error"]
        return
    res = verify(email, **kw)
    if "signingDomain" in case:
        assert res["signingDomain"] == case["signingDomain"]
    if "appliedSanitization" in case:
        assert res["appliedSanitization"] == case["appliedSanitization"]


def test_result_fields_of_the_two_real_emails():
    for name, which in (("test.eml", "test_eml"), ("email-good-large.eml", "email_good_large")):
        want, res = real_email.dkim_result(which), verify(cases.eml(name))
        for k in ("headers", "body", "bodyHash", "publicKey", "signature"):
            assert res[k] == want[k], (name, k)
        assert (res["signingDomain"], res["selector"], res["algo"], res["format"], res["modulusLength"]) == ("icloud.com", "1a1hai", "rsa-sha256", "relaxed/relaxed", 2048)
        assert res["appliedSanitization"] is None


def test_raw_email_inputs_equal_the_inputs_from_the_dkim_result():
    got = inputs.generate_email_verifier_inputs(cases.eml("test.eml"), {"maxHeadersLength": 640, "maxBodyLength": 768}, keys=cases.keys(), device=HOST)
    want = real_email.ev_inputs()
    assert got.keys() == want.keys()
    for k in want:
        assert got[k] == want[k], k


def test_lengths_and_body_hashes_of_all_ten_emails():
    exp = cases.expected()["emails"]
    assert len(exp) == 10
    for name, e in exp.items():
        for sig in e["signatures"]:
            call = dkim._Call([cases.eml(name)], sig["d"], {}, False, HOST, 1)
            assert call._hlen[0] == sig["header_len"] and call._blen[0] == sig["body_len"], (name, sig["d"])
            assert (base64.b64encode(call.body_digest(0)).decode() == sig["bh"]) == sig["body_sha256_is_bh"], name
            assert call.body_digest(0) == hashlib.sha256(call.body(0)).digest() and call.header_digest(0) == hashlib.sha256(call.header(0)).digest()


def test_lorem_ipsum_and_both_signatures_of_multi_dkim_sig():
    for name, domain in (("lorem_ipsum.eml", ""), ("multi-dkim-sig.eml", "bf01.eu1.hubspotstarter.net"), ("multi-dkim-sig.eml", "starknet.org")):
        call = dkim._Call([cases.eml(name)], domain, cases.keys(), False, HOST, 1)
        assert base64.b64encode(hashlib.sha256(call.body(0)).digest()) == bytes(call._parsed[0].bh_b64), (name, domain)
        assert call.status == [_lib.DKIM_NO_KEY]
        with pytest.raises(dkim.DkimError, match="Reason: no key"):
            verify(cases.eml(name), domain=domain)
    st, _, P = dkim.parse(cases.eml("multi-dkim-sig.eml"))
    assert st == 0 and P.d == b"starknet.org" and P.s == b"hs1-145681388"          # the From domain picks the signature


# ------------------------------------------------------------------ body canonicalisation against tests/dkim_ref.py
def check_body(raw, l=None):
    for name, mode, ref in MODES:
        want = ref(raw, l)
        for wave in (False, True):
            n, fits, row = dkimtest.body(raw, mode, l, wave=wave)
            assert fits == 1 and row[:n] == want, (name, wave, raw, l)
            assert row[n:] == b"\xa5" * (len(row) - n), (name, wave, "a store beyond the canonical length")


def test_tile_size_of_the_cases():
    assert dkimtest.tile() == cases.TILE


def test_random_bodies():
    rng = random.Random(20240607)
    for length in list(range(0, 201)) + [rng.randrange(0, 201) for _ in range(100)]:
        check_body(cases.random_body(rng, length))


@pytest.mark.parametrize("name,raw", cases.boundary_bodies(), ids=[n for n, _ in cases.boundary_bodies()])
def test_boundary_bodies(name, raw):
    check_body(raw)


def test_random_bodies_around_the_tile_boundary():
    rng = random.Random(99)
    T = cases.TILE
    for n in (T - 1, T, T + 1, 2 * T + 1):
        for _ in range(6):
            check_body(cases.random_body(rng, n))


def test_l_tag_at_zero_inside_and_beyond():
    for raw in (b"first line \r\nsecond\tline\r\n\r\n", b"", b"x" * (cases.TILE + 5) + b" \r\ny\r\n"):
        full = len(dkim_ref.relaxed_body(raw)) + 2
        for l in (0, 1, 7, full - 3, full, full + 100):
            check_body(raw, max(l, 0))


def test_a_body_longer_than_its_slot_is_reported_and_nothing_is_stored_past_the_slot():
    raw = b"0123456789 \r\n" * 200
    for name, mode, ref in MODES:
        want = ref(raw)
        for stride in (0, 1, 100, cases.TILE, len(want) - 1):
            rows = []
            for wave in (False, True):
                n, fits, row = dkimtest.body(raw, mode, None, stride=stride, wave=wave)
                assert (n, fits) == (0, 0) and row == want[:stride]
                rows.append(row)
            assert rows[0] == rows[1]
        n, fits, row = dkimtest.body(raw, mode, None, stride=len(want), wave=True)
        assert (n, fits, row) == (len(want), 1, want)
        n, fits, row = dkimtest.body(raw, mode, 50, stride=64, wave=True)                 # l= makes it fit
        assert (n, fits, row[:50]) == (50, 1, want[:50]) and row[50:] == b"\xa5" * 14


def test_stray_cr_is_an_ordinary_byte():
    """The documented rule: a CR that no LF follows is content.  mailauth's fixLineBuffer keeps such a CR too, but lets the
    white space around it collapse across it: this one case pins our rule, where the two differ."""
    raw = b"a\r b\r\n"
    for wave in (False, True):
        n, _, row = dkimtest.body(raw, dkimtest.RELAXED, wave=wave)
        assert row[:n] == b"a\r b\r\n"
    assert dkim_ref.relaxed_body(raw) == b"a \rb\r\n"


# ------------------------------------------------------------------ the parser against tests/dkim_ref.py
def ref_header(raw, domain):
    parsed = dkim_ref.parse_headers(raw[:dkim_ref.body_offset(raw)])
    for key, _, line in parsed:
        if key == "dkim-signature" and f"d={domain};".encode() in line.replace(b" ", b""):
            text = line.decode("latin-1")
            import re
            h = re.search(r"[;\s]h=([^;]*)", re.sub(r"\r?\n", "", text)).group(1)
            c = re.search(r"c=(\w+)", text).group(1)
            return (dkim_ref.relaxed_header if c == "relaxed" else dkim_ref.simple_header)(dkim_ref.signing_lines(parsed, h), line)
    raise AssertionError("no signature")


def test_header_canonicalisation_of_hand_made_messages():
    base = (b"Received: one\r\nSubject: first\r\nFROM:  Someone\r\n\t<a@example.com>  \r\nsUbJeCt:   folded\r\n   over  three\r\n\tlines \r\nTo:x@y.z\r\n"
            b"DKIM-Signature: v=1; a=rsa-sha256; c=%s/relaxed; d=example.com; s=sel;\r\n\tbh=47DEQpj8HBSa+/TImW+5JCeuQeRkm5NMpJWZG3hSuFU=;\r\n"
            b" h=Subject : from:subject:SUBJECT:to:cc; b=AAAA\r\n\tBBBB\r\n CCA=\r\n\r\nbody\r\n")
    for hc in (b"relaxed", b"simple"):
        raw = base % hc
        st, header, P = dkimtest.parse(raw)
        assert st == 0 and header == ref_header(raw, "example.com")
        assert bytes(P.signature)[-8:] == base64.b64decode("AAAABBBBCCA=") and P.signature_len == 8 and P.header_canon == (hc == b"simple")
        assert P.body_offset == raw.index(b"body") and P.body_len == 6
    # the name that h= lists three times takes both Subject fields bottom-up and then nothing; cc has no field
    st, header, _ = dkimtest.parse(base % b"relaxed")
    assert header.startswith(b"subject:folded over three lines\r\nfrom:Someone <a@example.com>\r\nsubject:first\r\nto:x@y.z\r\ndkim-signature:v=1;")
    assert header.endswith(b"b=")
    # LF line ends give the same fields
    assert dkimtest.parse((base % b"relaxed").replace(b"\r\n", b"\n"))[1] == header


def test_parser_statuses():
    good = cases.signed_email(b"x\r\n")
    assert dkimtest.parse(good)[0] == 0
    assert dkimtest.parse(good.replace(b" h=From:Subject:To;", b""))[0] == _lib.DKIM_UNSUPPORTED                  # a tag list without h=
    assert dkimtest.parse(cases.signed_email(b"x\r\n", l=5).replace(b" l=5;", b" l=5x;"))[0] == _lib.DKIM_UNSUPPORTED
    assert dkimtest.parse(good.replace(b"b=", b"b=" + b"QUFB" * 100))[0] == _lib.DKIM_UNSUPPORTED                 # b= of more than 256 bytes
    assert dkimtest.parse(good.replace(b"bh=", b"bh=!"))[0] == _lib.DKIM_UNSUPPORTED
    assert dkimtest.parse(good, header_cap=32)[0] == _lib.DKIM_UNSUPPORTED
    assert dkimtest.parse(good, domain="other.org")[0] == _lib.DKIM_NOT_FOUND
    assert dkimtest.parse(b"")[0] == _lib.DKIM_NOT_FOUND and dkimtest.parse(b"no header at all")[0] == _lib.DKIM_NOT_FOUND
    arc = good.replace(b"DKIM-Signature:", b"ARC-Message-Signature:")
    assert dkimtest.parse(arc)[0] == _lib.DKIM_NOT_FOUND                                                          # ARC-* fields are ignored
    st, _, P = dkimtest.parse(b"From: a@b.c\r\n\r\n")
    assert st == _lib.DKIM_NOT_FOUND and P.d == b"b.c" and P.body_len == 0


# ------------------------------------------------------------------ signed here: all four c=, key sizes, several keys
@pytest.mark.parametrize("canon", ["relaxed/relaxed", "relaxed/simple", "simple/relaxed", "simple/simple"])
def test_all_four_canonicalisations_verify(canon):
    for i, body_len in enumerate((10, 90, 1500)):
        raw = synth.synthetic_raw_email(5, i, body_len, canon)
        res = verify(raw)
        assert res["format"] == canon and res["publicKey"] == synth.test_key()["n"]
        if canon == "relaxed/relaxed":
            want = synth.synthetic_dkim_result(5, i, body_len)
            assert {k: res[k] for k in want} == want
    raw = synth.synthetic_raw_email(5, 9, 400, canon, l=120)
    assert len(verify(raw)["body"]) == 120
    with pytest.raises(dkim.DkimError, match="Reason: bad signature"):
        verify(raw.replace(b"recipient@example.org", b"recipienT@example.org"), enable_sanitization=False)
    with pytest.raises(dkim.DkimError, match="Reason: body hash did not verify"):
        at = raw.index(b"\r\n\r\n") + 4                                   # (the first body byte: l= covers it)
        verify(raw[:at] + bytes([raw[at] ^ 1]) + raw[at + 1:])


def small_key(bits, seed):
    """an RSA key of `bits` bits with e = 65537 from a seeded generator (Miller-Rabin)"""
    rng = random.Random(seed)

    def prime(b):
        while True:
            p = rng.getrandbits(b) | (3 << (b - 2)) | 1
            if all(p % q for q in (3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)) and all(pow(a, p - 1, p) == 1 for a in (2, 3, 5, 7)) and (p - 1) % 65537:
                return p
    p, q = prime(bits // 2), prime(bits // 2)
    n, d = p * q, pow(65537, -1, (p - 1) * (q - 1))
    return {"n": n, "d": d, "p": p, "q": q, "e": 65537, "dp": d % (p - 1), "dq": d % (q - 1), "qinv": pow(q, -1, p)}


def test_a_1024_bit_key_passes():
    key = small_key(1024, 1)
    assert key["n"].bit_length() == 1024
    raw = cases.signed_email(b"short key\r\n", key=key, s="k1024")
    res = verify(raw, keys={"k1024._domainkey.example.com": [dkim.txt_record(key["n"])]})
    assert res["modulusLength"] == 1024 and res["publicKey"] == key["n"]
    digest = hashlib.sha256(res["headers"]).digest()
    for wave in (False, True):
        assert dkimtest.rsa(key["n"], res["signature"], digest, wave=wave) == 1
        assert dkimtest.rsa(key["n"], res["signature"] ^ 1, digest, wave=wave) == 0


def test_the_right_key_in_third_place():
    others = [small_key(1024, 2)["n"], synth.test_key()["n"] + 2]
    raw = cases.signed_email(b"three keys\r\n")
    recs = [dkim.txt_record(others[0]), "v=DKIM1; k=ed25519; p=11qYAYKxCrfVS/7TyWQHOg7hcvPapiMlrwIaaPcHURo=", dkim.txt_record(others[1]), dkim.txt_record(synth.test_key()["n"])]
    call = dkim._Call([raw], "", {"sel._domainkey.example.com": recs}, False, HOST, 1)
    assert call.status == [0] and call.key_index == [2]                     # (the ed25519 record is no RSA key: not a candidate)
    assert call.outcome(0)["publicKey"] == synth.test_key()["n"]
    unusable = {"sel._domainkey.example.com": [dkim.txt_record(synth.test_key()["n"], 3), dkim.txt_record((1 << 3000) + 1)]}
    with pytest.raises(dkim.DkimError, match="Reason: unsupported"):
        verify(raw, keys=unusable)


def test_the_rsa_cores_agree_and_refuse_what_they_must():
    d = synth.synthetic_dkim_result(3, 0, 100)
    digest = hashlib.sha256(d["headers"]).digest()
    n = d["publicKey"]
    for wave in (False, True):
        assert dkimtest.rsa(n, d["signature"], digest, wave=wave) == 1
        assert dkimtest.rsa(n, d["signature"], hashlib.sha256(b"other").digest(), wave=wave) == 0
        assert dkimtest.rsa(n, n, digest, wave=wave) == 0                           # s >= n
        assert dkimtest.rsa(n, (1 << 2048) - 1, digest, wave=wave) == 0
        assert dkimtest.rsa(n + 1, d["signature"], digest, wave=wave) == 0          # an even modulus
        assert dkimtest.rsa(n >> 1030, d["signature"] % (n >> 1030), digest, wave=wave) == 0   # fewer than 1024 bits


def test_sha256_core():
    rng = random.Random(4)
    for n in (0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 128, 1000):
        data = bytes(rng.randrange(256) for _ in range(n))
        assert dkimtest.sha256(data) == hashlib.sha256(data).digest()


# ------------------------------------------------------------------ malformed input
def malformed_corpus():
    rng = random.Random(6376)
    base = cases.eml("test.eml")
    out = [b"", b"\n", b"\r\n\r\n", b":", b"DKIM-Signature:", b"DKIM-Signature: b=;;;=;bh", base[:1], b"From: <\r\n\r\n", b"From: \"a\\\r\n\r\n", b"From: (((\r\n\r\nx"]
    for _ in range(150):
        out.append(base[:rng.randrange(len(base))])
    for _ in range(250):
        m = bytearray(base)
        for _ in range(rng.choice((1, 1, 2, 8))):
            m[rng.randrange(len(m))] ^= 1 << rng.randrange(8)
        out.append(bytes(m))
    return out


def test_malformed_messages_get_a_status():
    corpus = malformed_corpus()
    res = dkim.verify_batch(corpus, keys=cases.keys(), device=HOST, enable_sanitization=False)
    known = {_lib.DKIM_NOT_FOUND, _lib.DKIM_MULTIPLE_FROM, _lib.DKIM_NO_KEY, _lib.DKIM_BODY_HASH, _lib.DKIM_BAD_SIGNATURE, _lib.DKIM_UNSUPPORTED}
    assert len(res) == len(corpus)
    for r in res:
        assert isinstance(r, dict) or r.status in known
    assert sum(isinstance(r, dict) for r in res) < len(corpus) // 4                  # a flipped bit is noticed


def test_malformed_messages_under_the_sanitisers(tmp_path):
    """the stand-alone build of tests/native/dkimtest.cpp with -fsanitize=address,undefined takes the same corpus: every message sits in
    a heap block of exactly its length"""
    corpus = malformed_corpus()
    path = tmp_path / "corpus.bin"
    path.write_bytes(struct.pack("<I", len(corpus)) + b"".join(struct.pack("<I", len(m)) + m for m in corpus))
    prog = dkimtest.build_sanitized_program(str(tmp_path / "dkimtest_asan"))
    p = subprocess.run([prog, str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    assert f"{len(corpus)} messages" in p.stdout


def test_command_line_on_the_host(tmp_path, capsys):
    keys = tmp_path / "keys.json"
    import json
    keys.write_text(json.dumps(cases.keys()))
    files = [os.path.join(cases.GOLDEN, n) for n in ("test.eml", "email-body-tampered.eml")]
    assert dkim.main(["verify", files[0], "--keys", str(keys), "--device", "-1"]) == 0
    assert dkim.main(["verify", *files, "--keys", str(keys), "--device", "-1"]) == 1
    out = capsys.readouterr().out.splitlines()
    assert out[0].endswith("test.eml: pass d=icloud.com s=1a1hai a=rsa-sha256 bits=2048") and "FAIL" in out[2] and "body hash did not verify" in out[2]


def test_batch_parse_gives_the_names_and_a_stride_that_always_fits():
    import ctypes as C
    emails = [cases.signed_email(b, canon) for _, b in cases.boundary_bodies() for canon in ("relaxed/relaxed", "relaxed/simple")] + [cases.eml("email-invalid-domain.eml"), b""]
    n = len(emails)
    out = (_lib.DkimParsed * n)()
    rc = _lib.load().zkwg_dkim_parse_batch(n, (C.c_char_p * n)(*emails), (C.c_uint64 * n)(*map(len, emails)), None, 3, out)
    assert rc == 0 and [out[n - 2].status, out[n - 1].status] == [_lib.DKIM_NOT_FOUND] * 2
    for e, P in zip(emails[:-2], out):
        one = dkim.parse(e)[2]
        assert (P.status, P.s, P.d, P.header_len, P.body_offset, P.body_len) == (0, b"sel", b"example.com", one.header_len, one.body_offset, one.body_len)
        body = e[P.body_offset:]
        assert P.body_bound == len(body) + body.count(b"\n") - body.count(b"\r\n") + 2
        assert P.body_bound >= max(len(dkim_ref.relaxed_body(body)), len(dkim_ref.simple_body(body)))
