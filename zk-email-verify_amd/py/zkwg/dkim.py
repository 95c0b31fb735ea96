"""DKIM verification of raw emails, batched: `verifyDKIMSignature` of the reference
(packages/helpers/src/dkim/index.ts:36-97) over zkwg_dkim_verify_batch.  The host parses the messages and canonicalises the signed
headers; the device canonicalises the bodies, hashes and checks bh= and the RSA signature against every candidate key.

  verify_dkim_signature(email, ...)   one message -> the reference's DKIMVerificationResult as a dict, or DkimError with its message
  verify_batch(emails, ...)           a list of messages -> per message the dict or the DkimError; one device call for the batch and
                                      one more for the sanitised retries of the messages with a bad signature
  verify_batch_device(emails, ...)    the same verdicts, with the filled zkwg_dkim_batch left on the device: the handle goes to
                                      zkwg.generate_inputs_device in place of the list of dicts

There is no DNS here: `keys` maps `selector._domainkey.domain` to the TXT records of that name (`v=DKIM1; k=rsa; p=...`), or is a
callable name -> list of records.  Out of scope: resolvers, ed25519 and rsa-sha1, ARC sealing, the x= expiry policy.

`python -m zkwg.dkim verify FILE.eml... --key NAME=TXT | --keys keys.json [--domain D] [--skip-body-hash] [--device D]` prints one
line per message and exits 0 when every one passed, else 1.
"""
import base64
import ctypes as C
import json
import re
import sys

from . import _lib
from ._lib import DkimBatch, DkimKey, DkimParsed, DkimVerifyArgs

HEADER_CAP = 1 << 16


class DkimError(Exception):
    def __init__(self, message, status=None):
        super().__init__(message)
        self.status = status


def _check(rc):
    if rc < 0:
        lib = _lib.load()
        raise RuntimeError(f"{lib.zkwg_strerror(rc).decode()} ({lib.zkwg_last_error().decode()})")


# ---------------------------------------------------------------------------------------------- keys
def _der(buf, pos):
    """one DER element at pos -> (tag, content start, content end)"""
    tag = buf[pos]
    ln = buf[pos + 1]
    pos += 2
    if ln & 0x80:
        k = ln & 0x7F
        if k == 0 or k > 4:
            raise ValueError("DER length")
        ln = int.from_bytes(buf[pos:pos + k], "big")
        pos += k
    if pos + ln > len(buf):
        raise ValueError("DER element beyond the buffer")
    return tag, pos, pos + ln


def parse_txt_key(txt):
    """a DKIM TXT record -> (modulus, its bit length, exponent), or None when it is no RSA key (k= other than rsa, empty or broken p=).
    p= is a SubjectPublicKeyInfo in base64 (RFC 6376 3.6.1); a bare RSAPublicKey is taken too."""
    tags = {}
    for part in txt.split(";"):
        k, eq, v = part.partition("=")
        if eq:
            tags[k.strip().lower()] = re.sub(r"\s+", "", v)
    if tags.get("k", "rsa").lower() != "rsa" or not tags.get("p"):
        return None
    try:
        der = base64.b64decode(tags["p"] + "=" * (-len(tags["p"]) % 4), validate=True)
        tag, a, b = _der(der, 0)
        if tag != 0x30:
            return None
        t2, a2, b2 = _der(der, a)
        if t2 == 0x30:                                   # AlgorithmIdentifier, then BIT STRING { RSAPublicKey }
            if der[a2:a2 + 11] != bytes.fromhex("06092a864886f70d010101"):
                return None
            t3, a3, b3 = _der(der, b2)
            if t3 != 0x03 or der[a3] != 0:
                return None
            t4, a, b = _der(der, a3 + 1)
            if t4 != 0x30:
                return None
            t2, a2, b2 = _der(der, a)
        if t2 != 0x02:
            return None
        n = int.from_bytes(der[a2:b2], "big")
        t5, a5, b5 = _der(der, b2)
        if t5 != 0x02:
            return None
        return n, n.bit_length(), int.from_bytes(der[a5:b5], "big")
    except (ValueError, IndexError):
        return None


def txt_record(modulus, exponent=65537):
    """the TXT record of an RSA key (what a test or a key file writes)"""
    def der(tag, body):
        n = len(body)
        return bytes([tag]) + (bytes([n]) if n < 128 else bytes([0x80 | ((n.bit_length() + 7) // 8)]) + n.to_bytes((n.bit_length() + 7) // 8, "big")) + body

    def integer(x):
        return der(0x02, x.to_bytes(x.bit_length() // 8 + 1, "big"))
    rsa = der(0x30, integer(modulus) + integer(exponent))
    spki = der(0x30, der(0x30, bytes.fromhex("06092a864886f70d0101010500")) + der(0x03, b"\0" + rsa))
    return "v=DKIM1; k=rsa; p=" + base64.b64encode(spki).decode()


def _records(keys, name):
    if keys is None:
        return []
    if callable(keys):
        return list(keys(name) or [])
    return list(keys.get(name) or [])


# ---------------------------------------------------------------------------------------------- sanitisers (dkim/sanitizers.ts)
def _js_substring(s, a, b):
    a, b = max(a, 0), max(b, 0)
    return s[min(a, b):max(a, b)]


def _get_header_value(email, header):                    # sanitizers.ts:1-7, with String.indexOf's -1
    start = email.find(f"{header}: ") + len(header) + 2
    return _js_substring(email, start, email.find("\n", start))


def _set_header_value(email, header, value):             # sanitizers.ts:9-11: the first occurrence of the old value
    return email.replace(_get_header_value(email, header), value, 1)


def revertGoogleMessageId(email):                        # sanitizers.ts:16-29
    if "ARC-Authentication-Results" not in email:
        return email
    original = _get_header_value(email, "X-Google-Original-Message-ID")
    return _set_header_value(email, "Message-ID", original) if original else email


def removeLabels(email):                                 # sanitizers.ts:32-36: greedy within the line, first occurrence
    return re.sub("Subject: \\[[^\n\r\u2028\u2029]*\\]", "Subject:", email, count=1)


def insert13Before10(email):                             # sanitizers.ts:40-57 (its buffer has room for 1000 more bytes)
    raw = email.encode("latin-1")
    out = bytearray()
    for i, b in enumerate(raw):
        if b == 10 and i > 0 and raw[i - 1] != 13:
            out.append(13)
        out.append(b)
    return bytes(out[:len(raw) + 1000]).decode("latin-1")


def sanitizeTabs(email):                                 # sanitizers.ts:61-63: once
    return email.replace("=09", "\t", 1)


SANITIZERS = [revertGoogleMessageId, removeLabels, insert13Before10, sanitizeTabs]


# ---------------------------------------------------------------------------------------------- the batch call
def parse(email, domain=""):
    """zkwg_dkim_parse of one message -> (status, canonical signed header, DkimParsed)"""
    lib = _lib.load()
    P = DkimParsed()
    hdr = (C.c_uint8 * HEADER_CAP)()
    st = lib.zkwg_dkim_parse(email, len(email), domain.encode() if domain else None, hdr, HEADER_CAP, C.byref(P))
    _check(st)
    return st, bytes(hdr[:P.header_len]) if st == 0 else b"", P


def _as_bytes(email):
    return email.encode("latin-1") if isinstance(email, str) else bytes(email)


class _Call:
    """one zkwg_dkim_verify_batch: the arguments, and the results as Python values"""

    def __init__(self, emails, domain, keys, skip_body_hash, device, threads, body_stride=None, keep_on_device=False, want_bodies=True, timed=False,
                 fill=0, guard=0):
        """fill, guard: what the result rows hold before the call, and how many spare rows follow the n (for the tests of what is stored)"""
        lib = _lib.load()
        n = len(emails)
        self.n, self.emails = n, emails
        import time
        t_all = time.perf_counter()
        self._ptrs = (C.c_char_p * max(1, n))(*emails)
        self._lens = (C.c_uint64 * max(1, n))(*[len(e) for e in emails])
        # names and candidate keys: one threaded parse of the batch for s= and d= (zkwg_dkim_verify_batch parses again, with the headers)
        pre = (DkimParsed * max(1, n))()
        _check(lib.zkwg_dkim_parse_batch(n, self._ptrs, self._lens, domain.encode() if domain else None, threads, pre))
        flat, first, self.key_values = [], [0], []
        by_name, by_txt = {}, {}                         # a name is looked up once per call, a record is decoded once
        for i in range(n):
            P = pre[i]
            cand = []
            if P.status == 0:
                name = P.s + b"._domainkey." + P.d
                cand = by_name.get(name)
                if cand is None:
                    cand = []
                    for txt in _records(keys, name.decode("latin-1")):
                        if txt not in by_txt:
                            k, key = parse_txt_key(txt), None
                            if k is not None:
                                key = DkimKey()
                                C.memmove(key.modulus_be, (k[0] % (1 << 2048)).to_bytes(256, "big"), 256)
                                key.bits, key.exponent = k[1], k[2] if k[2] < (1 << 32) else 0
                            by_txt[txt] = (k, key)
                        if by_txt[txt][0] is not None:
                            cand.append(by_txt[txt])
                    by_name[name] = cand
            self.key_values.append([k for k, _ in cand])
            flat.extend(key for _, key in cand)
            first.append(len(flat))
        self.header_stride = max([pre[i].header_len for i in range(n) if pre[i].status == 0] + [16])
        if body_stride is None:                          # a canonical body outgrows its raw form by a CR per bare LF, and a final CR LF
            need = max([pre[i].body_bound for i in range(n) if pre[i].status == 0] + [16])
            body_stride = (need + 15) & ~15
        self.body_stride = body_stride
        A = DkimVerifyArgs()
        A.device, A.threads, A.n = device, threads, n
        self._keys = (DkimKey * max(1, len(flat)))(*flat)
        self._first = (C.c_uint32 * (n + 1))(*first)
        A.emails, A.email_len, A.keys, A.key_first = self._ptrs, self._lens, self._keys, self._first
        A.domain = domain.encode() if domain else None
        A.flags = _lib.DKIM_SKIP_BODY_HASH if skip_body_hash else 0
        A.header_stride, A.body_stride = self.header_stride, self.body_stride
        rows = max(1, n + guard)
        self._status, self._idx = (C.c_int32 * rows)(), (C.c_int32 * rows)()
        self._hlen, self._blen = (C.c_uint32 * rows)(), (C.c_uint32 * rows)()
        self._headers = (C.c_uint8 * (rows * self.header_stride))()
        self._bodies = (C.c_uint8 * (rows * self.body_stride))() if want_bodies else None
        self._bd, self._hd = (C.c_uint8 * (32 * rows))(), (C.c_uint8 * (32 * rows))()
        if fill:
            for a in (self._status, self._idx, self._hlen, self._blen, self._headers, self._bodies, self._bd, self._hd):
                if a is not None:
                    C.memset(a, fill, C.sizeof(a))
        self._parsed = (DkimParsed * max(1, n))()
        self._seconds = (C.c_double * 6)()
        A.status, A.key_index = C.addressof(self._status), C.addressof(self._idx)
        A.headers, A.header_len = C.addressof(self._headers), C.addressof(self._hlen)
        A.bodies = C.addressof(self._bodies) if want_bodies else None
        A.body_len = C.addressof(self._blen)
        A.body_digest, A.header_digest = C.addressof(self._bd), C.addressof(self._hd)
        A.parsed = self._parsed
        A.seconds = self._seconds if timed else None
        self.batch = DkimBatch() if keep_on_device else None
        if keep_on_device:
            A.device_batch = C.pointer(self.batch)
        self.args = A
        t0 = time.perf_counter()
        _check(lib.zkwg_dkim_verify_batch(C.byref(A)))
        self.call_seconds = time.perf_counter() - t0          # zkwg_dkim_verify_batch alone
        self.status = list(self._status[:n])
        self.key_index = list(self._idx[:n])
        self.seconds = list(self._seconds)
        self.total_seconds = time.perf_counter() - t_all      # with everything this wrapper does around the C call

    def header(self, i):
        return bytes(self._headers[i * self.header_stride:i * self.header_stride + self._hlen[i]])

    def body(self, i):
        return bytes(self._bodies[i * self.body_stride:i * self.body_stride + self._blen[i]])

    def body_digest(self, i):
        return bytes(self._bd[32 * i:32 * i + 32])

    def header_digest(self, i):
        return bytes(self._hd[32 * i:32 * i + 32])

    def outcome(self, i, applied=None):
        """the reference's result dict of message i, or the DkimError it throws"""
        lib = _lib.load()
        st, P = self.status[i], self._parsed[i]
        d = P.d.decode("latin-1")
        if st == _lib.DKIM_NOT_FOUND:
            return DkimError(f"{lib.zkwg_strerror(st).decode()} {d}", st)
        if st == _lib.DKIM_MULTIPLE_FROM:
            return DkimError(lib.zkwg_strerror(st).decode(), st)
        if st != 0:
            return DkimError(f"DKIM signature verification failed for domain {d}. Reason: {lib.zkwg_strerror(st).decode()}", st)
        mod, bits, _ = self.key_values[i][self.key_index[i]]
        return {"publicKey": mod, "signature": int.from_bytes(bytes(P.signature), "big"), "headers": self.header(i),
                "body": self.body(i) if self._bodies is not None else None, "bodyHash": P.bh_b64.decode(), "signingDomain": d,
                "selector": P.s.decode("latin-1"), "algo": P.a.decode("latin-1"), "format": P.c.decode("latin-1"), "modulusLength": bits,
                "appliedSanitization": applied}


def verify_batch(emails, domain="", enable_sanitization=True, keys=None, skip_body_hash=False, device=0, threads=0, body_stride=None):
    """-> per message the reference's result dict or a DkimError (not raised).  Sanitisers (dkim/index.ts:49-66) run only for the
    messages whose verdict is `bad signature`: their four variants go through one more call, and the first that passes, in the
    reference's order, gives the result and its name."""
    emails = [_as_bytes(e) for e in emails]
    call = _Call(emails, domain, keys, skip_body_hash, device, threads, body_stride)
    out = [call.outcome(i) for i in range(len(emails))]
    retry = [i for i, s in enumerate(call.status) if s == _lib.DKIM_BAD_SIGNATURE] if enable_sanitization else []
    if retry:
        variants = [_as_bytes(f(emails[i].decode("latin-1"))) for i in retry for f in SANITIZERS]
        again = _Call(variants, domain, keys, skip_body_hash, device, threads)
        for j, i in enumerate(retry):
            for k, f in enumerate(SANITIZERS):
                if again.status[4 * j + k] == 0:
                    out[i] = again.outcome(4 * j + k, f.__name__)
                    break
    return out


def verify_dkim_signature(email, domain="", enable_sanitization=True, keys=None, skip_body_hash=False, device=0):
    res = verify_batch([email], domain, enable_sanitization, keys, skip_body_hash, device)[0]
    if isinstance(res, DkimError):
        raise res
    return res


class DeviceBatch:
    """a verified batch whose zkwg_dkim_batch stays on the device (verify_batch_device); zkwg.generate_inputs_device takes it"""

    def __init__(self, call, device):
        self._call, self.device, self.n = call, device, call.n
        self.batch, self.status, self.key_index = call.batch, call.status, call.key_index

    def outcome(self, i):
        return self._call.outcome(i)

    def free(self):
        if self.batch is not None:
            _check(_lib.load().zkwg_dkim_batch_free(self.device, C.byref(self.batch)))
            self.batch = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def verify_batch_device(emails, domain="", keys=None, skip_body_hash=False, device=0, body_stride=None):
    """the verdicts of verify_batch without the sanitised retries; the canonical headers and bodies, bh=, the key that verified and the
    signature stay on the device in the layout zkwg_generate_inputs_device reads"""
    call = _Call([_as_bytes(e) for e in emails], domain, keys, skip_body_hash, device, 0, body_stride, keep_on_device=True, want_bodies=False)
    return DeviceBatch(call, device)


# ---------------------------------------------------------------------------------------------- command line
def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m zkwg.dkim")
    sub = ap.add_subparsers(dest="cmd", required=True)
    v = sub.add_parser("verify")
    v.add_argument("files", nargs="+")
    v.add_argument("--key", action="append", default=[], metavar="NAME=TXT")
    v.add_argument("--keys", metavar="keys.json")
    v.add_argument("--domain", default="")
    v.add_argument("--skip-body-hash", action="store_true")
    v.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    keys = {}
    if a.keys:
        for name, recs in json.load(open(a.keys)).items():
            keys.setdefault(name, []).extend([recs] if isinstance(recs, str) else recs)
    for kv in a.key:
        name, _, txt = kv.partition("=")
        keys.setdefault(name, []).append(txt)
    res = verify_batch([open(f, "rb").read() for f in a.files], a.domain, True, keys, a.skip_body_hash, a.device)
    failed = 0
    for f, r in zip(a.files, res):
        if isinstance(r, DkimError):
            failed += 1
            print(f"{f}: FAIL {r}")
        else:
            extra = f" sanitization={r['appliedSanitization']}" if r["appliedSanitization"] else ""
            print(f"{f}: pass d={r['signingDomain']} s={r['selector']} a={r['algo']} bits={r['modulusLength']}{extra}")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
