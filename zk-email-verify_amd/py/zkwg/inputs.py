"""Host-side input generation: mirrors packages/helpers/src/{input-generators,sha-utils,
binary-format}.ts of the reference (the `CircuitInput` object is the boundary format).

  sha256_pad                      <- sha-utils.ts:88-111      sha256Pad
  generate_partial_sha            <- sha-utils.ts:30-80       generatePartialSHA
  partial_sha                     <- sha-utils.ts:82-85 + lib/fast-sha256.ts:240-251 cacheState
  to_circom_bigint_bytes          <- binary-format.ts:71-83   toCircomBigIntBytes
  generate_email_verifier_inputs_from_dkim_result
                                  <- input-generators.ts:190-252
  generate_email_verifier_inputs  <- input-generators.ts:168-181 (the raw email; DKIM by zkwg.dkim)
"""
import struct

MAX_HEADER_PADDED_BYTES = 1024  # constants.ts:2
MAX_BODY_PADDED_BYTES = 1536    # constants.ts:3
CIRCOM_BIGINT_N = 121           # constants.ts:5
CIRCOM_BIGINT_K = 17            # constants.ts:6

_K = [
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
    0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
    0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
    0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
    0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2]
_IV = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]


def _rotr(x, r):
    return ((x >> r) | (x << (32 - r))) & 0xFFFFFFFF


def _compress(st, block):
    w = list(struct.unpack(">16I", block))
    for t in range(16, 64):
        s0 = _rotr(w[t - 15], 7) ^ _rotr(w[t - 15], 18) ^ (w[t - 15] >> 3)
        s1 = _rotr(w[t - 2], 17) ^ _rotr(w[t - 2], 19) ^ (w[t - 2] >> 10)
        w.append((w[t - 16] + s0 + w[t - 7] + s1) & 0xFFFFFFFF)
    a, b, c, d, e, f, g, h = st
    for t in range(64):
        t1 = (h + (_rotr(e, 6) ^ _rotr(e, 11) ^ _rotr(e, 25)) + ((e & f) ^ (~e & g)) + _K[t] + w[t]) & 0xFFFFFFFF
        t2 = ((_rotr(a, 2) ^ _rotr(a, 13) ^ _rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & 0xFFFFFFFF
        h, g, f, e, d, c, b, a = g, f, e, (d + t1) & 0xFFFFFFFF, c, b, a, (t1 + t2) & 0xFFFFFFFF
    return [(x + y) & 0xFFFFFFFF for x, y in zip(st, (a, b, c, d, e, f, g, h))]


def partial_sha(msg: bytes) -> bytes:
    """SHA-256 midstate after absorbing `msg` (a multiple of 64 bytes), as 32 big-endian bytes
    (sha-utils.ts:82-85 -> lib/fast-sha256.ts:240-251 cacheState)."""
    assert len(msg) % 64 == 0
    st = list(_IV)
    for i in range(0, len(msg), 64):
        st = _compress(st, msg[i:i + 64])
    return struct.pack(">8I", *st)


def sha256_pad(message: bytes, max_sha_bytes: int):
    """sha-utils.ts:88-111 -> (padded bytes of length max_sha_bytes, padded message length)."""
    msg_len_bits = len(message) * 8
    res = message + b"\x80"
    while (len(res) * 8 + 64) % 512 != 0:
        res += b"\x00"
    res += msg_len_bits.to_bytes(8, "big")
    assert (len(res) * 8) % 512 == 0, "Padding did not complete properly!"
    message_len = len(res)
    if len(res) > max_sha_bytes:
        raise ValueError(
            f"Padding to max length did not complete properly! Your padded message is {len(res)} long but max is {max_sha_bytes}!")
    res += b"\x00" * (max_sha_bytes - len(res))
    return res, message_len


def find_index_in_uint8array(array: bytes, selector: bytes) -> int:
    """sha-utils.ts:9-24, literally (on a mismatch j restarts at 0 and i still advances, so this is NOT a
    general substring search: "aab" is not found in "aaab")."""
    i = j = 0
    while i < len(array):
        if array[i] == selector[j]:
            j += 1
            if j == len(selector):
                return i - j + 1
        else:
            j = 0
        i += 1
    return -1


def generate_partial_sha(body: bytes, body_length: int, selector_string, max_remaining_body_length: int, selector_index=None):
    """sha-utils.ts:30-80.  selector_index (not the reference's): the position to cut below, in place of the selector's search."""
    if selector_index is not None:
        selector_string = None
    else:
        selector_index = 0
    if selector_string:
        sel = selector_string.encode() if isinstance(selector_string, str) else selector_string
        selector_index = find_index_in_uint8array(body, sel)
        if selector_index == -1:
            raise ValueError(f'SHA precompute selector "{selector_string}" not found in the body')
    sha_cutoff_index = (selector_index // 64) * 64
    precompute_text = body[:sha_cutoff_index]
    body_remaining = body[sha_cutoff_index:]
    body_remaining_length = body_length - len(precompute_text)
    if body_remaining_length > max_remaining_body_length:
        raise ValueError(
            f"Remaining body {body_remaining_length} after the selector is longer than max ({max_remaining_body_length})")
    if len(body_remaining) % 64 != 0:
        raise ValueError("Remaining body was not padded correctly with int64s")
    body_remaining = body_remaining + b"\x00" * max(0, max_remaining_body_length - len(body_remaining))
    return partial_sha(precompute_text), body_remaining, body_remaining_length


def to_circom_bigint_bytes(num: int):
    """binary-format.ts:71-83: 17 x 121-bit limbs as decimal strings."""
    msk = (1 << CIRCOM_BIGINT_N) - 1
    return [str((num >> (i * CIRCOM_BIGINT_N)) & msk) for i in range(CIRCOM_BIGINT_K)]


def remove_soft_line_breaks(body: bytes):
    """input-generators.ts:127-158: drops every "=\r\n", zero-pads back to len(body); also returns
    the clean -> original position map."""
    result = bytearray()
    position_map = {}
    i = 0
    n = len(body)
    while i < n:
        if i + 2 < n and body[i] == 61 and body[i + 1] == 13 and body[i + 2] == 10:
            i += 3
        else:
            position_map[len(result)] = i
            result.append(body[i])
            i += 1
    result.extend(b"\0" * (n - len(result)))
    return bytes(result), position_map


def get_adjusted_selector(original_body: bytes, selector: str, clean_content: bytes, position_map) -> str:
    """input-generators.ts:44-105 (findSelectorInCleanContent + getAdjustedSelector)."""
    body_string = original_body.decode("utf-8", errors="replace")
    if selector in body_string:
        return selector
    clean_string = clean_content.decode("utf-8", errors="replace")
    selector_index = clean_string.find(selector)
    if selector_index == -1:
        raise ValueError(f'SHA precompute selector "{selector}" not found in cleaned body')
    if selector_index not in position_map:
        raise ValueError("Failed to map selector position to original body")
    original_index = position_map[selector_index]
    return body_string[original_index:original_index + len(selector) + 3]


def generate_email_verifier_inputs_from_dkim_result(dkim, max_headers_length=None, max_body_length=None,
                                                    ignore_body_hash_check=False, sha_precompute_selector=None,
                                                    enable_header_masking=False, header_mask=None,
                                                    enable_body_masking=False, body_mask=None,
                                                    remove_soft_line_breaks_flag=False, cut_position=None):
    """input-generators.ts:190-252.  `dkim` = dict(headers: bytes, body: bytes, bodyHash: str,
    publicKey: int, signature: int) -- the DKIMVerificationResult fields the function uses.  cut_position (not the
    reference's): a position in the body; the SHA prefix is cut at the 64-byte boundary below it, without a selector."""
    headers = dkim["headers"]
    message_padded, message_padded_len = sha256_pad(headers, max_headers_length or MAX_HEADER_PADDED_BYTES)
    inputs = {
        "emailHeader": [str(b) for b in message_padded],
        "emailHeaderLength": str(message_padded_len),
        "pubkey": to_circom_bigint_bytes(dkim["publicKey"]),
        "signature": to_circom_bigint_bytes(dkim["signature"]),
    }
    if enable_header_masking:
        inputs["headerMask"] = list(header_mask)
    if not ignore_body_hash_check:
        body, body_hash = dkim.get("body"), dkim.get("bodyHash")
        if not body and body != b"" or not body_hash:
            raise ValueError("body and bodyHash are required when ignoreBodyHashCheck is false")
        body_hash_index = headers.decode("latin-1").find(body_hash)
        max_body = max_body_length or MAX_BODY_PADDED_BYTES
        body_sha_length = ((len(body) + 63 + 65) // 64) * 64
        body_padded, body_padded_len = sha256_pad(body, max(max_body, body_sha_length))
        adjusted_selector = sha_precompute_selector
        if cut_position is not None:
            if sha_precompute_selector:
                raise ValueError("a cut position and shaPrecomputeSelector exclude each other")
            # what remains is the padded body from the cut on, bpad - cut bytes: the zero fill up to bodySHALength, which the
            # reference slices into bodyRemaining with the rest (64 bytes more than the circuit takes when the cut leaves exactly
            # maxBodyLength), is not part of it
            body_padded = body_padded[:body_padded_len]
        elif sha_precompute_selector:
            clean, pmap = remove_soft_line_breaks(body_padded)
            sel = sha_precompute_selector if isinstance(sha_precompute_selector, str) else sha_precompute_selector.decode()
            adjusted_selector = get_adjusted_selector(body, sel, clean, pmap)
        pre, remaining, remaining_len = generate_partial_sha(body_padded, body_padded_len,
                                                             adjusted_selector, max_body, cut_position)
        inputs["emailBodyLength"] = str(remaining_len)
        inputs["precomputedSHA"] = [str(b) for b in pre]
        inputs["bodyHashIndex"] = str(body_hash_index)
        inputs["emailBody"] = [str(b) for b in remaining]
        if remove_soft_line_breaks_flag:
            clean, _ = remove_soft_line_breaks(remaining)
            inputs["decodedEmailBodyIn"] = [str(b) for b in clean]
        if enable_body_masking:
            inputs["bodyMask"] = list(body_mask)
    return inputs


def generate_email_verifier_inputs(raw_email, params=None, dkim_verification_args=None, keys=None, device=0):
    """input-generators.ts:168-181: verifyDKIMSignature(rawEmail, domain, enableSanitization), then the function above.
    `params`: the reference's InputGenerationArgs by their own names (maxHeadersLength, maxBodyLength, ignoreBodyHashCheck,
    shaPrecomputeSelector, enableHeaderMasking, headerMask, enableBodyMasking, bodyMask, removeSoftLineBreaks);
    `dkim_verification_args`: domain, enableSanitization; `keys`: see zkwg.dkim (there is no DNS)."""
    from . import dkim
    p, a = dict(params or {}), dict(dkim_verification_args or {})
    result = dkim.verify_dkim_signature(raw_email, a.get("domain") or "", a.get("enableSanitization", True), keys=keys, device=device)
    return generate_email_verifier_inputs_from_dkim_result(
        result, p.get("maxHeadersLength"), p.get("maxBodyLength"), bool(p.get("ignoreBodyHashCheck")), p.get("shaPrecomputeSelector"),
        bool(p.get("enableHeaderMasking")), p.get("headerMask"), bool(p.get("enableBodyMasking")), p.get("bodyMask"),
        bool(p.get("removeSoftLineBreaks")))


def locate_substring(source, needle=None, start=None, length=None, check_uniqueness=True):
    """(substringStartIndex, substringLength) of EmailReveal over `source` = the emailHeader / emailBody array the circuit sees
    (bytes or a list of numbers): the position of `needle`, or the given start and length checked against the array.  Raises
    ValueError when the needle is absent, or occurs more than once while the circuit checks uniqueness."""
    src = bytes(int(b) for b in source)
    if needle is not None:
        needle = needle.encode() if isinstance(needle, str) else bytes(needle)
        if not needle:
            raise ValueError("the needle is empty")
        at = src.find(needle)
        if at < 0:
            raise ValueError("the needle does not occur in what the circuit sees of the email")
        if check_uniqueness and src.find(needle, at + 1) >= 0:
            raise ValueError("the needle occurs more than once and the circuit checks uniqueness")
        return at, len(needle)
    if start is None or length is None:
        raise ValueError("give a needle, or start and length")
    if start < 0 or length < 0 or start + length > len(src):
        raise ValueError("start and length do not lie inside the source")
    return int(start), int(length)


def locate_needle(dkim, params, needle):
    """The rule of zkwg_generate_reveal_inputs_device for one email -> the first position of `needle` in the canonical
    signed header bytes, or (revealFromBody) in the canonical body bytes: a true substring search that never looks at the SHA padding.
    ValueError: the needle is empty or longer than maxSubstringLength (where params gives it), or absent."""
    p = dict(params or {})
    nd = needle.encode() if isinstance(needle, str) else bytes(needle or b"")
    if not nd or (p.get("maxSubstringLength") is not None and len(nd) > int(p["maxSubstringLength"])):
        raise ValueError("the needle is empty or longer than maxSubstringLength")
    pos = bytes(dkim["body"] if p.get("revealFromBody") else dkim["headers"]).find(nd)
    if pos < 0:
        raise ValueError("the needle does not occur in the canonical " + ("body" if p.get("revealFromBody") else "header"))
    return pos


def generate_email_reveal_inputs_from_dkim_result(dkim, params=None, needle=None, start=None, length=None, cut_at_needle=False):
    """generate_email_verifier_inputs_from_dkim_result plus substringStartIndex / substringLength of EmailReveal
    (circuits/email-reveal.circom).  params: maxHeadersLength, maxBodyLength, ignoreBodyHashCheck, shaPrecomputeSelector as for
    EmailVerifier, and revealFromBody, shouldCheckUniqueness (default 1), maxSubstringLength (optional: checked when given).
    cut_at_needle: the needle is the input, as for zkwg_generate_reveal_inputs_device, whose rule this states.  It is
    looked for in the canonical header or body bytes themselves (locate_needle); with revealFromBody the body's SHA prefix is cut at
    the 64-byte boundary below it -- shaPrecomputeSelector is refused beside it -- so a body much longer than maxBodyLength
    needs no selector.  The errors come in the order of the device's codes: header too long (1), selector not found (3), the needle
    empty or too long (7), absent (5), remaining body too long (2), not unique in the array the circuit sees (6)."""
    p = dict(params or {})
    if p.get("enableHeaderMasking") or p.get("enableBodyMasking") or p.get("removeSoftLineBreaks"):
        raise ValueError("EmailReveal has no masking and no soft-line-break removal")
    if p.get("revealFromBody") and p.get("ignoreBodyHashCheck"):
        raise ValueError("revealFromBody needs the body-hash check")
    uniq = bool(p.get("shouldCheckUniqueness", 1))
    if cut_at_needle:
        if needle is None or start is not None or length is not None:
            raise ValueError("cut_at_needle takes a needle, not start and length")
        from_body = bool(p.get("revealFromBody"))
        if from_body and p.get("shaPrecomputeSelector"):
            raise ValueError("the needle says where the body is cut: shaPrecomputeSelector is refused beside it")
        sha256_pad(dkim["headers"], p.get("maxHeadersLength") or MAX_HEADER_PADDED_BYTES)                       # (1)
        if p.get("shaPrecomputeSelector") and not p.get("ignoreBodyHashCheck"):                                  # (3)
            max_body = p.get("maxBodyLength") or MAX_BODY_PADDED_BYTES
            padded, padded_len = sha256_pad(dkim["body"], max(max_body, ((len(dkim["body"]) + 63 + 65) // 64) * 64))
            sel = p["shaPrecomputeSelector"]
            sel = sel if isinstance(sel, str) else sel.decode()
            adjusted = get_adjusted_selector(dkim["body"], sel, *remove_soft_line_breaks(padded))
            if find_index_in_uint8array(padded, adjusted.encode()) < 0:
                raise ValueError(f'SHA precompute selector "{adjusted}" not found in the body')
        pos = locate_needle(dkim, p, needle)                                                                    # (7), (5)
        inputs = generate_email_verifier_inputs_from_dkim_result(
            dkim, p.get("maxHeadersLength"), p.get("maxBodyLength"), bool(p.get("ignoreBodyHashCheck")), p.get("shaPrecomputeSelector"),
            cut_position=pos if from_body else None)                                                            # (2)
        nd = needle.encode() if isinstance(needle, str) else bytes(needle)
        src = bytes(int(b) for b in inputs["emailBody" if from_body else "emailHeader"])
        at = pos - (pos // 64) * 64 if from_body else pos
        assert src[at:at + len(nd)] == nd and src.find(nd) == at
        if uniq and src.find(nd, at + 1) >= 0:                                                                  # (6)
            raise ValueError("the needle occurs more than once and the circuit checks uniqueness")
        inputs["substringStartIndex"], inputs["substringLength"] = str(at), str(len(nd))
        return inputs
    inputs = generate_email_verifier_inputs_from_dkim_result(dkim, p.get("maxHeadersLength"), p.get("maxBodyLength"),
                                                             bool(p.get("ignoreBodyHashCheck")), p.get("shaPrecomputeSelector"))
    a, n = locate_substring(inputs["emailBody" if p.get("revealFromBody") else "emailHeader"], needle, start, length, uniq)
    inputs["substringStartIndex"], inputs["substringLength"] = str(a), str(n)
    return inputs


def generate_email_reveal_inputs(raw_eml, params=None, keys=None, needle=None, start=None, length=None, dkim_verification_args=None,
                                 device=0, cut_at_needle=False):
    """A raw email -> the CircuitInput of EmailReveal: verifyDKIMSignature, EmailVerifier's inputs, and the position of
    `needle` (or start / length) in the canonical header or body the circuit sees.  cut_at_needle: see
    generate_email_reveal_inputs_from_dkim_result."""
    from . import dkim
    a = dict(dkim_verification_args or {})
    result = dkim.verify_dkim_signature(raw_eml, a.get("domain") or "", a.get("enableSanitization", True), keys=keys, device=device)
    return generate_email_reveal_inputs_from_dkim_result(result, params, needle, start, length, cut_at_needle)


def clean_email_address(addr):
    """The address CleanEmailAddress (utils/email.circom:16-140) accepts as `decoded` for `encoded` = addr: the periods of the
    local part and the "+alias" up to the '@' removed ("a.b+c@d.e" -> "ab@d.e").  The template means exactly one '@' with no
    '+' behind it; anything else has a witness too, but not this meaning: ValueError."""
    if addr.count("@") != 1:
        raise ValueError("the address needs exactly one '@'")
    local, domain = addr.split("@")
    if "+" in domain:
        raise ValueError("a '+' behind the '@' is outside what the template means")
    return local.split("+")[0].replace(".", "") + "@" + domain


def generate_clean_email_address_inputs(addr, max_length):
    """The CircuitInput of CleanEmailAddress(max_length) for an address: encoded = its bytes, decoded = those of
    clean_email_address(addr), both zero-padded to max_length."""
    enc, dec = addr.encode("ascii"), clean_email_address(addr).encode("ascii")
    if len(enc) > max_length:
        raise ValueError(f"the address is longer than max_length = {max_length}")
    pad = lambda b: [str(v) for v in b] + ["0"] * (max_length - len(b))
    return {"encoded": pad(enc), "decoded": pad(dec)}
