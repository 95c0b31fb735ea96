"""GPU: DKIM verification of raw emails on the device (zk_dkim_body, zk_dkim_hash, zk_dkim_verify) against the same cores
on the host (device = -1, which tests/test_dkim_cpu.py holds against the reference), byte for byte, for batches of 1, 33 and 131 messages
that mix the reference's emails, synthetic ones of all four c= modes, the bodies on the tile boundaries and every failure kind; then the
records and the witness that come out of a raw email."""
import ctypes as C
import hashlib
import json
import os

import pytest

import dkim_cases as cases
import real_email
from zkwg import _lib, dkim, synth

pytestmark = pytest.mark.gpu
STRIDE = 4096          # the body of multi-dkim-sig.eml (38,919 canonical bytes) does not fit: batches of 33 and 131 hold it
FILL = 0xA5
_calls = {}


def calls(n):
    """the batch of n on the host and on the device: computed once, shared by the tests below"""
    if n not in _calls:
        batch = cases.mixed_batch(n)
        emails = [m for m, _ in batch]
        _calls[n] = (batch, *[dkim._Call(emails, "", cases.keys(), False, dev, 4, body_stride=STRIDE, fill=FILL, guard=1) for dev in (-1, 0)])
    return _calls[n]


@pytest.mark.parametrize("n", [1, 33, 131])
def test_device_equals_host_byte_for_byte(n):
    batch, host, gpu = calls(n)
    assert gpu.status == host.status and gpu.key_index == host.key_index
    for name in ("_blen", "_hlen", "_bd", "_hd", "_headers", "_bodies", "_status", "_idx"):
        assert bytes(getattr(gpu, name)) == bytes(getattr(host, name)), name
    for i, (_, want) in enumerate(batch):
        if want is not None and not (want == _lib.DKIM_NO_KEY and host._parsed[i].body_len > STRIDE):
            assert host.status[i] == want, (i, host.status[i], want)
    assert host.status[0] == 0 and len(set(host.status)) >= (1 if n == 1 else 7)      # every failure kind is in the larger batches


@pytest.mark.parametrize("n", [1, 33, 131])
def test_nothing_is_stored_beyond_a_body_or_beyond_the_batch(n):
    batch, host, gpu = calls(n)
    bodies = bytes(gpu._bodies)
    for i in range(n):
        row, ln = bodies[i * STRIDE:(i + 1) * STRIDE], gpu._blen[i]
        if gpu.status[i] == _lib.DKIM_BODY_DOES_NOT_FIT:
            assert ln == 0 and FILL not in set(row[:64])          # (its own row holds the part that fitted)
        elif gpu._parsed[i].status == 0:
            assert row[ln:] == bytes([FILL]) * (STRIDE - ln), i
            assert gpu.body_digest(i) == hashlib.sha256(row[:ln]).digest() and gpu.header_digest(i) == hashlib.sha256(gpu.header(i)).digest()
        else:
            assert row == bytes([FILL]) * STRIDE and ln == 0, i
    for a in (gpu._bodies, gpu._headers, gpu._bd, gpu._hd, gpu._status, gpu._idx, gpu._blen, gpu._hlen):
        per = C.sizeof(a) // (n + 1)
        assert bytes(a)[n * per:] == bytes([FILL]) * per                                 # the guard row


def test_the_body_that_does_not_fit_leaves_its_neighbours_alone():
    batch, host, gpu = calls(33)
    big = [i for i, s in enumerate(gpu.status) if s == _lib.DKIM_BODY_DOES_NOT_FIT]
    assert len(big) == 1 and gpu._parsed[big[0]].d == b"starknet.org"
    i = big[0]
    for j in (i - 1, i + 1):
        alone = dkim._Call([batch[j][0]], "", cases.keys(), False, 0, 1, body_stride=STRIDE, fill=FILL)
        assert (alone.status[0], alone.body(0), alone.body_digest(0)) == (gpu.status[j], gpu.body(j), gpu.body_digest(j))
    # with room for it the same message is hashed to its bh= and then has no key
    roomy = dkim._Call([batch[i][0]], "", cases.keys(), False, 0, 1)
    assert roomy.status == [_lib.DKIM_NO_KEY] and roomy._blen[0] == 38919


def test_verdicts_and_sanitised_retry_on_the_device():
    res = dkim.verify_batch([cases.eml("email-good.eml"), cases.eml("email-good.eml").replace(b"Subject: ", b"Subject: [EmailListABC]", 1),
                             cases.eml("email-body-tampered.eml")], keys=cases.keys(), device=0)
    assert res[0]["signingDomain"] == "icloud.com" and res[0]["appliedSanitization"] is None
    assert res[1]["appliedSanitization"] == "removeLabels" and res[1]["headers"] == res[0]["headers"]
    assert str(res[2]) == "DKIM signature verification failed for domain icloud.com. Reason: body hash did not verify"
    want = real_email.dkim_result("test_eml")
    assert {k: res[0][k] for k in want} == want


def test_records_from_the_device_batch_equal_records_from_the_host_dicts():
    import zkwg
    c = zkwg.Circuit(zkwg.MAIN_EMAIL_VERIFIER, max_header=640, max_body=768, device=0)
    emails = [cases.eml("test.eml"), cases.eml("email-good-large.eml")] + [
        synth.synthetic_raw_email(21, i, 200 + 131 * i, canon) for i, canon in enumerate(("relaxed/relaxed", "relaxed/simple", "simple/relaxed", "simple/simple"))]
    dicts = dkim.verify_batch(emails, keys=cases.keys(), device=-1)
    assert all(isinstance(d, dict) for d in dicts)
    handle = dkim.verify_batch_device(emails, keys=cases.keys(), device=0)
    assert handle.status == [0] * len(emails)
    recs_dev, st_dev = zkwg.generate_inputs_device(c, handle)
    recs_host, st_host = zkwg.generate_inputs_device(c, dicts)
    assert st_dev == st_host == [0] * len(emails)
    assert recs_dev.cpu().numpy().tobytes() == recs_host.cpu().numpy().tobytes()
    handle.free()
    assert handle.batch is None


def test_raw_test_eml_to_witness():
    import zkwg
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "real_email_digests.json")))["cases"]["ev_test_eml"]
    assert gold["params"][:2] == [640, 768]
    c = zkwg.Circuit(zkwg.MAIN_EMAIL_VERIFIER, max_header=640, max_body=768, device=0)
    handle = dkim.verify_batch_device([cases.eml("test.eml")], keys=cases.keys(), device=0)
    recs, st = zkwg.generate_inputs_device(c, handle)
    assert handle.status == [0] and st == [0]
    wit, status = c.calculate_batch_host(recs.cpu().numpy().tobytes())
    assert status == [0] and hashlib.sha256(wit).hexdigest() == gold["kept_sha256"]


def test_command_line_on_a_file(tmp_path, capsys):
    keys = tmp_path / "keys.json"
    keys.write_text(json.dumps(cases.keys()))
    assert dkim.main(["verify", os.path.join(cases.GOLDEN, "test.eml"), "--keys", str(keys)]) == 0
    assert "test.eml: pass d=icloud.com s=1a1hai" in capsys.readouterr().out


def test_witness_command_line_takes_an_eml(tmp_path):
    from zkwg import generate_witness
    keys = tmp_path / "keys.json"
    keys.write_text(json.dumps(cases.keys()))
    out = tmp_path / "w.wtns"
    assert generate_witness.main(["EmailVerifier(640,768,121,17,0,0,0,0)", "--eml", os.path.join(cases.GOLDEN, "test.eml"), "--keys", str(keys), str(out)]) == 0
    import zkwg
    c = zkwg.Circuit(zkwg.MAIN_EMAIL_VERIFIER, max_header=640, max_body=768, device=0)
    wit, status = c.calculate_batch_host(c.pack(real_email.ev_inputs()))
    assert status == [0] and out.read_bytes() == c.wtns(wit)
