"""The SHA-256 round records on the device (csrc/zkwg_sha_rounds.h): an EmailVerifier handle's zk_sha_trace leaves 200 words per
block, zk_expand3 recomputes the 30,952 kept signals of every Sha256compression from them, and the 952-group trace is written only
for a handle with a descriptor consumer.  EmailVerifier(576, 192): 5 emails whose padded body is one block, two blocks and the
frame's last block; one email has a non-zero padding byte (AssertZeroPadding, checked by zk_sha_trace itself) and gets status 4."""
import pytest

pytestmark = pytest.mark.gpu

N, M = 576, 192
P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
BODY_LEN = (20, 100, 150, 70, 100)     # padded to 64, 128, 192 (the frame's last block), 128, 128 bytes
BAD = 3                                # the tampered email
FILL = 0xA5


def _handle(attach=None):
    import zkwg
    c = zkwg.Circuit(zkwg.MAIN_EMAIL_VERIFIER, max_header=N, max_body=M, device=0)
    if attach is not None:
        c.attach_r1cs(attach)
    return c


def _run(c, recs, n, mont=False):
    """prepare + expand on a scratch buffer pre-filled with FILL -> (witnesses, status, scratch)"""
    import torch
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream()
    d_in = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to(dev)
    d_status = torch.zeros(n, dtype=torch.int32, device=dev)
    d_scr = torch.full((c.scratch_bytes(n),), FILL, dtype=torch.uint8, device=dev)
    d_wit = torch.empty(n * c.witness_bytes, dtype=torch.uint8, device=dev)
    c.prepare_device(d_in, n, d_status, d_scr, s)
    (c.expand_montgomery_device if mont else c.expand_device)(d_in, n, d_scr, 0, n, d_wit, s)
    torch.cuda.synchronize()
    return d_wit, d_status.cpu().tolist(), d_scr, d_in


@pytest.fixture(scope="module")
def batch():
    """inputs, the C oracle's witnesses (computed once, never modified) and the plain handle's run"""
    from oracle import coracle
    from test_ev_cpu import _inputs
    inps = [_inputs(N, M, 0, index=20 + i, body_len=bl) for i, bl in enumerate(BODY_LEN)]
    assert sorted({(int(i["emailBodyLength"]) // 64) for i in inps}) == [1, 2, 3]
    for i in inps:      # (the generator pads a body that fills the frame by one more block of zeros: the circuit takes maxBodyLength values)
        assert not any(int(b) for b in i["emailBody"][M:])
        i["emailBody"] = i["emailBody"][:M]
    hlen = int(inps[BAD]["emailHeaderLength"])
    inps[BAD]["emailHeader"][hlen + 1] = "1"                      # padding not zero
    owit, ostatus = [], []
    for part in (inps[:3], inps[3:]):                             # (the suite's oracle calls take up to three emails)
        w, st, W = coracle.calculate(0, N, M, 0, part, threads=3)
        owit += w
        ostatus += st
    assert ostatus == [4 if i == BAD else 0 for i in range(5)]
    c = _handle()
    assert W == c.W
    recs = b"".join(c.pack(i) for i in inps)
    wit, status, scr, d_in = _run(c, recs, 5)
    return dict(inps=inps, owit=owit, c=c, recs=recs, wit=wit, status=status, scr=scr, d_in=d_in)


def _trace_words(c, scr, n):
    """the u64 words of every block's trace area, all emails, from a device scratch buffer"""
    import numpy as np
    lay = c.image_layout(n)
    bits = np.frombuffer(scr.cpu().numpy().tobytes(), dtype=np.uint64, count=n * lay["bits_words"], offset=lay["off_bits"]).reshape(n, lay["bits_words"])
    starts = [src for _, _, typ, src, *_ in c.segment_table() if typ == 3]        # ZKWG_SEG_SHA_SP: the first group of a block's trace
    assert len(starts) == N // 64 + M // 64
    return np.concatenate([bits[:, s:s + 952] for s in starts], axis=1)


def test_every_witness_byte_of_the_good_emails_equals_the_oracle(batch):
    c, wb = batch["c"], batch["c"].witness_bytes
    assert batch["status"] == [4 if i == BAD else 0 for i in range(5)]
    wit = batch["wit"].cpu().numpy().tobytes()
    for e in range(5):
        if e != BAD:
            assert wit[e * wb:(e + 1) * wb] == bytes(batch["owit"][e]), e


def test_a_handle_without_a_descriptor_consumer_leaves_the_trace_area_untouched(batch):
    tr = _trace_words(batch["c"], batch["scr"], 5)
    assert tr.shape == (5, 12 * 952)
    import numpy as np
    assert bool((tr == np.uint64(int.from_bytes(bytes([FILL]) * 8, "little"))).all())


def test_montgomery_form_is_standard_form_times_r(batch):
    import numpy as np
    c = batch["c"]
    mont, status, _, _ = _run(c, batch["recs"], 5, mont=True)
    assert status == batch["status"]
    R = (1 << 256) % P
    std = batch["wit"].cpu().numpy().reshape(5, c.W, 32)
    mnt = mont.cpu().numpy().reshape(5, c.W, 32)
    good = [e for e in range(5) if e != BAD]
    # distinct (standard, Montgomery) pairs of the four good emails: a few thousand of the 2.9 M slots
    both = np.ascontiguousarray(np.concatenate([std[good], mnt[good]], axis=2)).reshape(-1, 64)
    pairs = np.unique(both.view("V64").ravel())
    assert 1000 < len(pairs) < 50000
    for row in pairs:
        b = row.tobytes()
        v, m = int.from_bytes(b[:32], "little"), int.from_bytes(b[32:], "little")
        assert m == v * R % P, v


def test_attached_constraint_system_still_gets_the_trace(batch):
    """a handle with a system attached before the prepare: A.w | B.w | C.w from the image (descriptors name trace words) are
    byte-identical to the evaluation of the expanded witness, the `.r1cs` check passes, and the trace area is written"""
    import torch
    import zkwg
    c0 = batch["c"]
    cs = zkwg.WitnessCalculator(c0).constraint_system()
    c1 = _handle(attach=cs)
    w1, status, scr, d_in = _run(c1, batch["recs"], 5)
    assert status == batch["status"]
    assert torch.equal(w1, batch["wit"])
    s = torch.cuda.current_stream()
    good = [e for e in range(5) if e != BAD]
    assert [cs.first_violations_device(batch["wit"], 5, c0.witness_bytes)[e] for e in good] == [None] * 4
    want = cs.evaluate_device(batch["wit"], 5, c0.witness_bytes, s)
    got = torch.empty((5, c1.abc_bytes), dtype=torch.uint8, device=w1.device)
    c1.expand_abc_device(d_in, 5, scr, 0, 5, got, s)
    torch.cuda.synchronize()
    for e in good:
        assert torch.equal(got[e], want[e]), e
    tr = _trace_words(c1, scr, 5)
    import numpy as np
    fill = np.uint64(int.from_bytes(bytes([FILL]) * 8, "little"))
    assert not bool((tr == fill).any())                      # every group is below 2^35
