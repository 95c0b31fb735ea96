"""GPU: EmailReveal's records from one needle per email (zkwg_generate_reveal_inputs_device, zk_gen_reveal_inputs) against
the host mirror's cut_at_needle, byte for byte; every per-email code; the refused argument combinations; and a raw email to its witness
with nothing of it looked at on the host."""
import ctypes as C
import random

import pytest

import emailreveal as er

pytestmark = pytest.mark.gpu

BODY_UNIQ = (576, 192, 0, 1, 12, 1, 0)         # reveal from the body, uniqueness checked
MARK = b"~MARK~ER~"
_c = {}


def _circuit(shape):
    import zkwg
    shape = er.SHAPES.get(shape, shape)
    if shape not in _c:
        _c[shape] = zkwg.Circuit(device=0, **er.circuit_kwargs(shape))
    return _c[shape]


def _params(shape):
    shape = er.SHAPES.get(shape, shape)
    return dict(er.reveal_params(shape), maxSubstringLength=shape[4])


def _with_body(seed, index, length, marker=b"", at=0):
    from zkwg import synth
    b = bytearray(synth.synthetic_body(random.Random(seed * 1000 + index), length))
    b[at:at + len(marker)] = marker
    return synth.synthetic_dkim_result(seed, index, body=bytes(b))


def _mirror(c, shape, d, needle):
    from zkwg import inputs
    return c.pack(inputs.generate_email_reveal_inputs_from_dkim_result(d, _params(shape), needle=needle, cut_at_needle=True))


def _status(c, ds, needles, **kw):
    import zkwg
    return zkwg.generate_inputs_device(c, ds, needles=needles, **kw)[1]


def test_device_records_equal_the_mirrors_for_header_and_body_needles():
    import zkwg
    from zkwg import synth
    # the body: position on both sides of 64, 1,024 and 2,048, across the tile boundaries, a multiple of 64, the body's last bytes
    where = [(70, 20), (150, 70), (1100, 1020), (1200, 1088), (2150, 2043), (2900, 2900 - len(MARK))]
    ds = [_with_body(41, i, ln, MARK, at) for i, (ln, at) in enumerate(where)]
    assert [d["body"].find(MARK) for d in ds] == [at for _, at in where] and ds[5]["body"].endswith(MARK)
    c = _circuit(BODY_UNIQ)
    recs, st = zkwg.generate_inputs_device(c, ds, needles=[MARK] * 6)
    assert st == [0] * 6
    raw = recs.cpu().numpy().tobytes()
    for i, d in enumerate(ds):
        assert raw[i * c.in_stride:(i + 1) * c.in_stride] == _mirror(c, BODY_UNIQ, d, MARK), i
    wit, status = c.calculate_batch_host(raw)
    assert status == [0] * 6
    slot = {nm: s for s, nm in c.symbols()}["main.revealed[0]"]
    for e in range(6):
        v = wit[e * c.witness_bytes + 32 * slot:e * c.witness_bytes + 32 * slot + 32]
        assert v[:len(MARK)] == MARK and v[len(MARK):] == bytes(32 - len(MARK))
    # the header: a needle of its own per email, a str among them, bodies of several lengths prepared as without a needle
    a = _circuit("A")
    hs = [synth.synthetic_dkim_result(42, i, body_len=60 + 10 * i) for i in range(6)]
    needles = [b"message-id:<", "subject:", b"from:Synthet", b"to:recipient", hs[4]["headers"][hs[4]["headers"].index(b"date:"):][:12], b"bh="]
    recs, st = zkwg.generate_inputs_device(a, hs, needles=needles)
    assert st == [0] * 6
    raw = recs.cpu().numpy().tobytes()
    for i, d in enumerate(hs):
        assert raw[i * a.in_stride:(i + 1) * a.in_stride] == _mirror(a, "A", d, needles[i]), i
    assert a.calculate_batch_host(raw, want_witness=False)[1] == [0] * 6


def test_every_code_once():
    import zkwg
    u, b = _circuit(BODY_UNIQ), _circuit("B")
    good = _with_body(43, 0, 150, MARK, 70)
    assert _status(u, [good], [MARK]) == [0]
    assert _status(u, [good, good], [b"~ABSENT~", MARK]) == [5, 0]                               # absent
    soft = _with_body(43, 1, 150, b"hel=\r\nlo", 80)
    assert _status(u, [soft], [b"hello"]) == [5] and _status(u, [soft], [b"hel=\r\nlo"]) == [0]  # only across a soft line break
    twice = _with_body(43, 2, 150, MARK, 70)
    twice = dict(twice, body=twice["body"][:100] + MARK + twice["body"][100 + len(MARK):])
    recs, st = zkwg.generate_inputs_device(u, [twice, good], needles=[MARK, MARK])
    assert st == [6, 0]                                                                          # twice in the window, uniqueness on
    off = [u.lib.zkwg_input_offset(u.h, f) for f in (7, 13, 14)]
    row = recs[0].cpu().numpy().tobytes()
    assert all(row[o:o + 4] == bytes(4) for o in off)                                            # no body length, no indices
    recs, st = zkwg.generate_inputs_device(b, [twice], needles=[MARK])
    assert st == [0]                                                                             # the same without the check
    assert recs[0].cpu().numpy().tobytes() == _mirror(b, "B", twice, MARK)
    assert _status(u, [good, good], [b"", MARK]) == [7, 0]                                       # empty
    assert _status(u, [good], [good["body"][64:64 + 13]]) == [7]                                 # max_substring + 1
    assert _status(u, [good], [good["body"][64:64 + 12]]) == [0]
    early = _with_body(43, 3, 400, MARK, 10)
    assert _status(u, [early, good], [MARK, MARK]) == [2, 0]                                     # so early that the rest is too long
    assert _status(u, [early], [b"~ABSENT~"]) == [5] and _status(u, [early], [b""]) == [7]       # 7 and 5 come before 2
    big = dict(good, headers=good["headers"] + b"x" * 600)
    assert _status(u, [big, good], [b"", MARK]) == [1, 0]                                        # 1 as before, and before 7
    # the header: the needle's occurrences in the SHA padding count for uniqueness, but it is not found there
    a = _circuit("A")
    assert _status(a, [good], [b"\x80"]) == [5]
    assert _status(a, [good, good], [b"<", b"message-id:<"]) == [6, 0]                           # '<' : in from: and in message-id:
    assert _status(a, [early], [b"message-id:<"]) == [2]                                         # the body as without a needle


def test_code_4_is_reported_as_before():
    """a body longer than its slot (the C-ABI directly: the Python entry sizes the slot itself)"""
    import torch
    from zkwg import _lib
    u = _circuit(BODY_UNIQ)
    d = _with_body(44, 0, 150, MARK, 70)
    dev = "cuda:0"
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    body = t(d["body"] + d["body"])
    stride = len(d["body"])
    bl = torch.tensor([stride + 1, stride], dtype=torch.int32, device=dev)
    bh = t(d["bodyHash"].encode().ljust(44, b"\0")[:44] * 2)
    pk, sg = t(int(d["publicKey"]).to_bytes(256, "big") * 2), t(int(d["signature"]).to_bytes(256, "big") * 2)
    hdr2 = t(d["headers"] * 2)
    hl2 = torch.tensor([len(d["headers"])] * 2, dtype=torch.int32, device=dev)
    batch = _lib.DkimBatch(hdr2.data_ptr(), hl2.data_ptr(), body.data_ptr(), bl.data_ptr(), bh.data_ptr(), pk.data_ptr(), sg.data_ptr(),
                           None, len(d["headers"]), stride, 0)
    nb, nf = t(MARK + MARK), torch.tensor([0, 9, 18], dtype=torch.int32, device=dev)
    q = _lib.Needles(nb.data_ptr(), nf.data_ptr())
    recs = torch.empty((2, u.in_stride), dtype=torch.uint8, device=dev)
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    assert u.lib.zkwg_generate_reveal_inputs_device(u.h, C.byref(batch), C.byref(q), 2, recs.data_ptr(), st.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [4, 0]
    assert recs[1].cpu().numpy().tobytes() == _mirror(u, BODY_UNIQ, d, MARK)
    # null pointers and a selector beside body needles: ZKWG_RC_BAD_ARG (2); an EmailVerifier handle: ZKWG_RC_BAD_CONFIG
    import zkwg
    bad_arg = u.lib.zkwg_generate_reveal_inputs_device(u.h, C.byref(batch), None, 2, recs.data_ptr(), st.data_ptr(), None)
    assert bad_arg != 0
    q0 = _lib.Needles(nb.data_ptr(), None)
    assert u.lib.zkwg_generate_reveal_inputs_device(u.h, C.byref(batch), C.byref(q0), 2, recs.data_ptr(), st.data_ptr(), None) == bad_arg
    batch.selector, batch.selector_len = nb.data_ptr(), 9
    assert u.lib.zkwg_generate_reveal_inputs_device(u.h, C.byref(batch), C.byref(q), 2, recs.data_ptr(), st.data_ptr(), None) == bad_arg
    batch.selector, batch.selector_len = None, 0
    ev = zkwg.Circuit(zkwg.MAIN_EMAIL_VERIFIER, max_header=576, max_body=192, device=0)
    bad_cfg = ev.lib.zkwg_generate_reveal_inputs_device(ev.h, C.byref(batch), C.byref(q), 2, recs.data_ptr(), st.data_ptr(), None)
    assert bad_cfg not in (0, bad_arg)
    torch.cuda.synchronize()


def test_aaab_succeeds_with_the_needle_where_the_shared_selector_gives_3():
    import zkwg
    u = _circuit(BODY_UNIQ)
    d = _with_body(45, 0, 150, b"aaab", 100)
    assert d["body"].count(b"aab") == 1
    assert zkwg.generate_inputs_device(u, [d], selector="aab", substrings=[(0, 3)])[1] == [3]
    recs, st = zkwg.generate_inputs_device(u, [d], needles=[b"aab"])
    assert st == [0]
    assert recs[0].cpu().numpy().tobytes() == _mirror(u, BODY_UNIQ, d, b"aab")


def test_raw_emails_to_witnesses_with_nothing_computed_on_the_host():
    """.eml -> DKIM verification on the device -> records from the needles, from the resident batch -> witnesses"""
    import zkwg
    import dkim_cases as cases
    from zkwg import dkim, synth
    emails = [synth.synthetic_raw_email(21, i, 70 + 9 * i) for i in range(3)]
    handle = dkim.verify_batch_device(emails, keys=cases.keys(), device=0)
    assert handle.status == [0, 0, 0]
    results = [synth.synthetic_dkim_result(21, i, 70 + 9 * i) for i in range(3)]      # (what the mirror is given: the same emails' results)
    for shape, needles in (("A", [b"message-id:<"] * 3), (BODY_UNIQ, [r["body"][30 + i:40 + i] for i, r in enumerate(results)])):
        c = _circuit(shape)
        recs, st = zkwg.generate_inputs_device(c, handle, needles=needles)
        assert st == [0, 0, 0]
        raw = recs.cpu().numpy().tobytes()
        assert raw == b"".join(_mirror(c, shape, r, nd) for r, nd in zip(results, needles))
        wit, status = c.calculate_batch_host(raw)
        assert status == [0, 0, 0]
        slot = {nm: s for s, nm in c.symbols()}["main.revealed[0]"]
        for e in range(3):
            v = wit[e * c.witness_bytes + 32 * slot:e * c.witness_bytes + 32 * slot + 32]
            assert v[:len(needles[e])] == needles[e] and v[len(needles[e]):] == bytes(32 - len(needles[e]))


def test_refused_argument_combinations():
    import zkwg
    from zkwg import synth
    a, u = _circuit("A"), _circuit(BODY_UNIQ)
    ds = [synth.synthetic_dkim_result(46, i, body_len=90) for i in range(2)]
    nd = [b"message-id:<"] * 2
    with pytest.raises(zkwg.ZkwgError):
        zkwg.generate_inputs_device(a, ds, needles=nd, substrings=[(0, 1)] * 2)
    ev = zkwg.Circuit(zkwg.MAIN_EMAIL_VERIFIER, max_header=576, max_body=192, device=0)
    with pytest.raises(zkwg.ZkwgError):
        zkwg.generate_inputs_device(ev, ds, needles=nd)
    with pytest.raises(zkwg.ZkwgError):
        zkwg.generate_inputs_device(u, ds, needles=[ds[0]["body"][5:9]] * 2, selector="x")
    with pytest.raises(zkwg.ZkwgError):
        zkwg.generate_inputs_device(a, ds, needles=nd[:1])
    with pytest.raises(zkwg.ZkwgError):
        zkwg.generate_inputs_device(a, ds)                                   # neither: as before
    # a selector beside header needles is the body's as before
    assert zkwg.generate_inputs_device(a, ds, needles=nd, selector=ds[0]["body"][:1].decode())[1][0] == 0
