"""The application main EmailReveal on the device (ZKWG_MAIN_EMAIL_REVEAL: EmailVerifier's roles, zk_substr and zk_app_tail,
csrc/zkwg_kernels_app.hip) against the interpreter's fixtures of tests/golden/email_reveal, against the plain EmailVerifier and
RevealSubstring handles over the same records slot by slot, through the device constraint check, the host expansion, a groth16
proof at the smallest shape, and from a raw email.  All comparisons are exact."""
import random
import struct

import pytest

import emailreveal as er

pytestmark = pytest.mark.gpu

_c = {}


def _circuit(name, device=0):
    import zkwg
    if (name, device) not in _c:
        _c[name, device] = zkwg.Circuit(device=device, **er.circuit_kwargs(name))
    return _c[name, device]


def _with_indices(c, recs, pairs):
    """packed records with (substringStartIndex, substringLength) written into their two u32 fields"""
    out = bytearray(recs)
    off = c.lib.zkwg_input_offset(c.h, 13)
    for e, (a, n) in enumerate(pairs):
        struct.pack_into("<II", out, e * c.in_stride + off, a, n)
    return bytes(out)


def _seeded_batch(c, n, seed):
    """n synthetic emails with seeded (start, length) inside the text of the revealed-from array -> (records, pairs)"""
    from zkwg import synth
    cfg, app = c.cfg, c.app
    recs, fields = synth.packed_batch(c, seed=seed, n=n, body_len=90)
    rng = random.Random(seed)
    src, L = (fields["body"], cfg.max_body) if app.reveal_from_body else (fields["header"], cfg.max_header)
    pairs = []
    for e in range(n):
        used = bytes(src[e * L:(e + 1) * L]).index(b"\x80")          # the text is ASCII: the first byte of the SHA padding ends it
        ln = rng.randrange(1, app.max_substring + 1) if e % 5 else app.max_substring      # short ones are rarely unique: status 4
        pairs.append((rng.randrange(0, used - ln), ln))
    return _with_indices(c, recs, pairs), pairs


def _device_witnesses(c, recs):
    """-> (tensor [n, W, 32] on the device, status list)"""
    import torch
    n = len(recs) // c.in_stride
    d_in = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to("cuda:0")
    d_out = torch.full((n * c.witness_bytes,), 0xA5, dtype=torch.uint8, device="cuda:0")       # an unwritten slot would show
    d_status = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d_scr = torch.empty(c.scratch_bytes(n), dtype=torch.uint8, device="cuda:0")
    c.calculate_batch_device(d_in, n, d_out, d_status, d_scr)
    torch.cuda.synchronize()
    return d_out.view(n, c.W, 32), d_status.cpu().tolist()


@pytest.mark.parametrize("name", tuple(er.SHAPES))
def test_fixture_email_equals_the_interpreter_in_every_slot(name):
    import zkwg
    c = _circuit(name)
    fx = er.load_fixture(name)
    rec = c.pack(fx["inputs"])
    wit, status = c.calculate_batch_host(rec)
    assert status == [0]
    if wit != fx["witness"]:
        j = next(s for s in range(c.W) if wit[32 * s:32 * s + 32] != fx["witness"][32 * s:32 * s + 32])
        raise AssertionError(f"slot {j} ({c.symbols()[j][1]})")
    # the circom_tester surface: calculateWitness, assertOut by output name, the `.wtns` writer
    calc = zkwg.WitnessCalculator(c)
    w = calc.calculateWitness(fx["inputs"])
    N, M, ignore, body, S, uniq, nul = er.SHAPES[name]
    a, ln = int(fx["inputs"]["substringStartIndex"]), int(fx["inputs"]["substringLength"])
    sub = bytes(int(x) for x in fx["inputs"]["emailBody" if body else "emailHeader"])[a:a + ln] + bytes(S - ln)
    c.assertOut(w, {"revealed": [int.from_bytes(sub[31 * i:31 * i + 31], "little") for i in range((S + 30) // 31)], "pubkeyHash": w[1]})
    if nul:
        c.assertOut(w, {"emailNullifier": w[2]})
    with pytest.raises(AssertionError):
        c.assertOut(w, {"revealed": [0] * ((S + 30) // 31)})
    assert calc.calculateWTNSBin(fx["inputs"])[-32 * c.W:] == fx["witness"]
    with pytest.raises(zkwg.ZkwgError, match="Assert Failed"):
        c.calculate_witness(dict(fx["inputs"], substringLength=S + 1))


@pytest.mark.parametrize("name,n", [("A", 139), ("B", 65), ("C", 1), ("B", 139)])
def test_batches_equal_the_plain_handles_slot_by_slot(name, n):
    """the `ev` part against the EmailVerifier handle's witnesses of the same records, the `rs` part against the RevealSubstring
    handle's with in = the header or the body: 65 and 139 are not multiples of a wavefront of emails (64, and 4 for the key hash)"""
    import torch
    import zkwg
    c = _circuit(name)
    cfg, app = c.cfg, c.app
    recs, pairs = _seeded_batch(c, n, seed=1000 + n)
    d_app, st_app = _device_witnesses(c, recs)
    ev = zkwg.Circuit(zkwg.MAIN_EMAIL_VERIFIER, max_header=cfg.max_header, max_body=cfg.max_body, ignore_body_hash_check=cfg.ignore_body_hash_check, device=0)
    assert ev.in_stride == c.in_stride - 16
    ev_recs = b"".join(recs[e * c.in_stride:e * c.in_stride + ev.in_stride] for e in range(n))
    d_ev, st_ev = _device_witnesses(ev, ev_recs)
    L = cfg.max_body if app.reveal_from_body else cfg.max_header
    rs = zkwg.Circuit(zkwg.MAIN_REVEAL_SUBSTRING, max_header=L, max_body=app.max_substring, n=app.check_uniqueness, k=0, device=0)
    src_off = c.lib.zkwg_input_offset(c.h, 1 if app.reveal_from_body else 0)
    rs_recs = bytearray(n * rs.in_stride)
    o = [rs.lib.zkwg_input_offset(rs.h, f) for f in (0, 8, 7)]
    for e, (a, ln) in enumerate(pairs):
        rs_recs[e * rs.in_stride + o[0]:e * rs.in_stride + o[0] + L] = recs[e * c.in_stride + src_off:e * c.in_stride + src_off + L]
        struct.pack_into("<I", rs_recs, e * rs.in_stride + o[1], a)
        struct.pack_into("<I", rs_recs, e * rs.in_stride + o[2], ln)
    d_rs, st_rs = _device_witnesses(rs, bytes(rs_recs))
    assert st_ev == [0] * n and st_app == st_rs and set(st_app) <= {0, 4}
    assert 0 in st_app
    if app.check_uniqueness and n > 1:
        assert 4 in st_app
    app_slot = {nm: s for s, nm in c.symbols()}
    for other, d_other, prefix in ((ev, d_ev, "main.ev."), (rs, d_rs, "main.rs.")):
        pairs_ = [(app_slot[prefix + nm[5:]], s) for s, nm in other.symbols() if prefix + nm[5:] in app_slot]
        # everything under the prefix is there: the handle's sub-component signals (its own I/O is main's I/O in the composition)
        assert len(pairs_) == sum(nm.startswith(prefix) for nm in app_slot)
        ia = torch.tensor([p[0] for p in pairs_], device="cuda:0")
        io = torch.tensor([p[1] for p in pairs_], device="cuda:0")
        assert torch.equal(d_app.index_select(1, ia), d_other.index_select(1, io)), prefix
    # main I/O: the key hash is the plain handle's, the revealed bytes pack the RevealSubstring handle's output
    assert torch.equal(d_app[:, app_slot["main.pubkeyHash"]], d_ev[:, 1])
    S = app.max_substring
    sub = d_rs[:, 1:1 + S, 0].cpu().tolist()
    assert int(d_rs[:, 1:1 + S, 1:].max()) == 0
    got = d_app[:, app_slot["main.revealed[0]"]:app_slot["main.revealed[0]"] + (S + 30) // 31].cpu().numpy()
    for e in range(n):
        for i in range((S + 30) // 31):
            assert int.from_bytes(got[e, i].tobytes(), "little") == int.from_bytes(bytes(sub[e][31 * i:31 * i + 31]), "little"), (e, i)


def test_status_4_leaves_the_neighbours_alone():
    import zkwg
    from zkwg import synth
    c = _circuit("A")
    cfg, app = c.cfg, c.app
    n = 7
    recs, fields = synth.packed_batch(c, seed=77, n=n, body_len=90)
    hdr = [bytes(fields["header"][e * 576:(e + 1) * 576]) for e in range(n)]
    at = [h.index(b"subject:") for h in hdr]
    L, S = cfg.max_header, app.max_substring
    good = [(at[e], 12) for e in range(n)]
    once = hdr[4].index(b"<")                                    # '<' : in from: and in message-id:
    assert hdr[4].count(b"<") == 2
    pairs = list(good)
    pairs[2] = (L - S + 1, S)                                     # start + length = L + 1
    pairs[3] = (at[3], S + 1)                                     # length = S + 1
    pairs[4] = (once, 1)                                          # a one-byte needle that occurs twice
    bad = bytearray(_with_indices(c, recs, pairs))
    bad[1 * c.in_stride + c.lib.zkwg_input_offset(c.h, 4) + 3] ^= 0x10      # a tampered signature
    wit, status = c.calculate_batch_host(bytes(bad))
    assert status == [0, 4, 4, 4, 4, 0, 0]
    ref, st_ref = c.calculate_batch_host(_with_indices(c, recs, good))
    assert st_ref == [0] * n
    wb = c.witness_bytes
    for e in (0, 5, 6):
        assert wit[e * wb:(e + 1) * wb] == ref[e * wb:(e + 1) * wb], e
    # the same needle without the uniqueness check passes
    nu = zkwg.Circuit(device=0, **dict(er.circuit_kwargs("A"), check_uniqueness=0))
    w2, st2 = nu.calculate_batch_host(_with_indices(nu, synth.packed_batch(nu, seed=77, n=n, body_len=90)[0], [good[0]] * 4 + [(once, 1)] + good[5:]))
    assert st2 == [0] * n
    slot = {nm: s for s, nm in nu.symbols()}["main.revealed[0]"]
    assert int.from_bytes(w2[4 * nu.witness_bytes + 32 * slot:4 * nu.witness_bytes + 32 * slot + 32], "little") == ord("<")


def test_device_constraint_check_accepts_the_batch_and_rejects_a_tampered_output():
    import zkwg
    c = _circuit("C")
    n = 5
    recs, pairs = _seeded_batch(c, n, seed=5)
    h0 = c.lib.zkwg_input_offset(c.h, 0)
    pairs = [(recs[e * c.in_stride + h0:(e + 1) * c.in_stride].index(b"message-id:"), 33) for e in range(n)]      # unique in every email
    d_out, status = _device_witnesses(c, _with_indices(c, recs, pairs))
    assert status == [0] * n
    r = zkwg.WitnessCalculator(c).constraint_system()
    assert r.n_wires == c.W and r.n_pub_out == c.n_public == 4
    flat = d_out.view(-1)
    assert r.first_violations_device(flat, n, c.witness_bytes) == [None] * n
    slot = {nm: s for s, nm in c.symbols()}
    for name in ("main.revealed[1]", "main.emailNullifier", "main.anon_EmailNullifier.anon_Poseidon.pEx.sigmaP[3].in4"):
        flat[2 * c.witness_bytes + 32 * slot[name]] ^= 1
        got = r.first_violations_device(flat, n, c.witness_bytes)
        assert got[2] is not None and [g for k, g in enumerate(got) if k != 2] == [None] * (n - 1), name
        flat[2 * c.witness_bytes + 32 * slot[name]] ^= 1
    assert r.first_violations_device(flat, n, c.witness_bytes) == [None] * n


@pytest.mark.parametrize("name", ("A", "B"))
def test_host_expansion_of_the_downloaded_image_equals_the_device_witness(name):
    c = _circuit(name)
    recs, _ = _seeded_batch(c, 6, seed=31)
    wit_dev, st_dev = c.calculate_batch_host(recs, max_tile=4)
    c.set_host_expand(3)
    wit_host, st_host = c.calculate_batch_host(recs, max_tile=4)
    c.set_host_expand(0)
    assert st_host == st_dev and 0 in st_dev
    assert wit_host == wit_dev


def test_existing_mains_compute_what_they_did_before_the_new_main_ran():
    import zkwg
    from zkwg import synth

    def others():
        ev = zkwg.Circuit(zkwg.MAIN_EMAIL_VERIFIER, max_header=576, max_body=192, device=0)
        we, se = ev.calculate_batch_host(synth.packed_batch(ev, seed=3, n=3, body_len=80)[0])
        rs = zkwg.Circuit(zkwg.MAIN_REVEAL_SUBSTRING, max_header=64, max_body=8, n=1, k=0, device=0)
        wr, sr = rs.calculate_batch_host(rs.pack({"in": list(range(1, 65)), "substringStartIndex": 5, "substringLength": 6}))
        assert se == [0, 0, 0] and sr == [0]
        return we, wr, ev.lib.zkwg_inverse_table_half(ev.h), rs.lib.zkwg_inverse_table_half(rs.h), ev.in_stride, rs.in_stride
    before = others()
    for name in ("A", "B"):
        c = zkwg.Circuit(device=0, **er.circuit_kwargs(name))     # a handle of its own: created and destroyed in between
        assert c.calculate_batch_host(c.pack(er.load_fixture(name)["inputs"]))[1] == [0]
        c.close()
    assert others() == before


def test_montgomery_output_is_refused():
    import torch
    import zkwg
    c = _circuit("C")
    rec = c.pack(er.load_fixture("C")["inputs"])
    d_in = torch.frombuffer(bytearray(rec), dtype=torch.uint8).to("cuda:0")
    d_out = torch.zeros(c.witness_bytes, dtype=torch.uint8, device="cuda:0")
    d_status = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    d_scr = torch.empty(c.scratch_bytes(1), dtype=torch.uint8, device="cuda:0")
    c.prepare_device(d_in, 1, d_status, d_scr)
    with pytest.raises(zkwg.ZkwgError):
        c.expand_montgomery_device(d_in, 1, d_scr, 0, 1, d_out)
    torch.cuda.synchronize()


def test_raw_email_to_witness_through_the_device_records():
    """.eml -> DKIM verification on the device -> records generated on the device with the two indices copied in -> witness: the one of
    the record packed on the host from the same email"""
    import zkwg
    import dkim_cases as cases
    from zkwg import dkim, inputs, synth
    c = _circuit("A")
    emails = [synth.synthetic_raw_email(21, i, 70 + 9 * i) for i in range(3)]
    handle = dkim.verify_batch_device(emails, keys=cases.keys(), device=0)
    assert handle.status == [0, 0, 0]
    params = er.reveal_params(er.SHAPES["A"])
    host = [inputs.generate_email_reveal_inputs(m, params, keys=cases.keys(), needle=b"message-id:<", device=-1) for m in emails]
    subs = [(int(h["substringStartIndex"]), int(h["substringLength"])) for h in host]
    recs, st = zkwg.generate_inputs_device(c, handle, substrings=subs)
    assert st == [0, 0, 0]
    with pytest.raises(zkwg.ZkwgError):
        zkwg.generate_inputs_device(c, handle)
    raw = recs.cpu().numpy().tobytes()
    assert raw == b"".join(c.pack(h) for h in host)
    wit, status = c.calculate_batch_host(raw)
    assert status == [0, 0, 0]
    slot = {nm: s for s, nm in c.symbols()}["main.revealed[0]"]
    for e in range(3):
        v = wit[e * c.witness_bytes + 32 * slot:e * c.witness_bytes + 32 * slot + 32]
        assert v[:12] == b"message-id:<" and v[12:] == bytes(20)


def test_end_to_end_prove_verify_at_the_smallest_shape():
    """the exported `.r1cs` of shape C -> powers of tau from generators and one beacon -> new_zkey -> proofs of two device-resident
    witnesses -> verify_each accepts each under its own public signals, rejects one whose revealed[0] was changed; the public signals
    decode to the needle's bytes"""
    import torch
    import zkwg
    from zkwg import prover, ptau, r1cs as zr, setup, verify, zkey
    c = _circuit("C")
    r1cs = zr.email_reveal_r1cs(c.symbols(), *er.SHAPES["C"])
    power = setup.key_shape(r1cs)[0]
    z = setup.new_zkey(r1cs, ptau.prepare(ptau.beacon(ptau.new(power), "beacon", "00ff" * 16, 10)))
    recs, _ = _seeded_batch(c, 2, seed=8)
    h0 = c.lib.zkwg_input_offset(c.h, 0)
    at = [recs[e * c.in_stride + h0:(e + 1) * c.in_stride].index(b"message-id:") for e in range(2)]
    recs = _with_indices(c, recs, [(a, 33) for a in at])
    d_out, status = _device_witnesses(c, recs)
    assert status == [0, 0]
    wp = prover.WitnessProver(z, device=0, slots=2)
    assert wp.n_public == c.n_public == 4 and wp.n_vars == c.W
    rng = random.Random(9)
    st_p, proofs = wp.prove(d_out.view(-1), [(rng.randrange(zr.P), rng.randrange(zr.P)) for _ in range(2)])
    assert st_p == [0, 0]
    wit = d_out.cpu().numpy().tobytes()
    pubs = [wp.public_signals(wit[k * c.witness_bytes:(k + 1) * c.witness_bytes]) for k in range(2)]
    for k in range(2):
        needle = recs[k * c.in_stride + h0 + at[k]:k * c.in_stride + h0 + at[k] + 33]
        assert needle.startswith(b"message-id:<")
        assert int(pubs[k][2]).to_bytes(31, "little") + int(pubs[k][3]).to_bytes(31, "little")[:2] == needle
    # one key; two signatures, two message ids; the last two revealed bytes ("am" of "@example") are the same
    assert pubs[0][0] == pubs[1][0] and pubs[0][1] != pubs[1][1] and pubs[0][2] != pubs[1][2] and pubs[0][3] == pubs[1][3]
    vk = zkey.verification_key(z)
    pj = [prover.Prover.proof_json(p) for p in proofs]
    forged = list(pubs[0])
    forged[2] = str(int(forged[2]) ^ 1)
    assert verify.verify_each(vk, [pubs[0], pubs[1], forged, pubs[0]], [pj[0], pj[1], pj[0], pj[1]], device=0) == [True, True, False, False]
