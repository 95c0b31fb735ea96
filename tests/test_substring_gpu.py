"""The substring mains on the device: RevealSubstring(L, S, uniq) / CountSubstringOccurrences(L, S) through zk_substr and
zk_expand3_subm (csrc/zkwg_kernels_substr.hip) against the fixtures of tests/golden/substring -- what the circom interpreter computes
from the reference's own templates (tests/golden/make_substring_fixtures.py): reveal-substring.test.ts,
count-substring-occurrences.test.ts, the project's edge cases and a seeded batch of 130.  All comparisons are exact."""
import random

import pytest

import substrtest as st

pytestmark = pytest.mark.gpu

BATCH = (st.REVEAL, 64, 8, 1)


def _circuit(shape, device=0):
    import zkwg
    return zkwg.Circuit(device=device, **st.circuit_kwargs(*shape))


def _check_batch(c, fx, idx, max_tile=0):
    recs = b"".join(c.pack(fx["cases"][i][1]) for i in idx)
    wit, status = c.calculate_batch_host(recs, max_tile=max_tile)
    assert status == [fx["cases"][i][2] for i in idx]
    wb = c.witness_bytes
    for k, i in enumerate(idx):
        if status[k] == 0:
            got, exp = wit[k * wb:(k + 1) * wb], fx["witness"][i]
            if got != exp:
                j = next(s for s in range(c.W) if got[32 * s:32 * s + 32] != exp[32 * s:32 * s + 32])
                raise AssertionError(f"{fx['cases'][i][0]}: slot {j} ({c.symbols()[j][1]})")


@pytest.mark.parametrize("shape", st.SHAPES)
def test_every_fixture_case_equals_the_interpreter_in_every_slot(shape):
    import zkwg
    c = _circuit(shape)
    fx = st.load_fixture(*shape)
    n = len(fx["cases"])
    _check_batch(c, fx, list(range(n)))                    # the whole file as one batch (130 + 9 emails for the seeded shape)
    _check_batch(c, fx, [0])                               # a batch of one
    if shape == BATCH:
        _check_batch(c, fx, list(range(9, 9 + 65)))        # 65: one email past a full wavefront of emails
        _check_batch(c, fx, list(range(n)), max_tile=48)   # ragged tiles
    calc = zkwg.WitnessCalculator(c)
    for name, inp, status in fx["cases"][:12]:
        if status:
            with pytest.raises(zkwg.ZkwgError, match="Assert Failed"):
                c.calculate_witness(inp)
    ok = next(i for i, cs in enumerate(fx["cases"]) if cs[2] == 0)
    assert calc.calculateBinWitness(fx["cases"][ok][1]) == fx["witness"][ok]


def test_device_constraint_check_accepts_the_batch_and_rejects_a_tampered_witness():
    import torch
    import zkwg
    c = _circuit(BATCH)
    fx = st.load_fixture(*BATCH)
    batch = [i for i, cs in enumerate(fx["cases"]) if cs[0].startswith("batch_")]
    assert len(batch) == 130
    n = len(batch)
    r = zkwg.WitnessCalculator(c).constraint_system()
    recs = b"".join(c.pack(fx["cases"][i][1]) for i in batch)
    d_in = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to("cuda:0")
    d_out = torch.full((n * c.witness_bytes,), 0xA5, dtype=torch.uint8, device="cuda:0")    # an unwritten slot would read >= r
    d_status = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d_scr = torch.empty(c.scratch_bytes(n), dtype=torch.uint8, device="cuda:0")
    c.calculate_batch_device(d_in, n, d_out, d_status, d_scr)
    torch.cuda.synchronize()
    status = d_status.cpu().tolist()
    assert status == [fx["cases"][i][2] for i in batch] and 4 * status.count(0) >= 3 * n
    bad = r.first_violations_device(d_out, n, c.witness_bytes)
    assert all(b is None for b, s in zip(bad, status) if s == 0)
    slot_of = {nm: s for s, nm in c.symbols()}
    e = status.index(0)
    for name in ("main.countSubstringOccurrences.matches[5].difference[2]", "main.countSubstringOccurrences.matches[5].matchAccumulator[1]",
                 "main.selectSubArray.shifter.tmp[70]"):
        d_out[e * c.witness_bytes + 32 * slot_of[name]] ^= 1
        got = r.first_violations_device(d_out, n, c.witness_bytes)
        assert got[e] is not None and all(g is None for k, (g, s) in enumerate(zip(got, status)) if s == 0 and k != e), name
        d_out[e * c.witness_bytes + 32 * slot_of[name]] ^= 1
    assert r.first_violations_device(d_out, n, c.witness_bytes)[e] is None


def test_host_expansion_of_the_downloaded_image_equals_the_device_witness():
    shape = (st.REVEAL, 192, 12, 1)
    c = _circuit(shape)
    fx = st.load_fixture(*shape)
    recs = b"".join(c.pack(inp) for _, inp, _ in fx["cases"])
    wit_dev, st_dev = c.calculate_batch_host(recs, max_tile=4)
    c.set_host_expand(3)
    wit_host, st_host = c.calculate_batch_host(recs, max_tile=4)
    c.set_host_expand(0)
    assert st_host == st_dev == [s for _, _, s in fx["cases"]]
    wb = c.witness_bytes
    for i, s in enumerate(st_dev):
        if s == 0:
            assert wit_host[i * wb:(i + 1) * wb] == wit_dev[i * wb:(i + 1) * wb] == fx["witness"][i], i


def test_existing_mains_compute_what_they_did_before_the_new_mains_ran():
    """the inverse table and max_small are per handle: an FpMul and a Sha256Bytes witness before and after the substring mains"""
    import zkwg
    from conftest import sha_pad

    def others():
        f = zkwg.Circuit(zkwg.MAIN_FP_MUL, max_header=0, max_body=0, n=2, k=4, device=0)
        wf, sf = f.calculate_batch_host(f.pack({"a": [1, 0, 1, 0], "b": [0, 1, 1, 0], "p": [1, 1, 1, 1]}))
        s = zkwg.Circuit(zkwg.MAIN_SHA256_BYTES, max_header=128, max_body=0, device=0)
        p, n = sha_pad(b"hello world", 128)
        ws, ss = s.calculate_batch_host(s.pack({"paddedIn": list(p), "paddedInLength": n}))
        assert sf == ss == [0]
        return wf, ws, f.lib.zkwg_inverse_table_half(f.h), s.lib.zkwg_inverse_table_half(s.h)
    before = others()
    for shape in ((st.COUNT, 192, 12, 0), BATCH):
        c = _circuit(shape)
        fx = st.load_fixture(*shape)
        _check_batch(c, fx, list(range(4)))
    assert others() == before
    # fp-mul.test.ts:34-46: out = 0
    assert [int.from_bytes(before[0][32 * i:32 * i + 32], "little") for i in range(1, 5)] == [0, 0, 0, 0]


def test_montgomery_output_is_refused():
    import torch
    import zkwg
    c = _circuit(BATCH)
    fx = st.load_fixture(*BATCH)
    rec = c.pack(fx["cases"][0][1])
    d_in = torch.frombuffer(bytearray(rec), dtype=torch.uint8).to("cuda:0")
    d_out = torch.zeros(c.witness_bytes, dtype=torch.uint8, device="cuda:0")
    d_status = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    d_scr = torch.empty(c.scratch_bytes(1), dtype=torch.uint8, device="cuda:0")
    c.prepare_device(d_in, 1, d_status, d_scr)
    with pytest.raises(zkwg.ZkwgError):
        c.expand_montgomery_device(d_in, 1, d_scr, 0, 1, d_out)
    torch.cuda.synchronize()


def test_end_to_end_reveal_prove_verify():
    """python -m zkwg.r1cs's system -> powers of tau from generators and one beacon -> prepare -> new_zkey -> proofs of two device witnesses ->
    verify_each: each under its own public signals (the 8 revealed bytes), not under the other's"""
    import zkwg
    from zkwg import prover, ptau, r1cs as zr, setup, verify, zkey
    L, S = 64, 8
    c = _circuit(BATCH)
    sym = c.symbols()
    cons = zr.reveal_substring_main_constraints(sym, L, S, 1)
    r1cs = zr.write_r1cs(c.W, cons, n_pub_out=S, n_pub_in=0, n_prv_in=L + 2)
    assert c.n_public == S
    power = setup.key_shape(r1cs)[0]
    assert (1 << power) >= len(cons) + S + 1 > (1 << (power - 1))          # the smallest sufficient power
    # (the powers of ptau.new alone are those of tau = 1: every Lagrange point but one is the point at infinity; one beacon moves tau)
    z = setup.new_zkey(r1cs, ptau.prepare(ptau.beacon(ptau.new(power), "beacon", "00ff" * 16, 10)))
    fx = st.load_fixture(*BATCH)
    ok = [i for i, cs in enumerate(fx["cases"]) if cs[0].startswith("batch_") and cs[2] == 0][:2]
    recs = b"".join(c.pack(fx["cases"][i][1]) for i in ok)
    wit, status = c.calculate_batch_host(recs)
    assert status == [0, 0]
    wb = c.witness_bytes
    wp = prover.WitnessProver(z, device=0, slots=2)
    rng = random.Random(9)
    R = zr.P
    st_p, proofs = wp.prove(wit, [(rng.randrange(R), rng.randrange(R)) for _ in ok])
    assert st_p == [0, 0]
    pubs = [wp.public_signals(wit[k * wb:(k + 1) * wb]) for k in range(2)]
    for k, i in enumerate(ok):
        inp = fx["cases"][i][1]
        a, n = inp["substringStartIndex"], inp["substringLength"]
        assert pubs[k] == [str(v) for v in inp["in"][a:a + n] + [0] * (S - n)]
    assert pubs[0] != pubs[1]
    vk = zkey.verification_key(z)
    pj = [prover.Prover.proof_json(p) for p in proofs]
    assert verify.verify_each(vk, [pubs[0], pubs[1], pubs[0]], [pj[0], pj[1], pj[1]], device=0) == [True, True, False]
