"""A witness handle gives back everything it took: create, use, destroy, repeatedly, and the device's free memory stays put.
Every device buffer, pinned buffer, stream, event and the chunk-mapped output ring of a handle belongs to an owner in
csrc/zkwg_handle.h; zkwg_circuit_destroy only deletes the handle.

One cycle = create the handle, one calculate_batch of 4 emails (the cached staging of the host-buffer path), where the main
allows it one Montgomery-form expansion (the lazily built table pair) and one attach_r1cs + expand_abc_device (the attached
tables; it also drops and re-sizes the staging), one calculate_batch_resident (the resident buffers and the chunk-mapped
ring) and destroy WITHOUT zkwg_resident_release.  The records are valid inputs of the kind.  The substring mains and EmailReveal refuse Montgomery output and
attach_r1cs; a regex handle and a numbered handle have no constraint system of the built-in layout to attach.

Bound: after one warm-up cycle, CYCLES more cycles may lower torch.cuda.mem_get_info()'s free bytes by less than one
4 KiB page per cycle -- 4 KiB is the smallest unit a device allocation takes, so one forgotten hipFree per cycle cannot hide
under it.  No torch allocation happens between the readings (the device buffers of the test are allocated before the first)."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAND_IN = os.path.join(ROOT, "oracle", "circom", "lib", "@zk-email", "zk-regex-circom", "circuits", "common", "body_hash_regex.circom")
O0 = os.path.join(ROOT, "artifacts", "o0_ev_576_192")
N_EMAILS = 4
CYCLES = 4
PAGE = 4096


def _kinds():
    import zkwg
    import emailreveal as er
    ev = dict(main_kind=zkwg.MAIN_EMAIL_VERIFIER, max_header=576, max_body=192)
    return {
        "email_verifier": (ev, True, True),
        "remove_soft_line_breaks": (dict(ev, remove_soft_line_breaks=1), True, True),
        "both_masks": (dict(ev, enable_header_masking=1, enable_body_masking=1), True, True),
        "regex_stand_in": (dict(ev, regex=STAND_IN), True, False),
        "email_reveal_nullifier": (er.circuit_kwargs("A"), False, False),
        "reveal_substring": (dict(main_kind=zkwg.MAIN_REVEAL_SUBSTRING, max_header=64, max_body=8, n=1, k=0), False, False),
        "fp_mul": (dict(main_kind=zkwg.MAIN_FP_MUL, max_header=0, max_body=0, n=2, k=4), True, True),
        "numbered_o0": (dict(ev), True, False),
    }


def _records(kind, c):
    """N_EMAILS valid packed records of the kind, from the inputs the other GPU tests use"""
    if kind == "email_reveal_nullifier":
        import emailreveal as er
        return c.pack(er.synthetic_inputs("A")) * N_EMAILS
    if kind == "reveal_substring":
        import substrtest as st
        fx = st.load_fixture(st.REVEAL, 64, 8, 1)
        return b"".join(c.pack(fx["cases"][i][1]) for i in range(N_EMAILS))
    if kind == "fp_mul":
        return c.pack({"a": [1, 0, 1, 0], "b": [0, 1, 1, 0], "p": [1, 1, 1, 1]}) * N_EMAILS
    from zkwg import synth
    return synth.packed_batch(c, seed=77, n=N_EMAILS, body_len=100)[0]


KINDS = ["email_verifier", "remove_soft_line_breaks", "both_masks", "regex_stand_in", "email_reveal_nullifier", "reveal_substring",
         "fp_mul", "numbered_o0"]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_handle_returns_its_device_memory(kind):
    import torch
    import zkwg
    kw, mont, attach = _kinds()[kind]
    cycles = CYCLES
    if kind == "numbered_o0":
        files = {e: os.path.join(O0, "main." + e) for e in ("sym", "r1cs")}
        if not all(os.path.exists(p) for p in files.values()):
            pytest.skip("artifacts/o0_ev_576_192 is not built")
        kw = dict(kw, sym=open(files["sym"]).read(), r1cs=open(files["r1cs"], "rb").read())
        cycles = 2
    # everything the cycles need from outside the handle, before the first reading
    lay = zkwg.Circuit(device=-1, **{k: v for k, v in kw.items() if k not in ("sym", "r1cs")})
    cs_data = zkwg.WitnessCalculator(lay).constraint_system().data if attach else None
    probe = zkwg.Circuit(device=0, **kw)
    records = _records(kind, probe)
    assert len(records) == N_EMAILS * probe.in_stride
    if attach:
        probe.attach_r1cs(cs_data)
    dev = torch.device("cuda:0")
    d_in = torch.frombuffer(bytearray(records), dtype=torch.uint8).to(dev)
    d_status = torch.zeros(N_EMAILS, dtype=torch.int32, device=dev)
    d_scr = torch.zeros(probe.scratch_bytes(N_EMAILS) + 256, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(N_EMAILS * max(probe.witness_bytes, probe.abc_bytes) + 256, dtype=torch.uint8, device=dev)
    probe.close()
    del probe

    def cycle():
        c = zkwg.Circuit(device=0, **kw)
        c.calculate_batch_host(records)
        if mont:
            c.prepare_device(d_in, N_EMAILS, d_status, d_scr)
            c.expand_montgomery_device(d_in, N_EMAILS, d_scr, 0, N_EMAILS, d_out)
        if attach:
            c.attach_r1cs(cs_data)
            c.prepare_device(d_in, N_EMAILS, d_status, d_scr)
            c.expand_abc_device(d_in, N_EMAILS, d_scr, 0, N_EMAILS, d_out)
        torch.cuda.synchronize()
        c.calculate_batch_resident(records)
        c.close()      # zkwg_circuit_destroy, without zkwg_resident_release

    cycle()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(cycles):
        cycle()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    print(f"{kind}: free after warm-up {free0}, after {cycles} more cycles {free1}, drift {free0 - free1} bytes")
    assert free0 - free1 < cycles * PAGE
