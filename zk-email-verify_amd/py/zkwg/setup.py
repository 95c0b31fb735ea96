"""python -m zkwg.setup circuit.r1cs pot.ptau circuit.zkey [verification_key.json] -- `snarkjs groth16 setup` (+ `zkey export
verificationkey`) on the device: the step between the witness and the proof of the reference's workflow
(docs/zk-email-docs/UsageGuide/README.md:145-180, "Step 6 ... generate the keys").  The .ptau must be PREPARED (sections 12 - 15); the
key is snarkjs' initial key (gamma = delta = 1, no phase-2 contribution), section 10 is left empty: every prover reads the file,
`snarkjs zkey verify` does not accept it.  C side: zkwg_zkey_new (csrc/zkwg_setup_api.hip, csrc/zkwg_kernels_setup.hip)."""
import argparse
import ctypes as C
import json
import mmap
import sys

from . import _call, _lib

SLICE_NAMES = ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "tau_g1_next")


class SetupError(ValueError):
    pass


def _host_ptr(buf, keep):
    import numpy as np
    a = np.frombuffer(buf, dtype=np.uint8)      # (no copy; works for read-only buffers such as an mmap)
    keep.append(a)
    return a.ctypes.data, a.size


def key_shape(r1cs_bytes):
    """-> (domain power, bytes of the .zkey) of a compiler-format .r1cs"""
    lib = _lib.load()
    power, size = C.c_uint32(), C.c_uint64()
    _call.check(lib, lib.zkwg_zkey_new_size(r1cs_bytes, len(r1cs_bytes), C.byref(power), C.byref(size)), SetupError)
    return power.value, size.value


def new_zkey(r1cs_bytes, ptau_or_slices, device=0):
    """r1cs_bytes: a compiler-format .r1cs.  ptau_or_slices: a prepared .ptau (bytes / memoryview / mmap: read in place), or a dict with
    `power`, the five slices tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1 (2^power points) and tau_g1_next (2^(power + 1) points) -- host
    buffers or torch tensors on the device, all of one kind -- and alpha1, beta1, beta2 (bytes).  -> the .zkey (bytes)"""
    lib = _lib.load()
    power, size = key_shape(r1cs_bytes)
    keep = []
    sl = _lib.SetupSlices()
    if isinstance(ptau_or_slices, dict):
        d = ptau_or_slices
        sl.power = d["power"]
        on_device = [hasattr(d[k], "data_ptr") for k in SLICE_NAMES]
        if any(on_device) != all(on_device):
            raise SetupError("the slices must be all host buffers or all device tensors")
        sl.on_device = 1 if on_device[0] else 0
        for k in SLICE_NAMES:
            want = (128 if k == "tau_g2" else 64) << (sl.power + (1 if k == "tau_g1_next" else 0))
            if on_device[0]:
                ptr, n = d[k].data_ptr(), d[k].numel() * d[k].element_size()
                keep.append(d[k])
            else:
                ptr, n = _host_ptr(d[k], keep)
            if n != want:
                raise SetupError(f"slice {k} holds {n} bytes, a domain of 2^{sl.power} needs {want}")
            setattr(sl, k, ptr)
        for k, n in (("alpha1", 64), ("beta1", 64), ("beta2", 128)):
            if len(d[k]) != n:
                raise SetupError(f"{k} must be {n} bytes")
            C.memmove(getattr(sl, k), bytes(d[k]), n)
    else:
        ptr, n = _host_ptr(ptau_or_slices, keep)
        _call.check(lib, lib.zkwg_ptau_parse(ptr, n, power, C.byref(sl)), SetupError)
    out = (C.c_uint8 * size)()
    out_len = C.c_uint64()
    _call.check(lib, lib.zkwg_zkey_new(device, r1cs_bytes, len(r1cs_bytes), C.byref(sl), out, size, C.byref(out_len)), SetupError)
    return bytes(memoryview(out)[:out_len.value])


def last_stats():
    """seconds and group operations of this thread's last new_zkey (zkwg_zkey_new_stats)"""
    lib = _lib.load()
    sec, ops = (C.c_double * 7)(), (C.c_uint64 * 8)()
    lib.zkwg_zkey_new_stats(sec, ops)
    names = ("parse_plan", "upload_check", "sum_a", "sum_b1", "sum_b2", "sum_k", "h_download")
    return {"seconds": dict(zip(names, sec)), "ops": {n: {"add": ops[2 * i], "dbl": ops[2 * i + 1]} for i, n in enumerate(("a", "b1", "b2", "k"))}}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("r1cs")
    ap.add_argument("ptau")
    ap.add_argument("zkey")
    ap.add_argument("verification_key_json", nargs="?")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    from . import zkey
    r1cs = open(a.r1cs, "rb").read()
    with open(a.ptau, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as mm:
        try:
            z = new_zkey(r1cs, mm, device=a.device)
        except SetupError as e:
            hint = " (run `python -m zkwg.ptau prepare` on the file first)" if "not prepared" in str(e) else ""
            print(f"no key: {e}{hint}", file=sys.stderr)
            return 1
    open(a.zkey, "wb").write(z)
    if a.verification_key_json:
        json.dump(zkey.verification_key(z), open(a.verification_key_json, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
