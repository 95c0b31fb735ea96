"""What the key-ceremony modules (phase2, ptau, setup, pairing) call libzkwg.so with: the refusal of a return code, the encodings of a
scalar and of a base-field element, bytes to a device tensor and back, and the size / allocate / fill sequence of a file operation.
torch and numpy are imported inside the functions that need them: a module that imports this one imports neither."""
import ctypes as C

from .zkey import Q

BAD_CONFIG = -1                                   # ZKWG_RC_BAD_CONFIG: the one code zkwg_last_error has a message for


def check(lib, rc, Error):
    """raises Error("<zkwg_strerror>[: <zkwg_last_error>]") unless rc is 0"""
    if rc != 0:
        msg = lib.zkwg_last_error().decode() if rc == BAD_CONFIG else ""
        raise Error(f"{lib.zkwg_strerror(rc).decode()}{': ' + msg if msg else ''}")


def le32(v):
    """an integer (taken modulo 2^256) as the 32 little-endian bytes of a scalar argument"""
    return int(v % (1 << 256)).to_bytes(32, "little")


def mont(v):
    """an element of the base field in the zkey's form: little-endian Montgomery words"""
    return ((v << 256) % Q).to_bytes(32, "little")


def upload(data, device):
    """bytes (or any buffer) -> a uint8 tensor on cuda:device"""
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(torch.device("cuda", device))


def download(tensor):
    return bytes(tensor.cpu().numpy())


def sized_call(size_fn, fill_fn, data):
    """a file operation over `data` (bytes, or an mmap: read in place, no copy): size_fn(ptr, len, byref(bytes needed)), then
    fill_fn(ptr, len, out ptr, capacity, byref(bytes written)), both -> rc.  -> (rc, the output as bytes or None)"""
    import numpy as np
    a = np.frombuffer(data, dtype=np.uint8)
    size, out_len, out = C.c_uint64(), C.c_uint64(), None
    try:
        rc = size_fn(a.ctypes.data, a.size, C.byref(size))
        if rc == 0:
            out = np.empty(size.value, dtype=np.uint8)
            rc = fill_fn(a.ctypes.data, a.size, out.ctypes.data, size.value, C.byref(out_len))
    finally:
        del a                                      # (an mmap cannot be closed while a view of it lives, e.g. in a traceback)
    return rc, (out[:out_len.value].tobytes() if rc == 0 else None)
