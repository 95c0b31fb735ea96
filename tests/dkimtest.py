"""Test-only helpers of DKIM verification of raw emails: the host build of csrc/zkwg_dkim_host.h and csrc/zkwg_dkim_core.h
(tests/native/dkimtest.cpp) -- the parser, the serial cores of the device = -1 path, and the bodies of zk_dkim_body and zk_dkim_verify on
the simulated wavefront of tests/native/wavesim.h."""
import ctypes as C
import os
import subprocess

import nativelib

RELAXED, SIMPLE = 0, 1


def load():
    lib = nativelib.build("dkimtest", extra_includes=(nativelib.NATIVE,))
    u64, u32, vp = C.c_uint64, C.c_uint32, C.c_void_p
    lib.dt_parse.restype = C.c_int
    lib.dt_parse.argtypes = [C.c_char_p, u64, C.c_char_p, vp, u32, vp]
    for f in (lib.dt_body_serial, lib.dt_body_wave):
        f.restype = u32
        f.argtypes = [C.c_char_p, u32, u32, C.c_int, u64, vp, u32, C.POINTER(u32)]
    lib.dt_sha256.restype = None
    lib.dt_sha256.argtypes = [C.c_char_p, u32, vp]
    for f in (lib.dt_rsa_host, lib.dt_rsa_wave):
        f.restype = C.c_int
        f.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p]
    lib.dt_tile.restype = u32
    return lib


def tile():
    return load().dt_tile()


def parse(raw, domain="", header_cap=4096):
    """-> (status, canonical header bytes, zkwg._lib.DkimParsed)"""
    from zkwg._lib import DkimParsed
    P = DkimParsed()
    hdr = (C.c_uint8 * header_cap)()
    st = load().dt_parse(raw, len(raw), domain.encode(), hdr, header_cap, C.byref(P))
    return st, bytes(hdr[:P.header_len]) if st == 0 else b"", P


def body(raw, mode, l=None, stride=None, wave=False, fill=0xA5):
    """the canonical body by the serial core or by the wavefront core -> (length, fits, the whole row of `stride` bytes, pre-filled with
    `fill` so that a store beyond the length shows)"""
    stride = 2 * len(raw) + 2 if stride is None else stride
    out = (C.c_uint8 * max(1, stride))(*([fill] * max(1, stride)))
    fits = C.c_uint32(0)
    f = load().dt_body_wave if wave else load().dt_body_serial
    n = f(raw, len(raw), mode, 0 if l is None else 1, l or 0, out, stride, C.byref(fits))
    assert n != 0xffffffff, "the lanes disagree"
    return n, fits.value, bytes(out[:stride])


def sha256(data):
    out = (C.c_uint8 * 32)()
    load().dt_sha256(data, len(data), out)
    return bytes(out)


def rsa(modulus, signature, digest, wave=False):
    f = load().dt_rsa_wave if wave else load().dt_rsa_host
    return f(int(modulus).to_bytes(256, "big"), int(signature).to_bytes(256, "big"), digest)


def build_sanitized_program(out_path):
    """tests/native/dkimtest.cpp as a stand-alone program (its own main) under AddressSanitizer and UBSan -> out_path"""
    src = os.path.join(nativelib.NATIVE, "dkimtest.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-DDKIMTEST_MAIN",
                           "-I", nativelib.CSRC, src, "-o", out_path])
    return out_path
