"""Test-only helpers of the substring mains (RevealSubstring, CountSubstringOccurrences): the host build of
csrc/zkwg_substr_core.h (tests/native/substrtest.cpp), the fixtures under tests/golden/substring and their value coding."""
import ctypes as C
import hashlib
import json
import os
import zlib

import numpy as np

import nativelib
from conftest import ROOT

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
GOLDEN = os.path.join(ROOT, "tests", "golden", "substring")
REVEAL, COUNT = 4, 5          # include/zkwg.h ZKWG_MAIN_REVEAL_SUBSTRING, ZKWG_MAIN_COUNT_SUBSTRING
# (main kind, maxLength, maxSubstringLength, shouldCheckUniqueness) of every fixture file
SHAPES = ((REVEAL, 256, 16, 1), (COUNT, 1024, 128, 0), (REVEAL, 192, 12, 1), (REVEAL, 192, 12, 0), (COUNT, 192, 12, 0),
          (COUNT, 12, 12, 0), (REVEAL, 64, 8, 1))
# A fixture stores one int64 per slot: every value of these circuits is a small integer v (code v), the negative of one
# (code -m for r - m) or the inverse of a small signed integer d (code INV + d)
INV = 1 << 40


def fixture_name(kind, L, S, u):
    return f"reveal_{L}_{S}_{u}.npz" if kind == REVEAL else f"count_{L}_{S}.npz"


def encode(v, inv_of=None):
    if inv_of is not None and inv_of != 0:
        d = inv_of if inv_of < P // 2 else inv_of - P
        assert abs(d) < 1 << 30 and v == pow(inv_of, P - 2, P)
        return INV + d
    c = v if v < P // 2 else v - P
    assert abs(c) < 1 << 39
    return c


def decode(c):
    c = int(c)
    if c >= INV // 2:
        return pow((c - INV) % P, P - 2, P)
    return c % P


def witness_bytes(codes):
    return b"".join(decode(c).to_bytes(32, "little") for c in codes)


def circuit_kwargs(kind, L, S, u):
    return dict(main_kind=kind, max_header=L, max_body=S, n=u, k=0)


_fx = {}


def load_fixture(kind, L, S, u):
    """-> dict(cases = [(name, inputs, status)], witness = {case index: bytes} (status-0 cases), o0_index, sym_sha256)"""
    key = (kind, L, S, u)
    if key not in _fx:
        z = np.load(os.path.join(GOLDEN, fixture_name(*key)))
        cases = json.loads(bytes(z["cases"]).decode())
        W = int(z["W"][0])
        codes = np.frombuffer(zlib.decompress(bytes(z["witness"])), dtype="<i8")
        ok = [i for i, c in enumerate(cases) if c["status"] == 0]
        assert len(codes) == W * len(ok)
        cache = {}
        wit = {}
        for k, i in enumerate(ok):
            row = codes[k * W:(k + 1) * W]
            out = bytearray(32 * W)
            for j, c in enumerate(row.tolist()):
                if c:
                    b = cache.get(c)
                    if b is None:
                        b = cache[c] = decode(c).to_bytes(32, "little")
                    out[32 * j:32 * j + 32] = b
            wit[i] = bytes(out)
        _fx[key] = dict(cases=[(c["name"], c["inputs"], c["status"]) for c in cases], witness=wit, W=W,
                        o0_index=np.cumsum(np.frombuffer(zlib.decompress(bytes(z["o0_index"])), dtype="<u4"), dtype=np.uint64), sym_sha256=bytes(z["sym_sha256"]).decode())
    return _fx[key]


def sym_hash(symbols):
    return hashlib.sha256("\n".join(n for _, n in symbols).encode()).hexdigest()


class Cfg(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("main_kind", "max_header", "max_body", "n", "k", "ignore_body_hash_check",
                                          "enable_header_masking", "enable_body_masking", "remove_soft_line_breaks", "layout")]


def load():
    lib = nativelib.build("substrtest")
    lib.st_create.restype = C.c_void_p
    lib.st_create.argtypes = [C.c_void_p]
    lib.st_destroy.argtypes = [C.c_void_p]
    lib.st_sizes.argtypes = [C.c_void_p, C.c_void_p]
    lib.st_run.restype = C.c_int
    lib.st_run.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p]
    return lib


def host_images(circuit, records):
    """zkwg_substr_core.h on the host over packed records -> (scratch buffer in the layout zkwg_expand_host reads, statuses)"""
    lib = load()
    cfg = circuit.cfg
    h = lib.st_create(C.byref(Cfg(cfg.main_kind, cfg.max_header, cfg.max_body, cfg.n, cfg.k, 0, 0, 0, 0, 0)))
    assert h
    try:
        sizes = (C.c_uint32 * 4)()
        lib.st_sizes(h, sizes)
        n = len(records) // circuit.in_stride
        lay = circuit.image_layout(n)
        assert (sizes[0], sizes[1], sizes[2]) == (lay["bits_words"], lay["small_words"], circuit.in_stride)
        scr = (C.c_uint8 * lay["total_bytes"])()
        base = C.addressof(scr)
        status = []
        for e in range(n):
            rec = records[e * circuit.in_stride:(e + 1) * circuit.in_stride]
            status.append(lib.st_run(h, rec, C.c_void_p(base + lay["off_bits"] + 8 * sizes[0] * e),
                                     C.c_void_p(base + lay["off_small"] + 4 * sizes[1] * e)))
        return scr, status
    finally:
        lib.st_destroy(h)
