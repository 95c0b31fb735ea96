"""Test-only helpers of the application main EmailReveal (zk-email-verify_amd/circuits/email-reveal.circom): the shapes, the
synthetic inputs, the fixtures under tests/golden/email_reveal, and the host build of csrc/zkwg_app_core.h with
csrc/zkwg_substr_core.h (tests/native/apptest.cpp)."""
import ctypes as C
import hashlib
import json
import os
import zlib

import numpy as np

import nativelib
from conftest import ROOT

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
GOLDEN = os.path.join(ROOT, "tests", "golden", "email_reveal")
CIRCOM = os.path.join(ROOT, "zk-email-verify_amd", "circuits", "email-reveal.circom")
EMAIL_REVEAL = 6        # include/zkwg.h ZKWG_MAIN_EMAIL_REVEAL
# (maxHeadersLength, maxBodyLength, ignoreBodyHashCheck, revealFromBody, maxSubstringLength, shouldCheckUniqueness, withNullifier):
# the smallest at which each part can go wrong -- 576 is the smallest header that holds the synthetic headers; B has two packed
# outputs, the second partial, and no match matrix (the plain expansion kernel); C has no body
SHAPES = {"A": (576, 192, 0, 0, 12, 1, 1), "B": (576, 192, 0, 1, 40, 0, 0), "C": (576, 0, 1, 0, 33, 1, 1)}


def circuit_kwargs(name_or_shape):
    N, M, ignore, body, S, uniq, nul = SHAPES.get(name_or_shape, name_or_shape)
    return dict(main_kind=EMAIL_REVEAL, max_header=N, max_body=M, ignore_body_hash_check=ignore, reveal_from_body=body,
                max_substring=S, check_uniqueness=uniq, with_nullifier=nul)


def reveal_params(shape):
    N, M, ignore, body, S, uniq, nul = shape
    return {"maxHeadersLength": N, "maxBodyLength": M, "ignoreBodyHashCheck": ignore, "revealFromBody": body, "shouldCheckUniqueness": uniq}


def synthetic_inputs(name):
    """the CircuitInput of shape `name` over synthetic email 0 (zkwg.synth seed 7, body of 60 bytes)"""
    from zkwg import synth, inputs
    shape = SHAPES[name]
    d = synth.synthetic_dkim_result(7, 0, body_len=60)
    h = d["headers"]
    if name == "A":          # "subject:" and the first four letters of the subject
        at = h.index(b"subject:")
        sel = dict(needle=h[at:at + 12])
    elif name == "B":        # 35 bytes of the body: 31 + 4, the second packed output is partial; shorter than S = 40
        sel = dict(start=3, length=35)
    else:                    # the whole message-id field name, its bracket and 21 bytes of the id: S = 33 bytes, two outputs
        at = h.index(b"message-id:")
        sel = dict(needle=h[at:at + 33])
    return inputs.generate_email_reveal_inputs_from_dkim_result(d, reveal_params(shape), **sel)


def sym_hash(symbols):
    return hashlib.sha256("\n".join(n for _, n in symbols).encode()).hexdigest()


_fx = {}


def load_fixture(name):
    """-> dict(inputs, o0_index (per kept-v1 slot), witness (bytes, kept-v1 SLOT order), n_o0, dropped = [(count, pattern)], sym_sha256)"""
    if name not in _fx:
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        o0 = np.cumsum(np.frombuffer(zlib.decompress(bytes(z["o0_index"])), dtype="<i4").astype(np.int64))
        raw = zlib.decompress(bytes(z["witness"]))
        W = len(o0)
        assert len(raw) == 32 * W
        # the stored witness is in interpreter order: slot s holds the element of rank(o0[s])
        rank = np.empty(W, dtype=np.int64)
        rank[np.argsort(o0, kind="stable")] = np.arange(W)
        by_slot = np.frombuffer(raw, dtype=np.uint8).reshape(W, 32)[rank]
        dropped = [(int(l.split()[0]), l.split()[1]) for l in bytes(z["dropped"]).decode().splitlines()]
        _fx[name] = dict(inputs=json.loads(bytes(z["inputs"]).decode()), o0_index=o0, witness=by_slot.tobytes(), W=W,
                         n_o0=int(z["n_o0"][0]), dropped=dropped, sym_sha256=bytes(z["sym_sha256"]).decode())
    return _fx[name]


def ints(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


class Cfg(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("main_kind", "max_header", "max_body", "n", "k", "ignore_body_hash_check",
                                          "enable_header_masking", "enable_body_masking", "remove_soft_line_breaks", "layout")]


class App(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("reveal_from_body", "max_substring", "check_uniqueness", "with_nullifier")]


def load():
    lib = nativelib.build("apptest")
    lib.at_create.restype = C.c_void_p
    lib.at_create.argtypes = [C.c_void_p, C.c_void_p]
    lib.at_destroy.argtypes = [C.c_void_p]
    lib.at_sizes.argtypes = [C.c_void_p, C.c_void_p]
    lib.at_run.restype = C.c_int
    lib.at_run.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def host_images(circuit, records):
    """zkwg_substr_core.h and zkwg_app_core.h on the host over packed records -> (scratch buffer in the layout zkwg_expand_host
    reads, statuses of the RevealSubstring part).  EmailVerifier's own words stay zero: they have no host build."""
    lib = load()
    cfg, app = circuit.cfg, circuit.app
    h = lib.at_create(C.byref(Cfg(cfg.main_kind, cfg.max_header, cfg.max_body, cfg.n, cfg.k, cfg.ignore_body_hash_check, 0, 0, 0, 0)),
                      C.byref(App(app.reveal_from_body, app.max_substring, app.check_uniqueness, app.with_nullifier)))
    assert h
    try:
        sizes = (C.c_uint32 * 4)()
        lib.at_sizes(h, sizes)
        n = len(records) // circuit.in_stride
        lay = circuit.image_layout(n)
        assert (sizes[0], sizes[1], sizes[2], sizes[3]) == (lay["bits_words"], lay["small_words"], lay["fr_elems"], circuit.in_stride)
        scr = (C.c_uint8 * lay["total_bytes"])()
        base = C.addressof(scr)
        status = []
        for e in range(n):
            rec = records[e * circuit.in_stride:(e + 1) * circuit.in_stride]
            status.append(lib.at_run(h, rec, C.c_void_p(base + lay["off_bits"] + 8 * sizes[0] * e),
                                     C.c_void_p(base + lay["off_small"] + 4 * sizes[1] * e), C.c_void_p(base + lay["off_fr"] + 32 * sizes[2] * e)))
        return scr, status
    finally:
        lib.at_destroy(h)
