"""Test-only helpers of the CleanEmailAddress main (utils/email.circom:16-140, include/zkwg.h ZKWG_MAIN_CLEAN_EMAIL_ADDRESS): the host
build of csrc/zkwg_cea_core.h (tests/native/ceatest.cpp), the fixtures under tests/golden/clean_address and their value coding.

A fixture (tests/golden/make_clean_address_fixtures.py) holds per case one int64 code per slot: the small-value codes of
tests/substrtest.py, FR for a field-valued slot stored in full (array `fr`, 32 bytes each, case order then slot order), HS for a slot
inside one of rHasher's Poseidon components of which only the SHA-256 over the component's slots is stored (array `comp_sha`).  The
shape L = 8 stores every slot in full."""
import ctypes as C
import hashlib
import json
import os
import zlib

import numpy as np

import nativelib
from conftest import ROOT
from substrtest import INV, P, Cfg, decode, encode, sym_hash  # noqa: F401  (the value coding is the substring fixtures')

GOLDEN = os.path.join(ROOT, "tests", "golden", "clean_address")
MAIN = 7                      # include/zkwg.h ZKWG_MAIN_CLEAN_EMAIL_ADDRESS
SHAPES = (8, 24, 32, 72)      # maxLength of every fixture file: one chunk that straddles both record slots; three chunks, the middle
#                               one straddles; the reference's shape; more bytes than lanes, straddling again
BATCH = 24                    # the shape that carries the seeded batch of 130
FR, HS = 1 << 42, 1 << 43
FULL_HASH = 8                 # the shape whose hash internals are stored in full


def fixture_name(L):
    return f"clean_{L}.npz"


def circuit_kwargs(L):
    return dict(main_kind=MAIN, max_header=L, max_body=L, n=0, k=0)


def pad(s, L):
    b = s.encode("latin-1") if isinstance(s, str) else bytes(s)
    assert len(b) <= L
    return list(b) + [0] * (L - len(b))


def should_remove(enc):
    """shouldRemove[] of the template over the integers, formula by formula (utils/email.circom:55-98): -1, 0 or 1"""
    n = len(enc)
    is_plus, is_at = [int(b == 43) for b in enc], [int(b == 64) for b in enc]
    paa = [(1 - p) * (1 - a) for p, a in zip(is_plus, is_at)]
    local, after_plus, after_at = [paa[0]], [1 - is_plus[0]], [1 - is_at[0]]
    for i in range(1, n):
        local.append(local[-1] * paa[i])
        after_plus.append(after_plus[-1] * (1 - is_plus[i]))
        after_at.append(after_at[-1] * (1 - is_at[i]))
    has_alias = 1 - after_plus[-1]
    return [local[i] * int(enc[i] == 46) + has_alias * (after_at[i] - after_plus[i]) for i in range(n)]


def field_slot(name):
    """slots whose value is a field element with no small code"""
    return any(t in name for t in (".rDec[", ".sumEnc[", ".sumDec[", ".muxEnc[", ".rHasher.", ".anon_IsEqual_final.isz.inv"))


def hash_component(name):
    """the Poseidon component of rHasher a slot belongs to, or None"""
    return name.split(".pEx.")[0] if ".rHasher." in name else None


_fx = {}


def load_fixture(L):
    """-> dict(cases = [(name, inputs)], codes = int64 [n][W], fr = per case the bytes of its FR slots in slot order, comp_sha = per case
    the digests of its HS components in slot order, W, o0_index, sym_sha256)"""
    if L not in _fx:
        z = np.load(os.path.join(GOLDEN, fixture_name(L)))
        cases = json.loads(bytes(z["cases"]).decode())
        W = int(z["W"][0])
        codes = np.frombuffer(zlib.decompress(bytes(z["codes"])), dtype="<i8").reshape(len(cases), W)
        fr, sha = bytes(z["fr"]), bytes(z["comp_sha"])
        nfr, nhs = len(fr) // (32 * len(cases)), len(sha) // (32 * len(cases))
        _fx[L] = dict(cases=[(c["name"], {"encoded": c["encoded"], "decoded": c["decoded"]}) for c in cases], codes=codes, W=W,
                      fr=[fr[32 * nfr * i:32 * nfr * (i + 1)] for i in range(len(cases))],
                      comp_sha=[sha[32 * nhs * i:32 * nhs * (i + 1)] for i in range(len(cases))],
                      o0_index=np.cumsum(np.frombuffer(zlib.decompress(bytes(z["o0_index"])), dtype="<u4"), dtype=np.uint64),
                      sym_sha256=bytes(z["sym_sha256"]).decode())
    return _fx[L]


_small = {}


def mismatch(fx, i, got, names):
    """None if the witness bytes `got` equal case i of the fixture in every slot, else a description of the first difference; a hash
    component stored as a digest is located to the component"""
    row = fx["codes"][i].tolist()
    if len(got) != 32 * len(row):
        return f"witness has {len(got)} bytes, the layout {32 * len(row)}"
    k = 0
    comp, h, comps = None, None, []
    for s, c in enumerate(row):
        v = got[32 * s:32 * s + 32]
        if c == HS:
            nm = hash_component(names[s])
            if nm != comp:
                comp, h = nm, hashlib.sha256()
                comps.append((nm, h))
            h.update(v)
            continue
        if c == FR:
            exp = fx["fr"][i][32 * k:32 * k + 32]
            k += 1
        else:
            exp = _small.get(c)
            if exp is None:
                exp = _small[c] = decode(c).to_bytes(32, "little")
        if v != exp:
            return f"{fx['cases'][i][0]}: slot {s} ({names[s]}): {int.from_bytes(v, 'little')} != {int.from_bytes(exp, 'little')}"
    for j, (nm, h) in enumerate(comps):
        if h.digest() != fx["comp_sha"][i][32 * j:32 * j + 32]:
            return f"{fx['cases'][i][0]}: the signals of {nm} differ"
    return None


def load():
    lib = nativelib.build("ceatest")
    lib.ct_create.restype = C.c_void_p
    lib.ct_create.argtypes = [C.c_void_p]
    lib.ct_destroy.argtypes = [C.c_void_p]
    lib.ct_sizes.argtypes = [C.c_void_p, C.c_void_p]
    lib.ct_run.restype = C.c_int
    lib.ct_run.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p]
    return lib


def host_images(circuit, records):
    """zkwg_cea_core.h on the host over packed records -> (scratch buffer in the layout zkwg_expand_host reads, statuses)"""
    lib = load()
    cfg = circuit.cfg
    h = lib.ct_create(C.byref(Cfg(cfg.main_kind, cfg.max_header, cfg.max_body, cfg.n, cfg.k, 0, 0, 0, 0, 0)))
    assert h
    try:
        sizes = (C.c_uint32 * 4)()
        lib.ct_sizes(h, sizes)
        n = len(records) // circuit.in_stride
        lay = circuit.image_layout(n)
        assert (sizes[0], sizes[1], sizes[2], sizes[3]) == (lay["bits_words"], lay["small_words"], lay["fr_elems"], circuit.in_stride)
        scr = (C.c_uint8 * lay["total_bytes"])()
        base = C.addressof(scr)
        status = []
        for e in range(n):
            rec = records[e * circuit.in_stride:(e + 1) * circuit.in_stride]
            status.append(lib.ct_run(h, rec, C.c_void_p(base + lay["off_small"] + 4 * sizes[1] * e),
                                     C.c_void_p(base + lay["off_fr"] + 32 * sizes[2] * e)))
        return scr, status
    finally:
        lib.ct_destroy(h)


def host_witnesses(circuit, inputs):
    """[CircuitInput] -> (witness bytes of every input through the host core and zkwg_expand_host, statuses)"""
    recs = b"".join(circuit.pack(i) for i in inputs)
    scr, status = host_images(circuit, recs)
    return circuit.expand_host(recs, len(inputs), scr, 0, len(inputs)), status
