"""The SHA-256 round records of the compact image (csrc/zkwg_sha_rounds.h): 200 words per block from which zk_expand's decoders
recompute the 30,952 kept signals of a Sha256compression.  On the host (tests/native/shacompacttest.cpp): for every
(chaining state, block) the product's writer leaves the record, and every slot decoded from it must be the bit of the 952-group
trace, restated in the helper as zk_sha_trace wrote it before the records; hin + {A[63..60], E[63..60]} must be the next
chaining state of the textbook compression.  Also as a stand-alone program under the address / undefined-behaviour sanitizers."""
import ctypes as C
import hashlib
import os
import random
import struct
import subprocess

import pytest

import nativelib
from conftest import ROOT

IV = (0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19)
ONES = (0xffffffff,) * 8


def _cases():
    """[(name, state, block)]: 200 seeded random pairs and the fixed blocks"""
    rng = random.Random(20)
    out = [(f"random {i}", tuple(rng.getrandbits(32) for _ in range(8)), bytes(rng.getrandbits(8) for _ in range(64))) for i in range(200)]
    out.append(("all-zero block", IV, bytes(64)))
    out.append(("all-0xFF block", IV, b"\xff" * 64))
    # round 0 of this one: h = bs1 = ch = W[0] = 2^32 - 1, so t1 = 4 (2^32 - 1) + K[0] > 2^34
    out.append(("t1 above 2^34", ONES, b"\xff" * 64))
    out.append(("IV, padded empty message", IV, b"\x80" + bytes(63)))
    return out


@pytest.fixture(scope="module")
def lib():
    lib = nativelib.build("shacompacttest")
    lib.sc_check.restype = C.c_longlong
    lib.sc_check.argtypes = [C.c_void_p] * 5
    return lib


def test_every_slot_decoded_from_the_record_is_the_bit_of_the_trace(lib):
    seen_big = False
    for name, st, blk in _cases():
        hin = (C.c_uint32 * 8)(*st)
        a, b = (C.c_uint32 * 8)(), (C.c_uint32 * 8)()
        t1 = C.c_uint64(0)
        r = lib.sc_check(hin, blk, a, b, C.byref(t1))
        assert r == -1, (name, r)
        assert list(a) == list(b), name                     # A[63]..E[60] + hin = the next chaining state
        if name == "t1 above 2^34":
            assert t1.value > 1 << 34
            seen_big = True
        if name == "IV, padded empty message":
            assert struct.pack(">8I", *a) == hashlib.sha256(b"").digest()
    assert seen_big


def test_writer_and_decoders_under_the_sanitizers_as_a_stand_alone_program(tmp_path):
    exe = tmp_path / "shacompacttest_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSHACOMPACT_MAIN",
                           "-I", os.path.join(ROOT, "zk-email-verify_amd", "csrc"), os.path.join(ROOT, "tests", "native", "shacompacttest.cpp"),
                           "-o", str(exe)])
    cases = _cases()
    path = tmp_path / "cases.bin"
    path.write_bytes(b"".join(struct.pack("<8I", *st) + blk for _, st, blk in cases))
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.split() == ["-1"] * len(cases)
