"""Test-only helpers of the substring search of csrc/zkwg_locate_core.h: its host build (tests/native/locatetest.cpp), the wavefront
function on the simulated wavefront of tests/native/wavesim.h beside the serial statement."""
import ctypes as C

import nativelib

FIRST, COUNT = 0, 1
NONE = 0xffffffff


def load():
    lib = nativelib.build("locatetest", extra_includes=(nativelib.NATIVE,))
    u32 = C.c_uint32
    for f in (lib.lt_tile, lib.lt_chunk):
        f.restype = u32
    lib.lt_serial.restype = u32
    lib.lt_serial.argtypes = [C.c_char_p, u32, C.c_char_p, u32, u32]
    lib.lt_wave.restype = u32
    lib.lt_wave.argtypes = [C.c_char_p, u32, C.c_char_p, u32, u32, u32]
    return lib


def tile():
    return load().lt_tile()


def chunk():
    return load().lt_chunk()


def locate(src, needle, what=FIRST, wave=True, offset=0, length=None):
    """first position (None: absent) or number of occurrences of `needle` in src[0, length)"""
    n = len(src) if length is None else length
    r = load().lt_wave(src, n, needle, len(needle), what, offset) if wave else load().lt_serial(src, n, needle, len(needle), what)
    assert r != 0xfffffffe, "the lanes disagree"
    return None if what == FIRST and r == NONE else r
