"""The `.ptau` container: zkwg.ptau (Python) and zk_ptau_parse (csrc/zkwg_setup_core.h, through the host build tests/native/setuptest.cpp)
read what zkwg.ptau.write_ptau writes, hand out the same slices, and refuse what the set-up must refuse -- sizes are checked before any
point is read, so no truncated or mis-sized file can make a reader look past its buffer.  The container itself is restated from snarkjs
[EXT] and unpinned: what is checked here is the round trip and the refusals."""
import struct

import setuptest
from zkwg import ptau

Q = setuptest.Q


def _sections(power, prepared=True):
    """sections whose bytes name their place: point k of section s is filled with the byte (7 s + k) & 255"""
    n = 1 << power
    out = {}
    for sid, point, count in ptau.SECTIONS:
        if sid >= 12 and not prepared:
            continue
        out[sid] = b"".join(bytes([(7 * sid + k) & 255]) * point for k in range(count(n)))
    return out


def _both(data, power):
    """(Python's answer, C's answer): each None when refused, else the offsets of tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, tau_g1_next"""
    try:
        s = ptau.slices(data, power)
        info = ptau.read_ptau(data)
        sec = info["sections"]
        first = (1 << power) - 1
        py = [sec[12][0] + 64 * first, sec[13][0] + 128 * first, sec[14][0] + 64 * first, sec[15][0] + 64 * first, sec[12][0] + 64 * ((2 << power) - 1)]
        assert bytes(s["tau_g1"]) == bytes(data[py[0]:py[0] + (64 << power)]) and bytes(s["tau_g1_next"]) == bytes(data[py[4]:py[4] + (128 << power)])
    except ValueError as e:
        py = None
        py_msg = str(e)
    rc, msg, off, pts = setuptest.host_ptau_parse(data, power)
    c = off if rc == 0 else None
    assert rc in (0, -1)
    return py, c, (msg if rc else ""), (py_msg if py is None else "")


def test_round_trip_and_slices():
    power = 3
    secs = _sections(power)
    data = ptau.write_ptau(power, secs, ceremony_power=28)
    info = ptau.read_ptau(data)
    assert info["power"] == power and info["ceremony_power"] == 28
    for sid, point, count in ptau.SECTIONS:
        o, size = info["sections"][sid]
        assert data[o:o + size] == secs[sid]
    for p in (1, 2, 3):
        py, c, msg, _ = _both(data, p)
        assert py == c and py is not None, msg
        s = ptau.slices(data, p)
        first = (1 << p) - 1
        # level p starts at point 2^p - 1 of its section; level p + 1 of section 12 at 2^(p + 1) - 1
        assert s["tau_g1"][0] == (7 * 12 + first) & 255 and s["tau_g1"][-1] == (7 * 12 + 2 * first) & 255 and len(s["tau_g1"]) == 64 << p
        assert s["tau_g2"][0] == (7 * 13 + first) & 255 and len(s["tau_g2"]) == 128 << p
        assert s["alpha_tau_g1"][0] == (7 * 14 + first) & 255 and s["beta_tau_g1"][0] == (7 * 15 + first) & 255
        assert s["tau_g1_next"][0] == (7 * 12 + 2 * first + 1) & 255 and len(s["tau_g1_next"]) == 128 << p
        assert s["alpha1"] == secs[4][:64] and s["beta1"] == secs[5][:64] and s["beta2"] == secs[6]
        rc, msg, off, pts = setuptest.host_ptau_parse(data, p)
        assert pts == secs[4][:64] + secs[5][:64] + secs[6]
    # a memoryview / bytearray reads the same
    assert ptau.read_ptau(memoryview(bytearray(data)))["sections"] == info["sections"]


def test_refusals():
    power = 2
    secs = _sections(power)
    good = ptau.write_ptau(power, secs)
    assert _both(good, 2)[0] is not None
    # power < p
    py, c, msg, py_msg = _both(good, 3)
    assert py is None and c is None and "too small" in msg and "too small" in py_msg
    # sections 12 - 15 absent
    py, c, msg, py_msg = _both(ptau.write_ptau(power, _sections(power, prepared=False)), 2)
    assert py is None and c is None and "not prepared" in msg and "not prepared" in py_msg
    # one of them absent
    py, c, msg, py_msg = _both(ptau.write_ptau(power, {k: v for k, v in secs.items() if k != 14}), 2)
    assert py is None and c is None and "not prepared" in msg and "not prepared" in py_msg
    # wrong prime
    o = good.index(Q.to_bytes(32, "little"))
    bad = bytearray(good)
    bad[o] ^= 2
    py, c, msg, py_msg = _both(bytes(bad), 2)
    assert py is None and c is None and "prime" in msg and "prime" in py_msg
    # a truncated section table: the last section's 12-byte head cut short, and the count naming a section that is not there
    last = len(good) - len(secs[15]) - 12
    for cut in (good[:last + 5], good[:last]):
        py, c, msg, py_msg = _both(cut, 2)
        assert py is None and c is None and "truncated" in msg and "truncated" in py_msg
    # section 12 without level power + 1 (the size of an unextended Lagrange section)
    n = 1 << power
    short12 = dict(secs)
    short12[12] = secs[12][:64 * (2 * n - 1)]
    blob = _write_unchecked(power, short12)
    py, c, msg, py_msg = _both(blob, 2)
    assert py is None and c is None and "size" in msg and "expected" in py_msg
    # a point section of the wrong size, a bad magic, a bad version
    wrong = dict(secs)
    wrong[3] = secs[3] + bytes(128)
    assert _both(_write_unchecked(power, wrong), 2)[:2] == (None, None)
    assert _both(b"ptaX" + good[4:], 2)[:2] == (None, None)
    assert _both(good[:4] + struct.pack("<I", 2) + good[8:], 2)[:2] == (None, None)


def _write_unchecked(power, sections):
    """write_ptau without its size assertions"""
    hdr = struct.pack("<I", 32) + Q.to_bytes(32, "little") + struct.pack("<II", power, power)
    secs = [(1, hdr)] + [(sid, sections[sid]) for sid in (2, 3, 4, 5, 6) if sid in sections] + [(7, b"")] + [(sid, sections[sid]) for sid in (12, 13, 14, 15) if sid in sections]
    return b"ptau" + struct.pack("<II", 1, len(secs)) + b"".join(struct.pack("<IQ", sid, len(p)) + p for sid, p in secs)


def test_write_unchecked_matches_the_writer():
    assert _write_unchecked(2, _sections(2)) == ptau.write_ptau(2, _sections(2))


def test_every_truncation_is_refused_or_parses():
    """every prefix of a small file: both readers refuse it (no exception but ValueError, no crash) -- only the whole file parses"""
    power = 1
    good = ptau.write_ptau(power, _sections(power))
    assert _both(good, 1)[0] is not None
    for cut in range(len(good)):
        py, c, msg, py_msg = _both(good[:cut], 1)
        assert py is None and c is None, cut
    # bytes after the last section change nothing
    py, c, _, _ = _both(good + b"tail", 1)
    assert py == c and py is not None


def test_r1cs_mutations_are_refused_or_parse():
    """every truncation point of a small .r1cs through the set-up's size entry: refused (-1) or parsed (0), never a crash"""
    import ctypes as C
    from zkwg import r1cs as zr
    lib = setuptest.load()
    n_wires, cons, w = setuptest.system(seed=3, n_in=4, n_public=1, n_cons=3)
    good = zr.write_r1cs(n_wires, cons, n_pub_out=1, n_prv_in=2)
    power, size, err = C.c_uint32(), C.c_uint64(), C.create_string_buffer(256)
    assert lib.st_zkey_new_size(good, len(good), C.byref(power), C.byref(size), err, 256) == 0 and power.value == 3
    seen = set()
    for cut in range(len(good)):
        seen.add(lib.st_zkey_new_size(good[:cut], cut, C.byref(power), C.byref(size), err, 256))
    assert seen <= {0, -1} and -1 in seen
