"""Test-only helpers of `zkey verify` (zkwg.phase2.verify / verify_from_init): the two-array form of the host sums (what
zkwg_point_rlc_device must equal when d_b is an array of its own), zkwg.phase2 with every device call replaced by its host mirror, and the
tampers with a .zkey that the CPU and the GPU tests share."""
import struct

import phase2test
import setuptest
import verifytest

HEADER_AT = {"alpha1": (84, 64), "beta1": (148, 64), "beta2": (212, 128), "gamma2": (340, 128), "delta1": (468, 64), "delta2": (532, 128)}
POINT = {3: 64, 5: 64, 6: 64, 7: 128, 8: 64, 9: 64}


def rlc2(group, points, other, scalars, scalar_bytes=16):
    """(sum_i s_i P_i, sum_i s_i O_i) on the host, or None when a point of either array is not on its curve"""
    a, b = verifytest.rlc(group, points, scalars, scalar_bytes), verifytest.rlc(group, other, scalars, scalar_bytes)
    return None if a is None or b is None else (a, b)


class HostBackend(verifytest.HostBackend):
    """verifytest.HostBackend with the two-array form of zkwg.ptau._Device.rlc"""

    def rlc(self, group, points, first, n, scalars, wide=False, shifted=False, piece=0, other=None):
        if other is None:
            return super().rlc(group, points, first, n, scalars, wide=wide, shifted=shifted, piece=piece)
        from zkwg import ptau
        pt, sb = (64 if group == 1 else 128), (32 if wide else 16)
        out = rlc2(group, points[first * pt:(first + n) * pt], other[first * pt:(first + n) * pt], scalars[:n * sb], sb)
        if out is None:
            raise ptau.PointRefused("a point is not on its curve (or not reduced)")
        return out


def host_mirrors(mp):
    """zkwg.phase2 / zkwg.setup / zkwg.ptau with every device call replaced by its host mirror (mp: a pytest.MonkeyPatch)"""
    import torch
    from zkwg import phase2, prover, ptau, setup
    mp.setattr(phase2, "scale_points", lambda group, pts, s, device=0: phase2test.scale(group, pts, s))
    mp.setattr(prover, "fixed_base", lambda device, group, scalars: torch.frombuffer(bytearray(setuptest.host_points(group, scalars)), dtype=torch.uint8))

    def apply_delta(z, k, section10, device=0):
        rc, msg, out = phase2test.apply_delta(bytes(z), k, section10)
        if rc != 0:
            raise phase2.Phase2Error(msg)
        return out
    mp.setattr(phase2, "apply_delta", apply_delta)

    def new_zkey(r1cs, ptau_bytes, device=0):
        power, _ = setup.key_shape(r1cs)               # (zkwg_zkey_new_size: host only)
        sl = dict(ptau.slices(ptau_bytes, power), power=power)
        rc, msg, z, _ = setuptest.host_new_zkey(r1cs, sl)
        if rc != 0:
            raise setup.SetupError(msg)
        return z
    mp.setattr(setup, "new_zkey", new_zkey)
    mp.setattr(ptau, "_backend", lambda device: HostBackend())


# ---- reading and changing a .zkey -------------------------------------------------------------------------------------------------------------
def _sec(z):
    from zkwg import zkey
    return zkey.sections(z)


def point(z, sid, i):
    o = _sec(z)[sid][0] + POINT[sid] * i
    return bytes(z[o:o + POINT[sid]])


def set_point(z, sid, i, p):
    o = _sec(z)[sid][0] + POINT[sid] * i
    assert len(p) == POINT[sid] and bytes(z[o:o + len(p)]) != p
    return bytes(z[:o]) + p + bytes(z[o + len(p):])


def swap_points(z, sid, i, j):
    a, b = point(z, sid, i), point(z, sid, j)
    return set_point(set_point(z, sid, i, b), sid, j, a)


def count(z, sid):
    return _sec(z)[sid][1] // POINT[sid]


def two_distinct(z, sid):
    """the lowest two indices of the section whose points differ and are not infinity"""
    i = next(k for k in range(count(z, sid)) if any(point(z, sid, k)))
    j = next(k for k in range(i + 1, count(z, sid)) if any(point(z, sid, k)) and point(z, sid, k) != point(z, sid, i))
    return i, j


def infinity_at(z, sid):
    return [k for k in range(count(z, sid)) if not any(point(z, sid, k))]


def header_point(z, name):
    o, size = HEADER_AT[name]
    o += _sec(z)[2][0]
    return bytes(z[o:o + size])


def set_header_point(z, name, p):
    o, size = HEADER_AT[name]
    o += _sec(z)[2][0]
    assert len(p) == size and bytes(z[o:o + size]) != p
    return bytes(z[:o]) + p + bytes(z[o + size:])


def with_records(z, records):
    """the key with these records (dicts as zkwg.phase2.read_contributions gives them, re-packed) as its section 10, which keeps its length"""
    from zkwg import phase2
    o, size = _sec(z)[10]
    s10 = phase2.pack_section10(bytes(z[o:o + 64]), [phase2.pack_record(r) for r in records])
    assert len(s10) == size
    return bytes(z[:o]) + s10 + bytes(z[o + size:])


def flip_coefficient_byte(z, i):
    """the lowest byte of the value of coefficient i of section 4, one bit changed"""
    o = _sec(z)[4][0] + 4 + 44 * i + 12
    return bytes(z[:o]) + bytes([z[o] ^ 1]) + bytes(z[o + 1:])


# ---- the tampers --------------------------------------------------------------------------------------------------------------------------------
G1_GENERATOR = setuptest.mont1((1, 2))
UNRECORDED_K = 0x1234567890abcdef1234567890abcdef1234567


def tampers():
    """name -> (change(final key) -> key, the checks that fail).  The final key holds a contribution and then a beacon (records 1, 2);
    every change uses zkwg.phase2 for its group operations, so it runs on the device or on the host mirrors, whichever is in place"""
    from zkwg import phase2
    double = lambda group, p: phase2.scale_points(group, p, 2)

    def swap(sid):
        return lambda z: swap_points(z, sid, *two_distinct(z, sid))

    def doubled_8(z):
        i = two_distinct(z, 8)[1]
        return set_point(z, 8, i, double(1, point(z, 8, i)))

    def infinity_8(z):
        return set_point(z, 8, infinity_at(z, 8)[0], G1_GENERATOR)

    def last_g1_sx(z):
        recs = [dict(r) for r in phase2.read_contributions(z)[1]]
        recs[-1]["g1_sx"] = double(1, recs[-1]["g1_sx"])
        return with_records(z, recs)

    def unrecorded(z):
        o, size = _sec(z)[10]
        return phase2.apply_delta(z, UNRECORDED_K, bytes(z[o:o + size]))

    def beacon_exponent(z):
        recs = [dict(r) for r in phase2.read_contributions(z)[1]]
        assert recs[-1]["type"] == phase2.TYPE_BEACON and recs[-1]["num_iterations_exp"] == 10
        recs[-1]["num_iterations_exp"] = 11
        return with_records(z, recs)
    out = {f"swap_{sid}": (swap(sid), {f"section_{sid}"}) for sid in (8, 9, 5, 6, 7, 3)}
    out.update({
        "doubled_8": (doubled_8, {"section_8"}),
        "infinity_8": (infinity_8, {"section_8"}),
        "coefficient_byte_4": (lambda z: flip_coefficient_byte(z, 5), {"section_4"}),
        # (sections 8 and 9 are compared UNDER delta2, so a delta2 that is not delta1's breaks both ratios as well: no single check can fail alone)
        "delta2_doubled": (lambda z: set_header_point(z, "delta2", double(2, header_point(z, "delta2"))), {"delta", "section_8", "section_9"}),
        "last_g1_sx": (last_g1_sx, {"record_2"}),
        "unrecorded_contribution": (unrecorded, {"last_record"}),
        "beacon_exponent": (beacon_exponent, {"record_2"}),
    })
    return out


def broken_containers(z):
    """keys that `structure` refuses: a truncated file, a section 10 one byte short of its records, a record count that is too large"""
    o, size = _sec(z)[10]
    short = bytearray(z[:-1])
    short[o - 8:o] = struct.pack("<Q", size - 1)
    more = bytearray(z)
    more[o + 64:o + 68] = struct.pack("<I", 3)
    return [bytes(z[:-30]), bytes(short), bytes(more)]


def failed(res):
    return {name for name, ok, _ in res["checks"] if ok is False}
