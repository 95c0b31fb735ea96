"""python -m zkwg.ptau prepare in.ptau out.ptau [--power P] [--device D]
python -m zkwg.ptau info file.ptau
-- snarkjs `.ptau` (powers of tau) reader / writer and `snarkjs powersoftau prepare phase2` on the device: the ceremony file `groth16 setup` takes its points from (reference workflow:
docs/zk-email-docs/UsageGuide/README.md:145-180, the prepared `powersOfTau28_hez_final_NN.ptau` files).

The container is not in the reference: the layout below is restated from snarkjs' published code (src/powersoftau_utils.js,
src/powersoftau_prepare_phase2.js) [EXT] and is UNPINNED until a real file is read -- as the `.zkey` container is (zkey.py).

    "ptau" | u32 version = 1 | u32 nSections | sections: u32 id, u64 size, payload
    1        u32 n8 (32), q | u32 power | u32 ceremonyPower
    2 .. 6   tau^k G1 (2^(power + 1) - 1 points) | tau^k G2 | alpha tau^k G1 | beta tau^k G1 (2^power each) | beta G2
    7        contributions
    12 - 15  the Lagrange forms of 2 - 5 ("prepared for phase 2"): levels q = 0 .. power back to back, level q starts at point
             2^q - 1; section 12 holds one level more, q = power + 1
Points: uncompressed affine, little-endian Montgomery words, x | y (G2: x.c0 | x.c1 | y.c0 | y.c1) -- the zkey's form, so slices of the
file are uploaded as they are.  alpha1 / beta1 of a key are the first points of sections 4 / 5, beta2 is section 6.

The C side (zkwg_ptau_parse, csrc/zkwg_setup_core.h) is what the set-up uses; this module is its Python twin for tools and tests.  The
writer makes a file from point sections the caller supplies (a test's toy ceremony; it computes nothing); `prepare` computes sections
12 - 15 of an unprepared file on the device (zkwg_ptau_prepare, csrc/zkwg_ptau_core.h: per level the inverse Fourier transform over the
points of the prefix; the extra level of section 12 over the 2 n - 1 powers and one point at infinity), `truncate` cuts an unprepared
file to a smaller power on the host."""
import argparse
import ctypes as C
import mmap
import struct
import sys

from .zkey import Q

# (section id, bytes per point, points as a function of n = 2^power)
SECTIONS = ((2, 64, lambda n: 2 * n - 1), (3, 128, lambda n: n), (4, 64, lambda n: n), (5, 64, lambda n: n), (6, 128, lambda n: 1),
            (12, 64, lambda n: 4 * n - 1), (13, 128, lambda n: 2 * n - 1), (14, 64, lambda n: 2 * n - 1), (15, 64, lambda n: 2 * n - 1))
LAGRANGE = {12: "tau_g1", 13: "tau_g2", 14: "alpha_tau_g1", 15: "beta_tau_g1"}


class PtauError(ValueError):
    pass


def read_ptau(data, prepared=True):
    """data: bytes, memoryview or mmap -> dict: power, ceremony_power, sections = {id: (offset, size)}.  Sizes are checked before any
    point is touched; a file without sections 12 - 15 is refused ("Powers of tau is not prepared") unless prepared=False, which reads
    an UNPREPARED file and refuses one that has any of them."""
    if len(data) < 12 or bytes(data[:4]) != b"ptau":
        raise ValueError("not a .ptau file")
    version, nsec = struct.unpack_from("<II", data, 4)
    if version != 1:
        raise ValueError(f".ptau version {version} is not supported")
    pos, sec = 12, {}
    for _ in range(nsec):
        if pos + 12 > len(data):
            raise ValueError(".ptau: truncated section table")
        sid, size = struct.unpack_from("<IQ", data, pos)
        if pos + 12 + size > len(data):
            raise ValueError(f".ptau: section {sid} runs past the end of the file")
        sec[sid] = (pos + 12, size)
        pos += 12 + size
    if 1 not in sec or sec[1][1] != 44:
        raise ValueError(".ptau: header section missing or of the wrong size")
    o = sec[1][0]
    n8 = struct.unpack_from("<I", data, o)[0]
    if n8 != 32 or int.from_bytes(bytes(data[o + 4:o + 36]), "little") != Q:
        raise ValueError(".ptau: the prime is not the BN254 base field")
    power, ceremony = struct.unpack_from("<II", data, o + 36)
    if not 1 <= power <= 28:
        raise ValueError(".ptau: power out of range")
    n = 1 << power
    if not prepared and any(sid in sec for sid in LAGRANGE):
        raise ValueError(".ptau: the file is already prepared (it has a section 12 - 15)")
    wanted = [t for t in SECTIONS if prepared or t[0] < 12]
    for sid, point, count in wanted:
        if sid not in sec:
            raise ValueError("Powers of tau is not prepared" if sid >= 12 else f".ptau: section {sid} is missing")
    for sid, point, count in wanted:
        if sec[sid][1] != point * count(n):
            raise ValueError(f".ptau: section {sid} holds {sec[sid][1]} bytes, expected {point * count(n)}")
    return {"power": power, "ceremony_power": ceremony, "sections": sec}


def level(data, info, sid, q):
    """the 2^q points of level q of Lagrange section sid (12 - 15), as a memoryview into data"""
    point = 128 if sid == 13 else 64
    if q > info["power"] + (1 if sid == 12 else 0):
        raise ValueError(f".ptau: the file (power {info['power']}) has no level {q}")
    o = info["sections"][sid][0] + ((1 << q) - 1) * point
    return memoryview(data)[o:o + (point << q)]


def slices(data, power):
    """what the set-up of a 2^power domain reads: dict tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1 (level power), tau_g1_next (level
    power + 1), alpha1, beta1, beta2 (bytes)"""
    info = read_ptau(data)
    if power > info["power"]:
        raise ValueError(f".ptau: the power of the file ({info['power']}) is too small for the circuit ({power})")
    out = {name: level(data, info, sid, power) for sid, name in LAGRANGE.items()}
    out["tau_g1_next"] = level(data, info, 12, power + 1)
    s = info["sections"]
    out["alpha1"] = bytes(data[s[4][0]:s[4][0] + 64])
    out["beta1"] = bytes(data[s[5][0]:s[5][0] + 64])
    out["beta2"] = bytes(data[s[6][0]:s[6][0] + 128])
    return out


def write_ptau(power, sections, ceremony_power=None, contributions=b""):
    """sections: {id: bytes} for ids 2 - 6 and, for a prepared file, 12 - 15 (whole sections, every level); sizes are asserted"""
    n = 1 << power
    for sid, point, count in SECTIONS:
        if sid in sections:
            assert len(sections[sid]) == point * count(n), (sid, len(sections[sid]), point * count(n))
    hdr = struct.pack("<I", 32) + Q.to_bytes(32, "little") + struct.pack("<II", power, power if ceremony_power is None else ceremony_power)
    secs = [(1, hdr)] + [(sid, bytes(sections[sid])) for sid in (2, 3, 4, 5, 6) if sid in sections] + [(7, contributions)]
    secs += [(sid, bytes(sections[sid])) for sid in (12, 13, 14, 15) if sid in sections]
    out = [b"ptau", struct.pack("<II", 1, len(secs))]
    for sid, payload in secs:
        out.append(struct.pack("<IQ", sid, len(payload)))
        out.append(payload)
    return b"".join(out)


def truncate(data, power):
    """an UNPREPARED file cut to a smaller power (host only): the header's power set, ceremonyPower kept, sections 2 - 6 cut to
    2 n - 1 | n | n | n | 1 points, section 7 verbatim"""
    info = read_ptau(data, prepared=False)
    if not 1 <= power <= info["power"]:
        raise PtauError(f".ptau: cannot cut a file of power {info['power']} to power {power}")
    n, sec = 1 << power, info["sections"]
    cut = {sid: bytes(data[sec[sid][0]:sec[sid][0] + point * count(n)]) for sid, point, count in SECTIONS if sid < 12}
    contributions = bytes(data[sec[7][0]:sec[7][0] + sec[7][1]]) if 7 in sec else b""
    return write_ptau(power, cut, ceremony_power=info["ceremony_power"], contributions=contributions)


def prepare(data, power=None, device=0):
    """an unprepared file (bytes, or an mmap: only the prefixes are read) -> the prepared file of `power` (None: the file's own) as
    bytes, sections 12 - 15 computed on the device (zkwg_ptau_prepare)"""
    import numpy as np
    from . import _lib
    lib = _lib.load()
    a = np.frombuffer(data, dtype=np.uint8)            # (no copy; works for an mmap)
    size, out_len = C.c_uint64(), C.c_uint64()
    try:
        rc = lib.zkwg_ptau_prepare_size(a.ctypes.data, a.size, power or 0, C.byref(size))
        if rc == 0:
            out = np.empty(size.value, dtype=np.uint8)
            rc = lib.zkwg_ptau_prepare(device, a.ctypes.data, a.size, power or 0, out.ctypes.data, size.value, C.byref(out_len))
    finally:
        del a                                          # (an mmap cannot be closed while a view of it lives)
    if rc != 0:
        msg = lib.zkwg_last_error().decode() if rc == -1 else ""
        raise PtauError(f"{lib.zkwg_strerror(rc).decode()}{': ' + msg if msg else ''}")
    return out[:out_len.value].tobytes()


def last_stats():
    """seconds and group operations of this thread's last prepare (zkwg_ptau_prepare_stats), per section 12 - 15"""
    from . import _lib
    sec, ops = (C.c_double * 140)(), (C.c_uint64 * 8)()
    _lib.load().zkwg_ptau_prepare_stats(sec, ops)
    return {sid: {"upload_check": sec[3 * i], "transforms": sec[3 * i + 1], "affine_download": sec[3 * i + 2], "add": ops[2 * i], "dbl": ops[2 * i + 1],
                  "levels": list(sec[12 + 32 * i:12 + 32 * i + 32])} for i, sid in enumerate((12, 13, 14, 15))}


def group_ntt(group, points, inverse, device=0):
    """the Fourier transform over `points` (bytes in the zkey's form, a power of two of them) -> bytes (zkwg_group_ntt_device)"""
    import torch
    from . import _lib
    lib = _lib.load()
    pt = 64 if group == 1 else 128
    n = len(points) // pt
    if n * pt != len(points) or n == 0 or n & (n - 1):
        raise PtauError("the points must be whole and a power of two of them")
    d = torch.frombuffer(bytearray(points), dtype=torch.uint8).to(torch.device("cuda", device))
    rc = lib.zkwg_group_ntt_device(device, group, d.data_ptr(), n.bit_length() - 1, 1 if inverse else 0, 0)
    if rc != 0:
        msg = lib.zkwg_last_error().decode() if rc == -1 else ""
        raise PtauError(f"{lib.zkwg_strerror(rc).decode()}{': ' + msg if msg else ''}")
    return bytes(d.cpu().numpy())


def main(argv=None):
    ap = argparse.ArgumentParser(description="powers of tau: prepare a file for phase 2 on the device, or describe one")
    sub = ap.add_subparsers(dest="cmd", required=True)
    pp = sub.add_parser("prepare")
    pp.add_argument("ptau_in")
    pp.add_argument("ptau_out")
    pp.add_argument("--power", type=int, default=None)
    pp.add_argument("--device", type=int, default=0)
    pi = sub.add_parser("info")
    pi.add_argument("ptau")
    a = ap.parse_args(argv)
    path = a.ptau_in if a.cmd == "prepare" else a.ptau
    out, why = None, ""
    with open(path, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as mm:
        try:
            if a.cmd == "prepare":
                out = prepare(mm, a.power, a.device)
            else:
                try:
                    info, state = read_ptau(mm), "prepared"
                except ValueError as e:
                    if "not prepared" not in str(e):
                        raise
                    info, state = read_ptau(mm, prepared=False), "not prepared"
                out = f"power {info['power']}, ceremony power {info['ceremony_power']}, {state}; sections " + \
                      ", ".join(f"{sid}: {size} bytes" for sid, (_, size) in sorted(info["sections"].items()))
        except ValueError as e:
            why = str(e)
    if out is None:
        print(f"no file: {why}", file=sys.stderr)
        return 1
    if a.cmd == "info":
        print(out)
    else:
        open(a.ptau_out, "wb").write(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
