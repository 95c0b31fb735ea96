"""snarkjs `.wtns` reader / writer: the witness file `groth16.prove(zkey, wtns)` takes (reference call site:
packages/helpers/src/chunked-zkey.ts:80-84; written by `snarkjs wtns calculate` / generate_witness.js,
docs/zk-email-docs/UsageGuide/README.md:132-140).

    "wtns" | u32 version = 2 | u32 nSections = 2 | sections: u32 id, u64 size, payload
    1  u32 n8 (32) | the prime r | u32 nWitness            2  nWitness values of n8 bytes, little-endian, standard form
The C reader is zkwg_wtns_parse (csrc/zkwg_zkey_core.h), the C writer zkwg_write_wtns; sections may come in either order.
"""
import struct

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def read_wtns(data, n_vars=None):
    """-> (nWitness, the 32 * nWitness bytes of the values); ValueError for anything that is not a BN254 .wtns (or, with n_vars given,
    not a witness of that many values)"""
    data = bytes(data)
    if len(data) < 12 or data[:4] != b"wtns":
        raise ValueError("not a .wtns file")
    version, nsec = struct.unpack_from("<II", data, 4)
    if version != 2:
        raise ValueError(f".wtns version {version} is not supported")
    pos, sec = 12, {}
    for _ in range(nsec):
        if pos + 12 > len(data):
            raise ValueError(".wtns: truncated section table")
        sid, size = struct.unpack_from("<IQ", data, pos)
        if pos + 12 + size > len(data):
            raise ValueError(f".wtns: section {sid} runs past the end of the file")
        sec[sid] = (pos + 12, size)
        pos += 12 + size
    if 1 not in sec or 2 not in sec or sec[1][1] != 40:
        raise ValueError(".wtns: header or value section missing")
    o = sec[1][0]
    n8 = struct.unpack_from("<I", data, o)[0]
    if n8 != 32 or int.from_bytes(data[o + 4:o + 36], "little") != R:
        raise ValueError(".wtns: not a BN254 witness")
    n = struct.unpack_from("<I", data, o + 36)[0]
    if sec[2][1] != 32 * n:
        raise ValueError(f".wtns: section 2 holds {sec[2][1]} bytes, expected {32 * n}")
    if n_vars is not None and n != n_vars:
        raise ValueError(f".wtns: {n} values, the key has {n_vars} wires")
    return n, data[sec[2][0]:sec[2][0] + 32 * n]


def write_wtns(values):
    """values: the 32 * nWitness bytes -> the file"""
    values = bytes(values)
    assert len(values) % 32 == 0
    s1 = struct.pack("<I", 32) + R.to_bytes(32, "little") + struct.pack("<I", len(values) // 32)
    return b"wtns" + struct.pack("<II", 2, 2) + struct.pack("<IQ", 1, len(s1)) + s1 + struct.pack("<IQ", 2, len(values)) + values
