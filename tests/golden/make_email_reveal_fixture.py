"""Writes tests/golden/email_reveal/{A,B,C}.npz: one synthetic email per shape of the application main EmailReveal
(zk-email-verify_amd/circuits/email-reveal.circom), computed by the circom interpreter (oracle/circom) executing the project's
circom file over the reference's unmodified templates.  CPU only; needs the reference tree:

    python tests/golden/make_email_reveal_fixture.py [--check]

The content follows tests/golden/make_circom_fixture.py (self-contained: the tests need neither the reference nor the interpreter):
  inputs      JSON of the CircuitInput
  o0_index    for every kept-v1 slot (product order, zkwg.Circuit.symbols()) the O0 signal index the interpreter assigns to that
              signal (0 = the constant 1) -- stored as zlib of the uint32 differences to the slot before (tests/emailreveal.py
              undoes it): the plain array is two thirds of circom_ev_576_192.npz and would push these files past 1 MiB
  witness     zlib(W x 32-byte LE values) of the interpreter's witness restricted to the kept signals, in INTERPRETER (O0) order
  n_o0        number of O0 signals (incl. the constant)
  dropped     text: one line `count pattern` per dropped-signal name pattern (indices collapsed)
  sym_sha256  SHA-256 of the kept-v1 slot names joined by newlines
"""
import collections
import json
import os
import re
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "zk-email-verify_amd", "py")):
    if p not in sys.path:
        sys.path.insert(0, p)

import emailreveal as er  # noqa: E402

# the three anonymous LessThan call sites of RevealSubstring (helpers/reveal-substring.circom:23, :27, :32)
ANON = {("RevealSubstring", "LessThan", 0): "anon_LessThan_start", ("RevealSubstring", "LessThan", 1): "anon_LessThan_length",
        ("RevealSubstring", "LessThan", 2): "anon_LessThan_sum"}


def program(shape):
    """the project's circom file with main = EmailReveal(shape), `@zk-email/circuits` mapped to the reference tree"""
    from oracle.circom import ev
    from oracle.circom.runtime import Program
    tmp = tempfile.mkdtemp(prefix="zkwg_pkg_")
    os.makedirs(os.path.join(tmp, "@zk-email"))
    os.symlink(ev.REF_CIRCUITS, os.path.join(tmp, "@zk-email", "circuits"))
    # EmailNullifier's Poseidon(1) needs the t = 2 tables, which the generated stand-in for circomlib's constants leaves out:
    # the same generator writes a copy with them, found first on the include path
    from oracle.circom import gen_poseidon_constants
    with open(os.path.join(tmp, "poseidon_constants.circom"), "w") as fh:
        fh.write(gen_poseidon_constants.render([2, 3, 6, 10, 17]))
    p = Program(None, [tmp] + ev.include_paths())
    p.load(er.CIRCOM)
    N, M, ignore, body, S, uniq, nul = shape
    p.main = ([], "EmailReveal", [("num", v) for v in (N, M, 121, 17, ignore, body, S, uniq, nul)])
    return p


def build(name):
    import zkwg
    from oracle.circom import compare
    compare.KEPT_V1_ANON.update(ANON)
    shape = er.SHAPES[name]
    inp = er.synthetic_inputs(name)
    prog = program(shape)
    root = prog.run({k: [int(x) for x in v] if isinstance(v, list) else int(v) for k, v in inp.items()})
    table = {}
    i = 1
    for nm, v, _, _ in compare.flat_walk_kept(root, prog.templates_src):
        assert nm not in table, nm
        table[nm] = (i, v)
        i += 1
    n_o0 = i
    c = zkwg.Circuit(device=-1, **er.circuit_kwargs(name))
    sym = c.symbols()
    assert sym[0] == (0, "one")
    o0 = np.zeros(len(sym), dtype=np.uint32)
    vals = [1] + [None] * (len(sym) - 1)
    for slot, nm in sym[1:]:
        o0[slot], vals[slot] = table[nm]
    assert len(set(o0.tolist())) == len(sym), "two kept slots map to one O0 signal"
    order = np.argsort(o0, kind="stable")
    wit = b"".join(int(vals[s]).to_bytes(32, "little") for s in order)
    kept = {nm for _, nm in sym}
    dropped = collections.Counter(re.sub(r"\[\d+\]", "[]", nm) for nm in table if nm not in kept)
    text = "".join(f"{n} {p}\n" for p, n in sorted(dropped.items()))
    return dict(inputs=np.frombuffer(json.dumps(inp, separators=(",", ":")).encode(), dtype=np.uint8),
                o0_index=np.frombuffer(zlib.compress(np.diff(o0.astype(np.int64), prepend=0).astype("<i4").tobytes(), 9), dtype=np.uint8),
                witness=np.frombuffer(zlib.compress(wit, 9), dtype=np.uint8), n_o0=np.array([n_o0], dtype=np.uint64),
                dropped=np.frombuffer(text.encode(), dtype=np.uint8),
                sym_sha256=np.frombuffer(er.sym_hash(sym).encode(), dtype=np.uint8))


def main(argv=None):
    check = "--check" in (sys.argv[1:] if argv is None else argv)
    os.makedirs(er.GOLDEN, exist_ok=True)
    bad = 0
    for name in er.SHAPES:
        arrays = build(name)
        path = os.path.join(er.GOLDEN, name + ".npz")
        if check:
            same = os.path.exists(path)
            if same:
                z = np.load(path)
                same = sorted(z.files) == sorted(arrays) and all(z[k].dtype == v.dtype and z[k].tobytes() == v.tobytes() for k, v in arrays.items())
            bad += not same
            print(f"{name}.npz: {'current' if same else 'DIFFERS'}")
        else:
            np.savez(path, **arrays)
            print(f"{name}.npz: {os.path.getsize(path)} bytes, {int(arrays['n_o0'][0])} O0 signals")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
