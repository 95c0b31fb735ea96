"""Writes tests/golden/clean_address/*.npz: inputs and expected witnesses of the CleanEmailAddress main, computed by executing the
reference's template (packages/circuits/utils/email.circom) with the circom interpreter (oracle/circom).  CPU only; needs the
reference tree.  Per shape one file with
  cases       JSON: [{name, encoded, decoded}] (the template asserts nothing: every case has a witness)
  codes       zlib of one int64 per slot (tests/ceatest.py) of every case, in case order, slot order
  fr          the 32-byte values of the slots coded FR, in the same order
  comp_sha    the SHA-256 over the slots of every Poseidon component coded HS, in the same order
  o0_index    zlib of the O0 index of every slot as uint32 differences to the slot before
  sym_sha256  SHA-256 of the slot names joined by newlines
  W           slots per witness
The slot names come from a layout-only zkwg handle; values and O0 indices are looked up by name in the interpreter's walk.

    python tests/golden/make_clean_address_fixtures.py [--check]
"""
import hashlib
import json
import os
import random
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "zk-email-verify_amd", "py")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ceatest as ct  # noqa: E402
from oracle.circom import ev, compare  # noqa: E402
from oracle.circom.runtime import Program  # noqa: E402

# the six anonymous IsEqual call sites of CleanEmailAddress (utils/email.circom:55, :56, :60, :61, :68, :139)
ANON = {("CleanEmailAddress", "IsEqual", i): "anon_IsEqual_" + nm for i, nm in enumerate(("plus0", "at0", "plus", "at", "period", "final"))}
# clean-email-address.test.ts: (encoded, decoded, isValid)
REFERENCE = (("dots_and_alias", "shreyas.londhe+alias@gmail.com", "shreyaslondhe@gmail.com", 1),
             ("wrong_domain", "shreyas.londhe+alias@gmail.com", "shreyaslondhe@yahoo.com", 0),
             ("only_dots", "shreyas.londhe@gmail.com", "shreyaslondhe@gmail.com", 1),
             ("only_alias", "shreyaslondhe+test@gmail.com", "shreyaslondhe@gmail.com", 1),
             ("multiple_dots", "shreyas.londhe.test@gmail.com", "shreyaslondhetest@gmail.com", 1),
             ("complex_alias", "shs.loe+test.alias+123@gmail.com", "shsloe@gmail.com", 1),
             ("no_modifications", "shreyaslondhe@gmail.com", "shreyaslondhe@gmail.com", 1))


def program(L):
    if L == 32:
        return ev.program("tests/test-circuits/clean-email-address-test.circom", track_how=True)
    p = Program(None, ev.include_paths(), track_how=True)    # the same main with another parameter
    p.load(os.path.join(ev.REF_CIRCUITS, "utils", "email.circom"))
    p.main = ([], "CleanEmailAddress", [("num", L)])
    return p


def cases(L):
    """(name, encoded, decoded, expected isValid or None): the reference suite where it fits, the project's own edge cases, the seeded batch"""
    out = []
    add = lambda name, enc, dec, valid=None: out.append((name, ct.pad(enc, L), ct.pad(dec, L), valid))
    if L >= 32:
        for name, enc, dec, valid in REFERENCE:
            add("ref_" + name, enc, dec, valid)
    add("own_at_before_plus", "a@b+c.d", "a@b+c.d")            # shouldRemove = -1 on @, b: processed doubles, rEnc takes 2 r - 1
    add("own_plus_first", "+ab@c.d", "@c.d", 1)
    add("own_period_first", ".ab@c.d", "ab@c.d", 1)
    add("own_no_at", "a.b+c.d", "ab", 1)                        # the alias never ends
    add("own_plain", "a.b.c", "abc", 1)                         # neither '+' nor '@'
    add("own_two_at", "a.b@c@d", "ab@c@d", 1)
    add("own_at_last", [97] * (L - 1) + [64], [97] * (L - 1) + [64], 1)
    add("own_all_zero", [], [], 1)
    add("own_all_255", [255] * L, [255] * L, 1)
    full = ("ab.cd+ef@gh.ij" * 8)[:L]                           # full length, no padding; decoded by the template's own rule
    add("own_full_length", full, [b for b, s in zip(ct.pad(full, L), ct.should_remove(ct.pad(full, L))) if s == 0], 1)
    add("own_neighbours", [42, 44, 45, 47, 63, 65, 43, 64][:L], [42, 44, 45, 47, 63, 65])   # differences of +-1 to '+', '.', '@'
    add("own_unequal_sums", "a.b@c", "a.b@c", 0)
    add("own_shifted", "ab@c", [0, 97, 98, 64, 99], 0)
    if L == ct.BATCH:
        alphabet = [97, 98, 99, 46, 46, 43, 64, 255]
        for k in range(130):
            r = random.Random(7919 * k + 1)
            enc = ct.pad([r.choice(alphabet) for _ in range(r.randrange(1, L + 1))], L)
            sr = ct.should_remove(enc)
            # decoded by the template's own rule over the integers; where a shouldRemove is -1 no decoding is meant: encoded unchanged
            dec = list(enc) if -1 in sr else ct.pad([b for b, s in zip(enc, sr) if s == 0], L)
            if k & 1:
                dec[r.randrange(L)] ^= 1 << r.randrange(8)
            add(f"batch_{k}", enc, dec)
    return out


def build(L):
    import zkwg
    compare.KEPT_V1_ANON.update(ANON)
    c = zkwg.Circuit(device=-1, **ct.circuit_kwargs(L))
    sym = c.symbols()
    names = [n for _, n in sym]
    prog = program(L)
    meta, rows, frs, shas, o0 = [], [], [], [], None
    n_valid = n_invalid = n_minus = 0
    for name, enc, dec, valid in cases(L):
        root = prog.run({"encoded": enc, "decoded": dec})
        got, idx = {}, {}
        for i, (k, v, _, _) in enumerate(compare.flat_walk_kept(root, prog.templates_src)):
            assert k not in got, k
            got[k], idx[k] = v, i + 1
        assert valid is None or got["main.isValid"] == valid, (name, got["main.isValid"])
        row = np.zeros(len(names), dtype="<i8")
        row[0] = 1
        comp, h = None, None
        for slot, nm in enumerate(names[1:], 1):
            v = got[nm]
            hc = ct.hash_component(nm)
            if hc is not None and L != ct.FULL_HASH:
                if hc != comp:
                    if h is not None:
                        shas.append(h.digest())
                    comp, h = hc, hashlib.sha256()
                h.update(v.to_bytes(32, "little"))
                row[slot] = ct.HS
            elif ct.field_slot(nm):
                frs.append(v.to_bytes(32, "little"))
                row[slot] = ct.FR
            else:
                row[slot] = ct.encode(v, got[nm[:-3] + "in"] if nm.endswith(".inv") else None)
        if h is not None:
            shas.append(h.digest())
        if o0 is None:
            o0 = np.array([0] + [idx[nm] for nm in names[1:]], dtype=np.uint32)
        if name.startswith("batch_"):      # the batch's mix, from the interpreter's results alone
            sr = [got[f"main.shouldRemove[{i}]"] for i in range(L)]
            n_valid += got["main.isValid"]; n_invalid += 1 - got["main.isValid"]; n_minus += int(ct.P - 1 in sr)
            assert [s if s < 2 else s - ct.P for s in sr] == ct.should_remove(enc), name
        meta.append({"name": name, "encoded": enc, "decoded": dec})
        rows.append(row)
    if L == ct.BATCH:
        assert n_valid >= 40 and n_invalid >= 40 and n_minus >= 10, (n_valid, n_invalid, n_minus)
        print(f"  batch: {n_valid} valid, {n_invalid} invalid, {n_minus} with a shouldRemove of -1")
    return dict(cases=np.frombuffer(json.dumps(meta, separators=(",", ":")).encode(), dtype=np.uint8),
                codes=np.frombuffer(zlib.compress(np.concatenate(rows).tobytes(), 9), dtype=np.uint8),
                fr=np.frombuffer(b"".join(frs), dtype=np.uint8), comp_sha=np.frombuffer(b"".join(shas), dtype=np.uint8),
                o0_index=np.frombuffer(zlib.compress(np.diff(o0, prepend=np.uint32(0)).astype('<u4').tobytes(), 9), dtype=np.uint8),
                sym_sha256=np.frombuffer(ct.sym_hash(sym).encode(), dtype=np.uint8), W=np.array([len(names)], dtype=np.uint64))


def main(argv=None):
    check = "--check" in (sys.argv[1:] if argv is None else argv)
    os.makedirs(ct.GOLDEN, exist_ok=True)
    bad = 0
    for L in ct.SHAPES:
        arrays = build(L)
        path = os.path.join(ct.GOLDEN, ct.fixture_name(L))
        if check:      # every stored array byte for byte (the archive itself carries a time stamp)
            same = os.path.exists(path)
            if same:
                z = np.load(path)
                same = sorted(z.files) == sorted(arrays) and all(z[k].dtype == v.dtype and z[k].tobytes() == v.tobytes() for k, v in arrays.items())
            bad += not same
            print(f"{os.path.basename(path)}: {'current' if same else 'DIFFERS'}")
        else:
            np.savez(path, **arrays)
            print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes")
            assert os.path.getsize(path) <= 715467
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
