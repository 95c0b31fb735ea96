"""Writes tests/golden/substring/*.npz: inputs and expected witnesses of the substring mains
(RevealSubstring, CountSubstringOccurrences), computed by executing the reference's templates with the circom
interpreter (oracle/circom).  CPU only; needs the reference tree.  Per shape one file with
  cases       JSON: [{name, inputs, status}] (status 4: the interpreter raised "Assert Failed")
  witness     zlib of one int64 code per slot (tests/substrtest.py) of every status-0 case, in case order, slot order
  o0_index    zlib of the O0 index of every slot as uint32 differences to the slot before
  sym_sha256  SHA-256 of the slot names joined by newlines
  W           slots per witness
The slot names come from a layout-only zkwg handle; values and O0 indices are looked up by name in the interpreter's walk.

    python tests/golden/make_substring_fixtures.py [--check]
"""
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

import substrtest as st  # noqa: E402
from oracle.circom import ev, compare, AssertFailed  # noqa: E402
from oracle.circom.runtime import Program  # noqa: E402

TC = "tests/test-circuits/"
# the three anonymous LessThan call sites of RevealSubstring (helpers/reveal-substring.circom:23, :27, :32)
ANON = {("RevealSubstring", "LessThan", 0): "anon_LessThan_start", ("RevealSubstring", "LessThan", 1): "anon_LessThan_length",
        ("RevealSubstring", "LessThan", 2): "anon_LessThan_sum"}


def program(kind, L, S, u):
    if (kind, L, S, u) == (st.REVEAL, 256, 16, 1):
        return ev.program(TC + "reveal-substring-test.circom", track_how=True)
    if (kind, L, S) == (st.COUNT, 1024, 128):
        return ev.program(TC + "count-substring-occurrences-test.circom", track_how=True)
    p = Program(None, ev.include_paths(), track_how=True)    # the same mains with other parameters
    if kind == st.REVEAL:
        p.load(os.path.join(ev.REF_CIRCUITS, "helpers", "reveal-substring.circom"))
        p.main = ([], "RevealSubstring", [("num", v) for v in (L, S, u)])
    else:
        p.load(os.path.join(ev.REF_CIRCUITS, "utils", "array.circom"))
        p.main = ([], "CountSubstringOccurrences", [("num", v) for v in (L, S)])
    return p


def pad(v, n):
    v = list(v)
    assert len(v) <= n
    return v + [0] * (n - len(v))


def reveal_cases(L, S, u):
    """reveal-substring.test.ts for (256, 16, 1); the project's own cases for every shape"""
    out = []
    add = lambda name, in_, start, length: out.append((name, {"in": pad(in_, L), "substringStartIndex": start, "substringLength": length}))
    if (L, S, u) == (256, 16, 1):
        ramp = [(i % 255) + 1 for i in range(100)]
        for name, a, b in (("middle", 50, 5), ("start", 0, 5), ("end_of_nonzero", 95, 5), ("length_1", 50, 1), ("maximum_length", 0, 16),
                           ("zero_padded", 0, 3)):
            add("ref_" + name, ramp, a, b)
        for name, a, b in (("start_eq_max", 256, 1), ("start_gt_max", 257, 1), ("length_eq_max", 0, 16), ("length_gt_max", 0, 17),
                           ("sum_gt_max", 250, 7)):
            add("ref_fail_" + name, [1] * 256, a, b)
    rng = random.Random(1000 * L + 10 * S + u)
    text = [rng.randrange(1, 256) for _ in range(L)]
    text[L - S:] = [200 + (i % 50) for i in range(S)]          # a tail unlike the rest, bytes >= 128
    add("own_sum_eq_max", text, L - S, S)                       # start + length = maxLength exactly, full length, no zero byte
    add("own_sum_one_more", text, L - S + 1, S)
    add("own_full_length", [7] * 3 + list(range(1, S + 1)) + [9] * 5, 3, S)
    add("own_high_bytes", [0, 255, 128, 0, 255, 255, 128, 1], 1, 2)       # (0 - 255) 255, (255 - 128) 128 among the differences
    add("own_overlap", [5, 5, 5, 6, 5, 5], 0, 2)               # 5,5 occurs at 0, 1, 4
    add("own_length_zero", text, 4, 0)                          # substring[0] = 0
    add("own_reveals_zero_first", [0, 3, 4], 0, 2)             # substring[0] = 0 with a non-zero length
    add("own_tail_window", [0] * (L - 2) + [9, 4], L - 2, 2)   # the match's window runs past the end of in[]
    add("own_last_byte", [0] * (L - 1) + [77], L - 1, 1)
    if (L, S, u) == (64, 8, 1):
        # 130 seeded emails; a duplicate of the revealed bytes is planted in at most a quarter
        for k in range(130):
            r = random.Random(7919 * k + 1)
            in_ = [r.randrange(1, 256) for _ in range(L)]
            n = r.randrange(1, S + 1)
            a = r.randrange(0, L - n + 1)
            if k % 4 == 3 and n <= 4:
                b = (a + n + r.randrange(0, L - 2 * n + 1)) % (L - n + 1)
                if abs(b - a) >= n:
                    in_[b:b + n] = in_[a:a + n]
            add(f"batch_{k}", in_, a, n)
    return out


def count_cases(L, S):
    """count-substring-occurrences.test.ts for (1024, 128); the project's own cases for every shape"""
    out = []
    add = lambda name, in_, sub: out.append((name, {"in": pad(in_, L), "substring": pad(sub, S)}))
    if (L, S) == (1024, 128):
        add("ref_single_at_start", [1, 2, 3, 4, 5], [1, 2, 3])
        add("ref_multiple", [1, 2, 3, 4, 1, 2, 3, 5, 1, 2, 3], [1, 2, 3])
        add("ref_none", [1, 2, 4, 5, 6], [1, 2, 3])
        add("ref_overlap", [1, 1, 1, 2, 1, 1], [1, 1])
        add("ref_full_match", [1, 2, 3, 4] * 256, [1, 2, 3, 4])
        add("ref_single_char", [1, 2, 1, 3, 1, 4, 1], [1])
        add("ref_at_end", [0] * 1021 + [1, 2, 3], [1, 2, 3])
        add("ref_fail_empty_substring", [1, 2, 3, 4, 5], [])
        add("own_high_bytes_full", [255] * 300 + [128] * 300 + [1] * 424, [255] * 64 + [128] * 64)
        return out
    rng = random.Random(100 * L + S)
    text = [rng.randrange(1, 256) for _ in range(L)]
    add("own_full_length", text, text[5:5 + S] if L > S else text)
    add("own_tail_match", [0] * (L - 2) + [9, 4], [9, 4])                  # matches against the zero fill past the end
    add("own_tail_no_match", [0] * (L - 2) + [9, 4], [9, 4, 1])            # the same window, the rest of the substring is not zero
    add("own_overlap", [5] * min(L, 9), [5, 5, 5])
    add("own_high_bytes", [0, 255, 128, 0, 255, 255, 128, 1], [255, 128])
    add("own_first_zero", text, [0, 1, 2])
    add("own_zero_inside", [3, 0, 4, 3, 9, 4], [3, 0, 4])                  # a zero byte of the substring matches anything
    add("own_all_255", [255] * L, [255] * S)
    return out


def build(kind, L, S, u):
    import zkwg
    compare.KEPT_V1_ANON.update(ANON)
    c = zkwg.Circuit(device=-1, **st.circuit_kwargs(kind, L, S, u))
    sym = c.symbols()
    names = [n for _, n in sym]
    prog = program(kind, L, S, u)
    cases, rows, o0 = [], [], None
    for name, inp in (reveal_cases(L, S, u) if kind == st.REVEAL else count_cases(L, S)):
        try:
            root = prog.run(inp)
        except AssertFailed:
            cases.append({"name": name, "inputs": inp, "status": 4})
            continue
        got, idx = {}, {}
        for i, (k, v, _, _) in enumerate(compare.flat_walk_kept(root, prog.templates_src)):
            assert k not in got, k
            got[k], idx[k] = v, i + 1
        row = np.zeros(len(names), dtype="<i8")
        row[0] = 1
        for slot, nm in enumerate(names[1:], 1):
            v = got[nm]
            row[slot] = st.encode(v, got[nm[:-3] + "in"] if nm.endswith(".inv") else None)
        if o0 is None:
            o0 = np.array([0] + [idx[nm] for nm in names[1:]], dtype=np.uint32)
        cases.append({"name": name, "inputs": inp, "status": 0})
        rows.append(row)
    batch = [cs for cs in cases if cs["name"].startswith("batch_")]
    if batch:      # at least three quarters of the seeded batch are status-0 witnesses, by the interpreter's results alone
        assert len(batch) == 130 and 4 * sum(cs["status"] == 0 for cs in batch) >= 3 * len(batch)
    blob = zlib.compress(np.concatenate(rows).tobytes(), 9)
    return dict(cases=np.frombuffer(json.dumps(cases, separators=(",", ":")).encode(), dtype=np.uint8),
                witness=np.frombuffer(blob, dtype=np.uint8),
                o0_index=np.frombuffer(zlib.compress(np.diff(o0, prepend=np.uint32(0)).astype('<u4').tobytes(), 9), dtype=np.uint8),
                sym_sha256=np.frombuffer(st.sym_hash(sym).encode(), dtype=np.uint8), W=np.array([len(names)], dtype=np.uint64))


def main(argv=None):
    check = "--check" in (sys.argv[1:] if argv is None else argv)
    os.makedirs(st.GOLDEN, exist_ok=True)
    bad = 0
    for shape in st.SHAPES:
        arrays = build(*shape)
        path = os.path.join(st.GOLDEN, st.fixture_name(*shape))
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
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
