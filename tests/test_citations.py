"""Every `file:line` citation of a reference file in the documentation, the C-ABI header and the product sources
must point inside that file.  The reference checkout's files and line counts are recorded in
tests/golden/reference_lines.json (tests/golden/make_reference_index.py), so the check runs without the checkout;
where the checkout is present, the record is checked against it first."""
import json
import os
import re

import pytest

from conftest import ROOT

REF = "/root/reference"
DOCS = ["DESIGN.md", "INTEGRATION.md", "README.md", "BASELINE.md", "include/zkwg.h"]
SRC_DIRS = ["zk-email-verify_amd/csrc", "zk-email-verify_amd/py/zkwg", "zk-email-verify_amd/js", "oracle/pyref", "oracle/c"]
CITE = re.compile(r"([A-Za-z0-9_./@-]+\.(?:circom|ts|md|yml|sol|json)):(\d+)(?:-(\d+))?")


INDEX = os.path.join(ROOT, "tests", "golden", "reference_lines.json")


def reference_lines(root):
    """{path relative to the checkout: line count} of every file a citation can name (node_modules and .git left out)"""
    out = {}
    for d, _, files in os.walk(root):
        if "/node_modules" in d or "/.git" in d:
            continue
        for f in files:
            if CITE.fullmatch(f + ":1"):
                p = os.path.join(d, f)
                with open(p, "rb") as fh:
                    out[os.path.relpath(p, root)] = fh.read().count(b"\n") + 1
    return out


def test_cited_reference_lines_exist():
    recorded = json.load(open(INDEX))
    if os.path.isdir(REF):
        assert reference_lines(REF) == recorded
    index = {}
    for p in recorded:
        index.setdefault(os.path.basename(p), []).append(p)

    def nlines(p):
        return recorded[p]

    files = [os.path.join(ROOT, d) for d in DOCS]
    for sd in SRC_DIRS:
        for d, _, fs in os.walk(os.path.join(ROOT, sd)):
            files += [os.path.join(d, f) for f in fs if f.endswith((".h", ".hip", ".py", ".js", ".c"))]
    bad, checked = [], 0
    for path in files:
        text = open(path, errors="replace").read()
        for m in CITE.finditer(text):
            name, lo, hi = m.group(1), int(m.group(2)), int(m.group(3) or m.group(2))
            base = os.path.basename(name)
            cands = [p for p in index.get(base, []) if p.endswith(name.lstrip("./")) or "/" not in name]
            if not cands:
                continue                       # not a reference file (our own file, or an [EXT] package)
            checked += 1
            if not any(lo <= hi <= nlines(p) for p in cands):
                bad.append(f"{os.path.relpath(path, ROOT)}: {m.group(0)}")
    assert checked > 200
    assert not bad, bad[:20]
